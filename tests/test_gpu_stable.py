"""Filter-level `stable=True` (LDL^T completion, mfs/utils.py:495-538 through mfs/one_dim/filtering.py:77,82 and
mfs/multi_dims/filtering.py) on the device against `oracle.moment_filter_*(..., stable=True)`:

  * on well-posed input the completed factor IS the Cholesky factor: stable=True equals stable=False;
  * an initial moment vector whose Hankel / Gram matrix has a NEGATIVE LDL^T pivot actually triggers the `eps`
    completion (R = L diag(d < 0 ? eps : sqrt(d)), eps = 1e-8 ||G||_F, :525-538): stable=False poisons at step 0,
    stable=True runs on and matches the oracle.
"""
import os

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import synth
from mfs_amd.multi_dims import filtering as fnd
from oracle import multi_dims as omd, one_dim as o, parity
from tests.nd_envelope_models import prey_predator, prey_predator_oracle
from tests.one_dim_support import MODES, benes, run_device, run_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('mode', MODES)
def test_1d_stable_filter_matches_oracle_and_plain_filter(mode):
    N, T, B = 5, 60, 3
    model = benes(N, 'tme', 2)
    ys, _ = synth.benes_bernoulli_batch(B, T, model.dt, seed=11)
    ref = run_oracle(mode, model, ys, stable=True)
    got, plain = run_device(mode, model, ys, stable=True), run_device(mode, model, ys, stable=False)
    for b in range(B):
        npt.assert_allclose(got.nell[b], ref.nell[b], rtol=1e-6)
        assert parity.rel_err(got.moments[b], ref.moments[b], parity.moment_floor(ref.moments[b])).max() <= 1e-6
        for e, r in zip(got[1:3], ref[1:3]):
            if e is not None:
                npt.assert_allclose(e[b], r[b], rtol=1e-6, atol=1e-9)
    # Cholesky == completed LDL^T on positive definite input (reference tests/test_utils.py:198-209, at filter level)
    npt.assert_allclose(got.nell, plain.nell, rtol=1e-9)
    assert parity.rel_err(got.moments, plain.moments, parity.moment_floor(plain.moments)).max() <= 1e-7


def test_1d_stable_completes_an_indefinite_start():
    """cms0 with E[(x - m)^4] < E[(x - m)^2]^2: the 3 x 3 Hankel matrix has LDL^T pivots (1, 0.3, < 0)."""
    N, T = 3, 40
    model = benes(N, 'tme', 2)
    cms0 = np.array([1., 0., 0.3, 0.01, 0.05, 0.002])      # 0.05 < 0.3^2: not a moment sequence
    start = model.start._replace(cms=cms0, mean=0.1)
    G = cms0[np.add.outer(np.arange(N), np.arange(N))]
    _, dpiv = o.ldl(G)
    assert dpiv.min() < 0.                                   # the completion branch is taken at the first rule
    ys, _ = synth.benes_bernoulli_batch(2, T, model.dt, seed=2)
    m, means, _, nell, fn = run_device('central', model, ys, start=start, stable=True, return_first_nan=True)
    compared = 0
    for b in range(2):
        r = run_oracle('central', model, ys[b:b + 1], start=start, stable=True)
        # A completed rule carries a node at ~1e13 with a negligible weight: from then on the filter effectively runs on
        # N - 1 atoms, the next Hankel matrix is singular to rounding, and whether its last pivot lands at -1e-17 (completed
        # again), +1e-17 or exactly 0 (singular solve: NaN in-band) is rounding luck on either side.  What the filter
        # delivers in that regime is the NLL, the mean and the variance; the top moments are ~1e26 noise.
        if not np.isfinite(r.nell[0]):
            continue
        compared += 1
        assert fn[b] == -1
        npt.assert_allclose(nell[b], r.nell[0], rtol=1e-6)
        npt.assert_allclose(means[b], r.means[0], rtol=1e-6, atol=1e-9)
        npt.assert_allclose(m[b, :, 2], r.moments[0][:, 2], rtol=1e-6)
        npt.assert_allclose(m[b, 3:, 3], r.moments[0][3:, 3], rtol=1e-5, atol=1e-9)
    assert compared >= 1
    # without the completion the same start poisons at once, as the reference's Cholesky does
    _, _, _, nell0, fn0 = run_device('central', model, ys, start=start, stable=False, return_first_nan=True)
    assert np.all(fn0 == 0) and np.all(np.isnan(nell0))
    assert np.isnan(run_oracle('central', model, ys[:1], start=start, stable=False).nell[0])


@pytest.mark.parametrize('family', ['tme_2', 'tme_normal_2'])
def test_nd_stable_filter(family):
    N, T, B = 3, 40, 2
    mi, inds, dt, gs, fns, sig, pmf, ogs, opmf = prey_predator(N, family)
    ocms, omean = prey_predator_oracle(N, family)
    ys, _ = synth.prey_predator_batch(B, T, dt, seed=9)
    # well-posed start: completion == Cholesky
    cs, ms, ns = fnd.moment_filter_nd_cms((fns[1], sig), fns[3], pmf, ys, (mi, inds), gs.cms, gs.mean, stable=True)
    cp, mp, np_ = fnd.moment_filter_nd_cms((fns[1], sig), fns[3], pmf, ys, (mi, inds), gs.cms, gs.mean, stable=False)
    npt.assert_allclose(ns, np_, rtol=1e-9)
    npt.assert_allclose(ms, mp, rtol=1e-9)
    r = omd.moment_filter_nd_cms((ocms, sig), omean, opmf, ys[0], (mi, inds), ogs.cms, ogs.mean, stable=True)
    npt.assert_allclose(ns[0], r[2], rtol=1e-6)
    npt.assert_allclose(ms[0], r[1], rtol=1e-6)
    # indefinite start: shrink the fourth-order moments until the Gram matrix has a negative pivot
    bad = gs.cms.copy()
    bad[mi.sum(axis=1) == 4] *= 0.2
    _, dpiv = o.ldl(bad[inds[0]])
    assert dpiv.min() < 0.
    cb, mb, nb, fnb = fnd.moment_filter_nd_cms((fns[1], sig), fns[3], pmf, ys, (mi, inds), bad, gs.mean, stable=True,
                                               return_first_nan=True)
    rb = omd.moment_filter_nd_cms((ocms, sig), omean, opmf, ys[0], (mi, inds), bad, ogs.mean, stable=True)
    if np.isfinite(rb[2]):
        assert fnb[0] == -1
        npt.assert_allclose(nb[0], rb[2], rtol=1e-6)
        npt.assert_allclose(mb[0], rb[1], rtol=1e-6)
    else:   # the completed rule may still be too far from a distribution for the filter to continue: same fate on both sides
        assert fnb[0] >= 0
    _, _, n0, fn0 = fnd.moment_filter_nd_cms((fns[1], sig), fns[3], pmf, ys, (mi, inds), bad, gs.mean, stable=False,
                                             return_first_nan=True)
    assert np.all(fn0 == 0) and np.all(np.isnan(n0))


@pytest.mark.parametrize('degree,shrink', [(8, 0.8), (4, 0.2)])
def test_nd_stable_register_front_end_against_the_dense_form_and_the_oracle(monkeypatch, degree, shrink):
    """stable=True on the N-D kernel's register front end (the completed factor only rescales rows and columns of the
    block-tridiagonal T = L^-1 (P_k L+), csrc/filternd_kernel.hpp front_nd) against (i) the LDS-tile form of the same
    completion, MFS_ND_STABLE=dense, which forms the dense K_k like quadratures.py:151-161, and (ii) the NumPy oracle with
    ldl=True, at N = 5 from starts whose Gram matrix has a negative pivot (mfs/utils.py:525-538 takes the eps branch): the
    moments of one degree shrunk -- degree 8 by 0.8 (pivot -1e-12: two of the three replicates run all T steps in the oracle)
    and degree 4 by 0.2 (pivot -8e-7: every implementation loses the replicate within five steps).  Compared on the steps
    before any of the three implementations is within two steps of losing the replicate (measured on those steps: register
    form 1e-10 .. 4e-9 from the oracle on the moments, LDS-tile form 2e-9 .. 8e-8)."""
    N, T, B = 5, 30, 3
    mi, inds, dt, gs, fns, sig, pmf, ogs, opmf = prey_predator(N)
    ocms, omean = prey_predator_oracle(N)
    ys, _ = synth.prey_predator_batch(B, T, dt, seed=11)
    bad = gs.cms.copy()
    bad[mi.sum(axis=1) == degree] *= shrink
    _, dpiv = o.ldl(bad[inds[0]])
    assert dpiv.min() < 0.
    run = lambda: fnd.moment_filter_nd_cms((fns[1], sig), fns[3], pmf, ys, (mi, inds), bad, gs.mean, stable=True,
                                           return_first_nan=True)
    cf, mf, nf, fnf = run()
    monkeypatch.setenv('MFS_ND_STABLE', 'dense')
    cd, md, nd_, fnd_ = run()
    monkeypatch.delenv('MFS_ND_STABLE')
    steps = lambda fn: T if fn < 0 else int(fn)
    compared = full = 0
    for b in range(B):
        rb = omd.moment_filter_nd_cms((ocms, sig), omean, opmf, ys[b], (mi, inds), bad, ogs.mean, stable=True)
        fin = np.isfinite(rb[1]).all(axis=1)
        ko = T if fin.all() else int(np.argmin(fin))
        ks = (steps(fnf[b]), steps(fnd_[b]), ko)
        # the same fate; WHEN a lost replicate goes differs by a few steps between any two implementations (measured here:
        # 4 / 5 / 8 for register form / LDS-tile form / oracle) -- its last two steps are ill-conditioned on every side
        assert len({kk == T for kk in ks}) == 1, ks
        k = T if min(ks) == T else min(ks) - 2
        if k < 1:
            continue
        compared += 1
        npt.assert_allclose(mf[b, :k], md[b, :k], rtol=1e-6)
        npt.assert_allclose(mf[b, :k], rb[1][:k], rtol=1e-6)
        floor = parity.natural_magnitude_nd(rb[0][:k], mi)
        assert parity.rel_err(cf[b, :k], rb[0][:k], floor).max() <= 1e-5
        assert parity.rel_err(cf[b, :k], cd[b, :k], floor).max() <= 1e-5
        if k == T:
            full += 1
            npt.assert_allclose(nf[b], rb[2], rtol=1e-6)
            npt.assert_allclose(nf[b], nd_[b], rtol=1e-6)
    assert compared >= 2 and (full >= 1 or degree == 4)


def test_config2_stable_runs_the_fast_kernel_and_matches_the_oracle_golden():
    """Config 2 (N = 15, TME-3, central) with stable=True on the 64 golden replicates x 300 steps against the frozen
    `oracle.moment_filter_cms(..., stable=True)` (tests/golden/filter_cfg2stable.npz, make_filter_golden.py cfg2stable).

    The completion only changes a rule whose LDL^T has a pivot that is not > 0 (mfs/utils.py:535-538); until a replicate's
    first such rule the stable run IS the plain run -- bit for bit on the device, which also shows that stable=True stays on
    the register-resident kernel -- and within 1e-6 of the oracle.  After a completion no two fp64 implementations of the
    reference stay within 1e-6 of each other on every replicate (the dense K of a completed factor carries rounding noise
    amplified by 1 / eps^2; NumPy oracle vs C port: variance 1.8e-4, mean 1e-5 on these replicates): there the NLL is held to
    1e-4, mean and variance to 1e-2; each to 1e-6 on half of those replicates and to 1e-4 on three quarters, and the survivor counts
    must agree."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'filter_cfg2stable.npz'))
    N, T, B = int(g['N']), int(g['T']), int(g['B'])
    ys = np.unpackbits(g['ys_bits'], axis=1)[:, :T].astype(np.float64)
    model = benes(N, 'tme', 3)
    sm, smean, _, snell, sfn = run_device('central', model, ys, stable=True, return_first_nan=True)
    pm, pmean, _, pnell, pfn = run_device('central', model, ys, stable=False, return_first_nan=True)
    first = np.where(pfn >= 0, pfn, T)             # the step of a replicate's first completed rule = where the plain run poisons
    gp = g['central_first_completion']
    ofirst = np.where(gp >= 0, gp, T)              # ... and the step of the ORACLE's first completed rule (its own rounding: the
                                                   # reference's explicit LDL^T loop, not LAPACK's potrf, decides there)
    gvar, gmean, gnell, gfn = g['central_variances'], g['central_means'], g['central_nell'], g['central_first_nan']
    ex = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'filter_cfg2_exact_B64.npz'))
    assert np.array_equal(ex['ys_bits'], g['ys_bits'])
    xmean, xvar, xnell = ex['central_means'], ex['central_variances'], ex['central_nell']
    xfirst = np.where(ex['central_first_nan'] >= 0, ex['central_first_nan'], T)
    clean = late = 0
    worst_var, worst_mean, worst_nll = [], [], []
    for b in range(B):
        k = int(first[b])
        # (i) before the first completion: the plain run, bit for bit, and the oracle to 1e-6 (until ITS first completion)
        assert np.array_equal(sm[b, :k], pm[b, :k]) and np.array_equal(smean[b, :k], pmean[b, :k])
        # ... and, up to there, the reference's algorithm in exact arithmetic to 1e-6 (filter_cfg2_exact_B64.npz: the same 64
        # replicates at 80 digits; the NumPy oracle itself is 2e-6 / 3e-5 off on mean / variance where cond(Hankel) >= 1e15)
        kx = min(k, int(xfirst[b]))
        assert parity.rel_err(smean[b, :kx], xmean[b, :kx], np.sqrt(xvar[b, :kx])).max(initial=0.) <= 1e-6
        npt.assert_allclose(sm[b, :kx, 2], xvar[b, :kx], rtol=1e-6)
        k = min(k, int(ofirst[b]))
        if k == T:
            clean += 1
            assert snell[b] == pnell[b]
            if xfirst[b] == T:
                npt.assert_allclose(snell[b], xnell[b], rtol=1e-6)
            continue
        # (ii) after it, where both are finite
        both = np.isfinite(sm[b, :, 2]) & np.isfinite(gvar[b])
        if np.isfinite(snell[b]) and np.isfinite(gnell[b]):
            late += 1
            npt.assert_allclose(snell[b], gnell[b], rtol=1e-4)
            worst_nll.append(abs(snell[b] - gnell[b]) / abs(gnell[b]))
        worst_var.append(np.max(parity.rel_err(sm[b, both, 2], gvar[b, both]), initial=0.))
        worst_mean.append(np.max(parity.rel_err(smean[b, both], gmean[b, both], 1e-12), initial=0.))
    worst_var, worst_mean = np.array(worst_var), np.array(worst_mean)
    assert clean >= 32 and late >= 8
    assert worst_var.max() <= 1e-2 and worst_mean.max() <= 1e-2
    for w_ in (worst_var, worst_mean, np.array(worst_nll)):
        assert np.median(w_) <= 1e-6 and np.mean(w_ <= 1e-4) >= 0.75
    # (iii) survivors: the completion keeps nearly every replicate alive, on both sides
    alive_dev, alive_ora, alive_plain = int((sfn < 0).sum()), int((gfn < 0).sum()), int((pfn < 0).sum())
    assert alive_dev >= alive_plain + 10 and alive_ora - 3 <= alive_dev   # (the device loses fewer replicates to rounding, as in plain mode)
