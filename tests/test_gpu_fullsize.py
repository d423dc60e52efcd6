"""BASELINE.json's configurations at FULL size, checked through size-independent properties (the oracle cannot run
4e6 filter-steps in seconds): exact Kalman agreement (config 3), NaN-poisoning structure, normalisation invariants,
replicate-order invariance, survivors' NLL against the C port on a sample (config 2), NLL grid consistency (config 4)."""
import math
import os

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import synth
from mfs_amd.multi_dims import filtering as fnd
from mfs_amd.one_dim import filtering
from oracle import c_oracle, parity
from tests.nd_envelope_models import prey_predator
from tests.one_dim_support import assert_poisoned_after, benes, benes_operator_tables, ou_gaussian, run_device, well

pytestmark = pytest.mark.gpu


def test_config2_benes_bernoulli_full_size():
    """Benes--Bernoulli N = 15, T = 1000, B = 4096, central, TME-3 (BASELINE configs[1])."""
    N, T, B = 15, 1000, 4096
    model = benes(N)
    ys, _ = synth.benes_bernoulli_batch(B, T, model.dt, seed=100)
    m, means, _, nell, fn = run_device('central', model, ys, return_first_nan=True)
    assert_poisoned_after(m, means, nell, fn)
    live = np.where(fn >= 0, fn, T)
    assert 0.3 < live.sum() / (B * T) < 0.9          # a large share survives, a large share poisons (SURVEY hard part 3)
    # normalisation invariants on live steps: cms[0] = 1, cms[1] = 0 (to rounding), variance > 0
    t = np.arange(T)[None, :]
    ok = t < live[:, None]
    npt.assert_allclose(m[..., 0][ok], 1., atol=1e-9)
    assert np.abs(m[..., 1][ok]).max() < 1e-9
    assert np.all(m[..., 2][ok] > 0)
    # replicate-order invariance, bit for bit
    perm = np.random.default_rng(0).permutation(B)[:257]
    m2, means2, _, nell2, _ = run_device('central', model, ys[perm])
    npt.assert_array_equal(nell2, nell[perm])
    npt.assert_array_equal(means2, means[perm])
    # survivors against the C port of the oracle on a sample of replicates
    nb = 192
    oic = model.oic
    _, cmeans, _, cnell = c_oracle.filter_1d(1, N, ys[:nb], oic.cms, oic.mean, None, 0, 1, 6, benes_operator_tables(N), 1.0, 0,
                                             np.array([0., 0., 0., 0.2]), want_moments=False)
    both = np.isfinite(cnell) & np.isfinite(nell[:nb])
    assert both.sum() > nb // 5
    # (the C port is itself up to 6.9e-6 from exact arithmetic on the NLL of this batch -- tests/test_oracle_golden.py -- the
    #  device 1e-10: the bulk agrees to 1e-8, the maximum is the port's own error)
    rel = np.abs(nell[:nb][both] - cnell[both]) / np.abs(cnell[both])
    assert np.quantile(rel, 0.9) <= 1e-8 and rel.max() <= 1e-5
    # NaN onset: the two implementations agree exactly for most replicates and statistically overall (measured: 76 % within
    # two steps; the two CPU implementations agree with each other on 71 %)
    c_first = np.where(np.isnan(cmeans).any(1), np.argmax(np.isnan(cmeans), 1), T)
    agree = np.mean(np.abs(c_first - live[:nb]) <= 2)
    assert agree > 0.68
    assert abs(np.mean(c_first) - np.mean(live[:nb])) < 0.1 * T
    # the worst replicates of THIS batch (largest device-vs-C-port deviations, tools/select_tails.py) against their
    # exact-arithmetic trajectories: the device within 1e-6 on every quantity at every finite step
    e = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'filter_cfg2_exact_tails.npz'))
    idx = e['central_idx']
    assert np.array_equal(np.packbits(ys[idx].astype(np.uint8), axis=1), e['central_ys_bits'])
    sc = parity.score_against_exact_tails(e, 'central', m[idx], means[idx], m[idx][..., 2], nell[idx])
    assert max(sc['max'].values()) <= 1e-6, sc['max']


@pytest.mark.parametrize('N', [5, 10, 15, 20, 25])
def test_config3_convergence_sweep_full_size(N):
    """OU / Gaussian, T = 1000, B = 1024, central, against the exact Kalman filter (BASELINE configs[2])."""
    T, B = 1000, 1024
    mdl = ou_gaussian(N)
    F, Sigma = mdl.F, mdl.Sigma
    ys, _ = synth.ou_gaussian_batch(B, T, seed=7)
    m, means, _, nell, fn = run_device('central', mdl, ys, return_first_nan=True)
    alive = fn < 0
    # cond(Hankel) reaches ~1e20 at N = 25: whether a Cholesky pivot rounds below zero within 2000 factorisations is
    # summation-order luck (measured over 256 replicates: fast path 65 % alive, dense device path 43 %, C port 45 %;
    # the NumPy/LAPACK oracle survives some replicates the others lose).  N <= 15 never poisons here.
    assert alive.mean() >= {5: 1.0, 10: 1.0, 15: 1.0, 20: 0.99, 25: 0.5}[N]
    # vectorised exact Kalman filter over the batch
    mf, vf, knell = np.zeros(B), np.full(B, mdl.var0), np.zeros(B)
    kmeans, kvars = np.empty((B, T)), np.empty((B, T))
    for k in range(T):
        mp, vp = F * mf, F * vf * F + Sigma
        s = vp + 1.
        g = vp / s
        knell += 0.5 * np.log(2 * math.pi * s) + 0.5 * (ys[:, k] - mp) ** 2 / s
        mf, vf = mp + g * (ys[:, k] - mp), vp - vp * g
        kmeans[:, k], kvars[:, k] = mf, vf
    # the N-point rule is exact for the Gaussian posterior only asymptotically: the error of the N = 5 filter is
    # dominated by rare large innovations, so the bound is on the worst case over 1e6 steps, per N
    err_mean = np.abs(means[alive] - kmeans[alive]).max()
    err_var = np.abs(m[alive][..., 2] - kvars[alive]).max()
    err_nell = np.abs(nell[alive] / knell[alive] - 1.).max()
    print(f'N={N}: alive {alive.mean():.4f}  max|mean-KF| {err_mean:.3e}  max|var-KF| {err_var:.3e}  '
          f'max rel NLL {err_nell:.3e}')
    tol_mean = {5: 1e-1, 10: 1e-3, 15: 1e-5, 20: 1e-6, 25: 1e-6}[N]
    assert err_mean < tol_mean and err_var < tol_mean
    assert err_nell < {5: 1e-3, 10: 1e-5, 15: 1e-7, 20: 1e-8, 25: 1e-8}[N]


def test_config4_nll_grid_per_replicate_theta():
    """Well--Poisson NLL grid (BASELINE configs[3], per-GPU shard shape scaled down): theta per replicate, NLL only.
    Grid points sharing a theta give identical NLLs; the C port agrees on a sample."""
    N, T = 7, 1000
    g1, g2 = np.meshgrid(np.linspace(0.5, 6., 32), np.linspace(0.5, 6., 16), indexing='ij')
    keys = 4
    p1 = np.tile(g1.ravel(), keys)
    p2 = np.tile(g2.ravel(), keys)
    B = p1.shape[0]
    grid = well(N, tuple(p1), 'tme_normal', 2, tuple(p2))
    ys_k, _ = synth.well_poisson_batch(keys, T, p1=3., p2=3., dt=grid.dt, seed=5)
    ys = np.repeat(ys_k, g1.size, axis=0)
    m, means, _, nell, fn = run_device('central', grid, ys, return_first_nan=True)
    assert np.isfinite(nell).mean() > 0.5
    # duplicate the first 64 grid points at the end of the batch: same theta, same data -> same NLL, bit for bit
    idx = np.arange(64)
    head = well(N, tuple(p1[idx]), 'tme_normal', 2, tuple(p2[idx]))
    nell2 = run_device('central', head, ys[idx]).nell
    npt.assert_array_equal(nell2, nell[idx])
    # the C port on a sample (tables from the product here: the SymPy route is checked in test_abi_and_host.py)
    tables, lik = filtering.trace_model('central', head.fns[1], head.fns[3], head.pmf)
    coef, _ = tables.table(64)
    _, _, _, cnell = c_oracle.filter_1d(1, N, ys[idx], head.ic.cms, head.ic.mean, None, 1, 0, 0, coef, tables.mean_x_coef, 1,
                                        lik.params, want_moments=False)
    both = np.isfinite(cnell) & np.isfinite(nell2)
    assert both.sum() >= 32
    npt.assert_allclose(nell2[both], cnell[both], rtol=1e-6)
    # the NLL surface has its minimum near the data-generating parameters for each data set
    surf = np.where(np.isfinite(nell), nell, np.inf).reshape(keys, 32, 16)
    for k in range(keys):
        i, j = np.unravel_index(np.argmin(surf[k]), surf[k].shape)
        assert 1.0 < g1[i, j] < 6.0 and 1.5 < g2[i, j] < 5.0


def test_config5_length_nd_modes_agree():
    """BASELINE config 5 at full length (d = 2, N = 6, T = 500) on a slice of the batch: no oracle can follow 500 steps
    of it in test time, so the size-independent property is the reference's own one (tests/test_filtering.py:168-242):
    the central and the scaled-central filters carry the same means and NLL."""
    N, T, B = 6, 500, 48
    mi, inds, dt, gs, fns, _, pmf, _, _ = prey_predator(N, 'tme_2')
    ys, _ = synth.prey_predator_batch(B, T, dt, seed=77)
    cmss, means_c, nell_c, fn = fnd.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], pmf, ys, (mi, inds), gs.cms,
                                                         gs.mean, return_first_nan=True)
    scale0 = np.sqrt(np.array([gs.cms[5], gs.cms[3]]))
    scmss, means_s, scales, nell_s = fnd.moment_filter_nd_scms((fns[2], 'multi-index'), fns[4], pmf, ys, (mi, inds),
                                                               gs.cms / np.prod(scale0 ** mi, axis=-1), gs.mean, scale0)
    alive = fn < 0
    assert alive.mean() > 0.9
    both = alive & np.isfinite(nell_s)
    assert both.mean() > 0.9
    npt.assert_allclose(nell_s[both], nell_c[both], rtol=1e-5)
    npt.assert_allclose(means_s[both], means_c[both], rtol=1e-5)
    npt.assert_allclose(scales[both] ** 2, np.stack([cmss[both][:, :, 5], cmss[both][:, :, 3]], axis=-1), rtol=1e-3)
