"""GPU parity of the d = 3 N-D path (filternd3_kernel) against the oracle's N-D filters (oracle/multi_dims.py).

Lorenz-63 in units of 10 with operator TME-2 tables or a Normal closure, a 3-D linear-Gaussian model with three Gaussian
factors, a 3-D OU model with a Poisson factor; raw, central and scaled modes; the LDL^T completion; batch independence,
per-replicate tables, NaN poisoning and the device-pointer plan.  Only filter outputs are compared (the rule's nodes are not
unique when the K_k have repeated eigenvalues)."""
import math

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import stats, sym
from mfs_amd.multi_dims import filtering, moments
from oracle import models as om, multi_dims as omd, one_dim as o1, tme_sympy
from tests.nd3_models import C0, DT, M0, MODELS, SD, lorenz_disp, lorenz_drift, lorenz_opdf, lorenz_pdf, lorenz_ys
from tests.nd_support import assert_moments, host_disp, host_drift, initial, tables
from tests.plan_api import run_plan_nd

pytestmark = pytest.mark.gpu

_lorenz, _disp = host_drift(MODELS['lorenz']), host_disp(MODELS['lorenz'])      # the forms the host traces


def _init(mi, mean=M0, cov=C0):
    st = initial(mi, mean, cov)
    return st['cms'], st['rms']


@pytest.mark.parametrize('N,T', [(2, 30), (3, 10), (4, 3)])
def test_lorenz_operator_central_and_raw(N, T):
    mi, inds = tables(3, N)
    cms0, rms0 = _init(mi)
    fns = moments.sde_cond_moments_tme(_lorenz, _disp, DT, 2, d=3)
    ofns = tme_sympy.sde_cond_moments_tme_nd(lorenz_drift, lorenz_disp, 3, DT, 2, mi)
    B = 2
    ys = lorenz_ys(B, T, seed=N)
    cmss, means, nell = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), cms0, M0)
    assert cmss.shape == (B, T, mi.shape[0]) and means.shape == (B, T, 3) and nell.shape == (B,)
    rc = omd.moment_filter_nd_cms((ofns[1], 'multi-index'), ofns[2], lorenz_opdf, ys[0], (mi, inds), cms0, M0)
    npt.assert_allclose(nell[0], rc[2], rtol=1e-6)
    npt.assert_allclose(means[0], rc[1], rtol=1e-6)
    assert_moments(cmss[0], rc[0], mi, rtol=1e-6)
    if N <= 3:
        rmss, nell_r = filtering.moment_filter_nd_rms((fns[0], 'multi-index'), lorenz_pdf, ys, (mi, inds), rms0)
        rr = omd.moment_filter_nd_rms((ofns[0], 'multi-index'), lorenz_opdf, ys[0], (mi, inds), rms0)
        npt.assert_allclose(nell_r[0], rr[1], rtol=1e-6)
        assert_moments(rmss[0], rr[0], mi, rtol=1e-6)
        # raw and central filters agree on the device (reference tests/test_filtering.py:229-242)
        npt.assert_allclose(means[:, :, 0], rmss[:, :, 3], rtol=1e-6)
        npt.assert_allclose(nell, nell_r, rtol=1e-6)


@pytest.mark.parametrize('N,T', [(2, 20), (3, 6)])
def test_lorenz_operator_scaled(N, T):
    mi, inds = tables(3, N)
    cms0, _ = _init(mi)
    scale0 = np.sqrt(np.diag(C0))
    scms0 = cms0 / np.prod(scale0 ** mi, axis=-1)
    fns = moments.sde_cond_moments_tme(_lorenz, _disp, DT, 2, d=3)
    _, ocms, _, omean_var = tme_sympy.sde_cond_moments_tme_nd(lorenz_drift, lorenz_disp, 3, DT, 2, mi)

    def oscms(x, idx, mean, scale):
        return ocms(x, idx, mean) / np.prod(np.asarray(scale) ** np.asarray(idx), axis=-1)

    ys = lorenz_ys(2, T, seed=20 + N)
    scmss, means, scales, nell = filtering.moment_filter_nd_scms((fns[2], 'multi-index'), fns[4], lorenz_pdf, ys, (mi, inds),
                                                                 scms0, M0, scale0)
    assert scales.shape == (2, T, 3)
    rs = omd.moment_filter_nd_scms((oscms, 'multi-index'), omean_var, lorenz_opdf, ys[0], (mi, inds), scms0, M0, scale0)
    npt.assert_allclose(nell[0], rs[3], rtol=1e-6)
    npt.assert_allclose(means[0], rs[1], rtol=1e-6)
    npt.assert_allclose(scales[0], rs[2], rtol=1e-6)
    assert_moments(scmss[0], rs[0], mi, rtol=1e-6)
    # scaled and central filters agree (reference tests/test_filtering.py:168-242)
    _, cmeans, cnell = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), cms0, M0)
    npt.assert_allclose(means, cmeans, rtol=1e-6)
    npt.assert_allclose(nell, cnell, rtol=1e-6)


@pytest.mark.parametrize('N,T,order,kan', [(2, 8, 'euler', True), (2, 8, 2, True), (3, 8, 'euler', False),
                                           (3, 6, 2, False), (4, 2, 'euler', False)])
def test_lorenz_normal_closures(N, T, order, kan):
    """'index' Normal closures against the oracle filter, with the oracle's per-node Kan closure (N = 2) or with the host's
    vectorised d = 3 closure, which tests/test_host_nd3.py pins to Kan."""
    mi, inds = tables(3, N)
    cms0, rms0 = _init(mi)
    if order == 'euler':
        fns = moments.sde_cond_moments_euler_maruyama(_lorenz, _disp, DT, mi)
    else:
        fns = moments.sde_cond_moments_tme_normal(_lorenz, _disp, DT, order, mi)
    orms, ocms, omean = tme_sympy.sde_cond_moments_normal_nd(lorenz_drift, lorenz_disp, 3, DT, order, mi)
    if not kan:
        orms, ocms = fns[0], fns[1]
    ys = lorenz_ys(2, T, seed=30 + N)
    cmss, means, nell = filtering.moment_filter_nd_cms((fns[1], 'index'), fns[3], lorenz_pdf, ys, (mi, inds), cms0, M0)
    rc = omd.moment_filter_nd_cms((ocms, 'index'), omean, lorenz_opdf, ys[0], (mi, inds), cms0, M0)
    npt.assert_allclose(nell[0], rc[2], rtol=1e-6)
    npt.assert_allclose(means[0], rc[1], rtol=1e-6)
    assert_moments(cmss[0], rc[0], mi, rtol=1e-6)
    if N == 2:
        rmss, nell_r = filtering.moment_filter_nd_rms((fns[0], 'index'), lorenz_pdf, ys, (mi, inds), rms0)
        rr = omd.moment_filter_nd_rms((orms, 'index'), lorenz_opdf, ys[0], (mi, inds), rms0)
        npt.assert_allclose(nell_r[0], rr[1], rtol=1e-6)
        assert_moments(rmss[0], rr[0], mi, rtol=1e-6)


def _linear_model():
    A = np.array([[-1., 0.5, 0.], [-0.5, -1., 0.2], [0., -0.2, -0.5]])
    F = np.eye(3) + A * 0.05
    Q = np.array([[0.02, 0.005, 0.], [0.005, 0.03, 0.002], [0., 0.002, 0.01]])
    return F, Q


@pytest.mark.parametrize('mode', ['central', 'scaled'])
def test_linear_gaussian_three_factors(mode):
    """A 3-D linear-Gaussian model observed in every component (ny = 3), the reference's math.prod(norm.pdf(y, x, sd))."""
    N, T = 3, 12
    mi, inds = tables(3, N)
    F, Q = _linear_model()
    fns = moments.cond_moments_linear_gaussian(F, Q, mi)
    mean0 = np.array([0.5, -0.3, 0.2])
    cov0 = np.diag([0.2, 0.1, 0.15])
    cms0, _ = _init(mi, mean0, cov0)
    rng = np.random.default_rng(4)
    ys = rng.normal(size=(2, T, 3)) * 0.5

    def pdf(y, x):
        return math.prod(stats.norm_pdf(y, x, SD))

    def opdf(y, x):
        return float(np.prod(om.norm_pdf(y, x, SD)))

    if mode == 'central':
        cmss, means, nell = filtering.moment_filter_nd_cms((fns[1], 'index'), fns[3], pdf, ys, (mi, inds), cms0, mean0)
        rc = omd.moment_filter_nd_cms((fns[1], 'index'), fns[3], opdf, ys[0], (mi, inds), cms0, mean0)
        npt.assert_allclose(nell[0], rc[2], rtol=1e-6)
        npt.assert_allclose(means[0], rc[1], rtol=1e-6)
        assert_moments(cmss[0], rc[0], mi, rtol=1e-6)
    else:
        scale0 = np.sqrt(np.diag(cov0))
        scms0 = cms0 / np.prod(scale0 ** mi, axis=-1)
        scmss, means, scales, nell = filtering.moment_filter_nd_scms((fns[2], 'index'), fns[4], pdf, ys, (mi, inds),
                                                                     scms0, mean0, scale0)
        rs = omd.moment_filter_nd_scms((fns[2], 'index'), fns[4], opdf, ys[0], (mi, inds), scms0, mean0, scale0)
        npt.assert_allclose(nell[0], rs[3], rtol=1e-6)
        npt.assert_allclose(means[0], rs[1], rtol=1e-6)
        npt.assert_allclose(scales[0], rs[2], rtol=1e-6)
        assert_moments(scmss[0], rs[0], mi, rtol=1e-6)


@pytest.mark.parametrize('mode', ['raw', 'central'])
def test_ou_operator_poisson_factor(mode):
    """3-D OU with operator TME-2 tables and a Poisson-softplus factor on x_1."""
    N, T = 2, 15
    mi, inds = tables(3, N)
    A = np.array([[-1., 0.3, 0.], [0., -0.8, 0.4], [0.2, 0., -0.6]])

    def drift(x):
        return np.array([sum(A[i, j] * x[j] for j in range(3)) for i in range(3)], dtype=object)

    def drift_sympy(x):
        return [sum(A[i, j] * x[j] for j in range(3)) for i in range(3)]

    def disp(x):
        return np.diag([0.3, 0.3, 0.3]).astype(object)

    def disp_sympy(x):
        return [[0.3, 0, 0], [0, 0.3, 0], [0, 0, 0.3]]

    dt = 0.1
    mean0 = np.array([1., 1.5, 0.5])
    cov0 = np.diag([0.1, 0.1, 0.1])
    cms0, rms0 = _init(mi, mean0, cov0)
    fns = moments.sde_cond_moments_tme(drift, disp, dt, 2, d=3)
    ofns = tme_sympy.sde_cond_moments_tme_nd(drift_sympy, disp_sympy, 3, dt, 2, mi)
    ys = np.random.default_rng(9).poisson(1.5, size=(2, T)).astype(np.float64)

    def pdf(y, x):
        return stats.poisson_pmf(y, sym_softplus(x[1]))

    def opdf(y, x):
        return float(om.poisson_pmf(y, np.log1p(np.exp(x[1]))))

    if mode == 'raw':
        rmss, nell = filtering.moment_filter_nd_rms((fns[0], 'multi-index'), pdf, ys, (mi, inds), rms0)
        rr = omd.moment_filter_nd_rms((ofns[0], 'multi-index'), opdf, ys[0], (mi, inds), rms0)
        npt.assert_allclose(nell[0], rr[1], rtol=1e-6)
        assert_moments(rmss[0], rr[0], mi, rtol=1e-6)
    else:
        cmss, means, nell = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], pdf, ys, (mi, inds), cms0,
                                                           mean0)
        rc = omd.moment_filter_nd_cms((ofns[1], 'multi-index'), ofns[2], opdf, ys[0], (mi, inds), cms0, mean0)
        npt.assert_allclose(nell[0], rc[2], rtol=1e-6)
        npt.assert_allclose(means[0], rc[1], rtol=1e-6)
        assert_moments(cmss[0], rc[0], mi, rtol=1e-6)


def sym_softplus(x):
    return sym.log(1. + sym.exp(x))


def test_stable_filter_and_an_indefinite_start():
    """stable=True (the LDL^T completion, mfs/utils.py:495-538): on a well-posed start the completed factor is the Cholesky
    factor; from initial moments whose Gram matrix is indefinite the first rule takes the completion, as the oracle's does."""
    N, T = 3, 8
    mi, inds = tables(3, N)
    cms0, _ = _init(mi)
    fns = moments.sde_cond_moments_tme(_lorenz, _disp, DT, 2, d=3)
    ofns = tme_sympy.sde_cond_moments_tme_nd(lorenz_drift, lorenz_disp, 3, DT, 2, mi)
    ys = lorenz_ys(2, T, seed=41)
    cs, ms, ns = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), cms0, M0, stable=True)
    cp, mp, np_ = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), cms0, M0)
    npt.assert_allclose(ns, np_, rtol=1e-9)
    npt.assert_allclose(ms, mp, rtol=1e-9)
    r = omd.moment_filter_nd_cms((ofns[1], 'multi-index'), ofns[2], lorenz_opdf, ys[0], (mi, inds), cms0, M0, stable=True)
    npt.assert_allclose(ns[0], r[2], rtol=1e-6)
    assert_moments(cs[0], r[0], mi, rtol=1e-6)
    # E[x0^4] < E[x0^2]^2: no law has these moments, the LDL^T of the Gram matrix has a negative pivot
    bad = cms0.copy()
    bad[int(np.where((mi == [4, 0, 0]).all(axis=1))[0][0])] *= 0.2
    _, dpiv = o1.ldl(bad[inds[0]])
    assert dpiv.min() < 0.
    cb, mb, nb, fnb = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), bad, M0,
                                                     stable=True, return_first_nan=True)
    rb = omd.moment_filter_nd_cms((ofns[1], 'multi-index'), ofns[2], lorenz_opdf, ys[0], (mi, inds), bad, M0, stable=True)
    # the completed rule carries a node far out with a negligible weight; the following Gram matrices are singular to
    # rounding, and when a later pivot lands at -1e-17, +1e-17 or exactly 0 is rounding luck on either side (as at d = 1, 2).
    # The first step, which takes the completion, is compared: its K_k have norms ~ 1 / eps^2, and both eigensolvers are
    # accurate relative to that norm only, so the posterior means agree to ~1e-3 (measured 5.8e-4), not to 1e-6.
    assert np.all(np.isfinite(rb[0][0])) and np.all(np.isfinite(cb[0, 0]))
    npt.assert_allclose(mb[0, 0], rb[1][0], rtol=2e-3)
    # without the completion the same start poisons at once, as the reference's Cholesky does
    _, _, nell_c, fn_c = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), bad, M0,
                                                        return_first_nan=True)
    assert np.all(fn_c == 0) and np.all(np.isnan(nell_c))


def test_batch_position_poisoning_and_per_replicate_tables():
    N, T, B = 3, 12, 4
    mi, inds = tables(3, N)
    cms0, _ = _init(mi)
    fns = moments.sde_cond_moments_tme(_lorenz, _disp, DT, 2, d=3)
    ys = lorenz_ys(B, T, seed=7)
    mB, meansB, nellB, fnB = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), cms0, M0,
                                                            return_first_nan=True)
    assert np.all(fnB == -1)
    # a replicate's bits do not depend on where it sits in the batch
    for b in (0, 2):
        m1, means1, nell1 = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys[b], (mi, inds), cms0, M0)
        npt.assert_array_equal(m1, mB[b])
        npt.assert_array_equal(means1, meansB[b])
        assert nell1 == nellB[b]
    rev = ys[::-1].copy()
    mR, _, nellR = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, rev, (mi, inds), cms0, M0)
    npt.assert_array_equal(mR[::-1], mB)
    npt.assert_array_equal(nellR[::-1], nellB)
    # NaN poisoning is per replicate: the others keep their bits
    cms_b = np.tile(cms0, (B, 1))
    cms_b[1, int(np.where((mi == [2, 0, 0]).all(axis=1))[0][0])] = -1.
    m, means, nell, fn = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys, (mi, inds), cms_b,
                                                        np.tile(M0, (B, 1)), return_first_nan=True)
    assert fn[1] == 0 and np.isnan(nell[1]) and np.all(np.isnan(m[1])) and np.all(np.isnan(means[1]))
    for b in (0, 2, 3):
        assert fn[b] == -1 and nell[b] == nellB[b]
        npt.assert_array_equal(m[b], mB[b])
    # per-replicate tables (batch_closures): each replicate equals its own single-table run
    sigmas = [0.1, 0.15, 0.2, 0.25]
    per = [moments.sde_cond_moments_tme(_lorenz, (lambda s: (lambda x: np.diag([s, s, s]).astype(object)))(s), DT, 2, d=3)
           for s in sigmas]
    bfns = moments.batch_closures(per)
    mP, _, nellP = filtering.moment_filter_nd_cms((bfns[1], 'multi-index'), bfns[3], lorenz_pdf, ys, (mi, inds), cms0, M0)
    for b in (0, 3):
        m1, _, nell1 = filtering.moment_filter_nd_cms((per[b][1], 'multi-index'), per[b][3], lorenz_pdf, ys[b], (mi, inds), cms0, M0)
        npt.assert_allclose(mP[b], m1, rtol=1e-12, atol=1e-15)
        npt.assert_allclose(nellP[b], nell1, rtol=1e-12)
    assert abs(nellP[0] - nellP[3]) > 1e-6


def test_plan_is_bit_identical_to_the_host_entry_point():
    N, T, B = 2, 20, 3
    mi, inds = tables(3, N)
    cms0, _ = _init(mi)
    fns = moments.sde_cond_moments_tme(_lorenz, _disp, DT, 2, d=3)
    ys = np.ascontiguousarray(lorenz_ys(B, T, seed=11)[..., None])
    cmss, means, nell = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], lorenz_pdf, ys[..., 0], (mi, inds), cms0, M0)
    model, keep = filtering._model_struct3(fns[1].tables, filtering._trace_likelihood(lorenz_pdf, 3), B)
    # the second run is NLL only: NULL outputs are allowed
    geo, (full, nll_only) = run_plan_nd(model, N, T, B, mi, inds, m0=cms0, mean0=M0, ys=ys,
                                        outputs=(('moments', 'means', 'nell'), ('nell',)))
    assert geo.threads_per_filter == 256 and geo.grid == B and 0 < geo.lds_bytes <= 160 * 1024
    npt.assert_array_equal(full.moments, cmss)
    npt.assert_array_equal(full.means, means)
    npt.assert_array_equal(full.nell, nell)
    assert nll_only[:3] == (None, None, None) and nll_only.first_nan is None
    npt.assert_array_equal(nll_only.nell, nell)
    del keep
