"""The brute-force grid filter on the device (mfs_grid_filter_1d) against the NumPy restatement of the reference
(tests/brute_force_ref.py) and against the exact Kalman filter.

Tolerance, device against restatement: rtol = 1e-9 on every pdf entry above 1e-12 x its row's maximum, atol = 1e-12 x the row
maximum below that, rtol = 1e-9 on means, variances and NLL.  Every product here has non-negative operands, so its
componentwise error is <= n u; over S T <= 400 products at n <= 256 that is <= 1.2e-11, and the device's exp differing from
libm by a few ulp adds <= 2e-13: 1e-9 leaves two orders of margin.  "Both NaN" counts as agreement.
"""
import ctypes as C
import math

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats
from mfs_amd.classical_filters_smoothers.brute_force import brute_force_filter
from mfs_amd.one_dim import ss_models
from tests import brute_force_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def _gauss_pdf(y, x):
    return stats.norm_pdf(y, x, math.sqrt(R.OU_R))


def _assert_result_close(res, ref, what=''):
    pdfs, means, variances, nell, first_nan = ref
    worst = R.assert_pdfs_close(res.pdfs, pdfs)
    with np.errstate(invalid='ignore'):
        rel = [np.nanmax(np.abs(d / r - 1)) if np.isfinite(r).any() else 0.
               for d, r in ((res.means, means), (res.variances, variances), (res.nell, nell))]
    print(f'{what}: worst relative error pdf {worst:.2e}, mean {rel[0]:.2e}, variance {rel[1]:.2e}, nell {rel[2]:.2e}')
    npt.assert_allclose(res.means, means, rtol=RTOL, atol=0, equal_nan=True)
    npt.assert_allclose(res.variances, variances, rtol=RTOL, atol=0, equal_nan=True)
    npt.assert_allclose(res.nell, nell, rtol=RTOL, atol=0, equal_nan=True)
    npt.assert_array_equal(res.first_nan, first_nan)


# ---- shape sweep: tile edges (n = 37, 130 straddle the 64-tile, 64 is exact), the padded replicate tile, both exponentiation paths
SWEEP_DT, SWEEP_T = 0.2, 12


def _sweep_case(n, B):
    rng = np.random.default_rng(1000 * n + B)
    xs = np.linspace(-3., 3., n)
    mu0, sd0 = 0.1 * np.arange(B) - 0.3, 0.5 + 0.02 * np.arange(B)
    init_ps = np.exp(-0.5 * ((xs[None, :] - mu0[:, None]) / sd0[:, None]) ** 2) / (math.sqrt(2 * math.pi) * sd0[:, None])
    ys = np.stack([R.ou_data(SWEEP_T, rng, SWEEP_DT) for _ in range(B)])
    return xs, init_ps, ys


@pytest.mark.parametrize('S', [1, 2, 5, 8])
@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('n', [37, 64, 130])
def test_shape_sweep_both_routes_against_restatement(n, B, S):
    xs, init_ps, ys = _sweep_case(n, B)
    ref = R.brute_force_ref(R.ou_drift, R.ou_dispersion, lambda b: _gauss_pdf, init_ps, xs, ys, SWEEP_DT, S, 'chapman-tme-2')
    res = {}
    for route in ('power', 'stepwise'):
        res[route] = brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, SWEEP_DT, S, 'chapman-tme-2',
                                        return_summaries=True, route=route)
        assert res[route].pdfs.shape == (B, SWEEP_T, n) and res[route].means.shape == (B, SWEEP_T)
        _assert_result_close(res[route], ref, f'n={n} B={B} S={S} {route}')
    a, b = res['power'], res['stepwise']
    _assert_result_close(a, (b.pdfs, b.means, b.variances, b.nell, b.first_nan), f'n={n} B={B} S={S} power vs stepwise')


# ---- models
def test_benes_bernoulli_tme3():
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
    n, S, T, B = 200, 4, 20, 3
    xs = np.linspace(-4., 4., n)
    ys = np.random.default_rng(3).random((B, T)) < 0.5          # boolean measurements
    init_ps = ic.pdf(xs)
    ref = R.brute_force_ref(drift, dispersion, lambda b: pmf, init_ps, xs, ys, dt, S, 'chapman-tme-3')
    for route in ('power', 'stepwise'):
        res = brute_force_filter(drift, dispersion, pmf, init_ps, xs, ys, dt, S, 'chapman-tme-3', return_summaries=True,
                                 route=route)
        _assert_result_close(res, ref, f'benes-bernoulli {route}')
    # the reference's call shape: one replicate, positional arguments, pdfs only
    one = brute_force_filter(drift, dispersion, pmf, init_ps, xs, ys[0], dt, S, 'chapman-tme-3')
    assert one.shape == (T, n)
    R.assert_pdfs_close(one, ref[0][0])


def test_well_poisson_per_replicate_likelihood_parameter_euler():
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.well_poisson(3.)
    n, S, T, B = 200, 4, 20, 3
    xs = np.linspace(-4., 4., n)
    theta2 = np.array([0.5, 1.5, 2.5])
    ys = np.random.default_rng(4).poisson(1., size=(B, T))
    init_ps = ic.pdf(xs)
    ref = R.brute_force_ref(lambda x: drift(x, 3.), dispersion, lambda b: (lambda y, x: pmf(y, x, theta2[b])), init_ps, xs,
                            ys, dt, S, 'chapman-euler')
    res = brute_force_filter(lambda x: drift(x, 3.), dispersion, lambda y, x: pmf(y, x, theta2), init_ps, xs, ys, dt, S,
                             'chapman-euler', return_summaries=True)
    _assert_result_close(res, ref, 'well-poisson')
    assert np.abs(res.nell[0] - res.nell[2]) > 1e-3       # the parameter reached its replicate


def test_uneven_grid():
    rng = np.random.default_rng(5)
    n, S, B = 130, 3, 3
    base = np.linspace(-3., 3., n)
    xs = np.sort(base + rng.uniform(-0.4, 0.4, n) * (base[1] - base[0]))
    assert np.all(np.diff(xs) > 0) and np.ptp(np.diff(xs)) > 0.01
    _, init_ps, ys = _sweep_case(n, B)
    ref = R.brute_force_ref(R.ou_drift, R.ou_dispersion, lambda b: _gauss_pdf, init_ps, xs, ys, SWEEP_DT, S, 'chapman-tme-2')
    for route in ('power', 'stepwise'):
        res = brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, SWEEP_DT, S, 'chapman-tme-2',
                                 return_summaries=True, route=route)
        _assert_result_close(res, ref, f'uneven grid {route}')


# ---- analytic pin on the device: independent of the restatement
def test_kalman_pin_on_the_device_power_route():
    xs, init_ps, ys, S = R.kalman_setting()
    res = brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, R.OU_DT, S, 'chapman-tme-3',
                             return_summaries=True, route='power')
    true_m, true_v, true_nell = R.kalman(ys)
    est_m = R.trapz(res.pdfs * xs[None, :], xs, axis=1)
    est_2nd = R.trapz(res.pdfs * xs[None, :] ** 2, xs, axis=1)
    print(f'max |mean err| {np.abs(est_m - true_m).max():.3e}, max rel 2nd-moment err '
          f'{np.abs(est_2nd / (true_v + true_m ** 2) - 1).max():.3e}, |nell err| {abs(res.nell - true_nell):.3e}')
    npt.assert_allclose(est_m, true_m, atol=1e-11, rtol=1e-10)
    npt.assert_allclose(est_2nd, true_v + true_m ** 2, atol=1e-11, rtol=1e-10)
    assert abs(res.nell - true_nell) <= 1e-10
    assert res.first_nan == -1 and res.means.shape == (100,)


# ---- outputs
def test_outputs_are_consistent_and_reproducible():
    n, B, S = 130, 3, 5
    xs, init_ps, ys = _sweep_case(n, B)
    args = (R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, SWEEP_DT, S, 'chapman-tme-2')
    full = brute_force_filter(*args, return_summaries=True)
    again = brute_force_filter(*args, return_summaries=True)
    for a, b in zip(full, again):
        assert np.array_equal(a, b), 'two identical calls differ'
    lean = brute_force_filter(*args, return_pdfs=False, return_summaries=True)
    assert lean.pdfs is None
    for a, b in zip(full[1:], lean[1:]):
        assert np.array_equal(a, b), 'summaries depend on return_pdfs'
    w = R.trapz_weights(xs)
    mass = full.pdfs @ w
    means = (full.pdfs * xs) @ w
    variances = np.einsum('btn,n->bt', (xs[None, None, :] - full.means[..., None]) ** 2 * full.pdfs, w)
    print(f'max |mass - 1| {np.abs(mass - 1).max():.2e}, mean rel {np.abs(full.means / means - 1).max():.2e}, '
          f'variance rel {np.abs(full.variances / variances - 1).max():.2e}, min |mean| {np.abs(means).min():.2e}')
    npt.assert_allclose(mass, 1., rtol=0, atol=1e-13)
    npt.assert_allclose(full.means, means, rtol=1e-13, atol=0)
    npt.assert_allclose(full.variances, variances, rtol=1e-13, atol=0)
    only_pdfs = brute_force_filter(*args)
    assert np.array_equal(only_pdfs, full.pdfs)


# ---- NaN isolation
def test_nan_poisons_one_replicate_only():
    n, B, S = 64, 4, 2
    xs, init_ps, ys = _sweep_case(n, B)
    ys[2, 5] = 1e4            # the likelihood underflows to zero on the whole grid
    ref = R.brute_force_ref(R.ou_drift, R.ou_dispersion, lambda b: _gauss_pdf, init_ps, xs, ys, SWEEP_DT, S, 'chapman-tme-2')
    assert list(ref[4]) == [-1, -1, 5, -1]
    for route in ('power', 'stepwise'):
        res = brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, SWEEP_DT, S, 'chapman-tme-2',
                                 return_summaries=True, route=route)
        assert list(res.first_nan) == [-1, -1, 5, -1]
        assert np.isnan(res.pdfs[2, 5:]).all() and np.isfinite(res.pdfs[2, :5]).all()
        assert np.isnan(res.means[2, 5:]).all() and np.isnan(res.variances[2, 5:]).all() and np.isnan(res.nell[2])
        assert np.isfinite(res.pdfs[[0, 1, 3]]).all() and np.isfinite(res.nell[[0, 1, 3]]).all()
        _assert_result_close(res, ref, f'nan isolation {route}')


# ---- the GEMM on its own: exact integer data, asymmetric operands (a transposed store or a wrong tile cannot pass)
def test_gemm_exact_on_integer_data():
    rng = np.random.default_rng(6)
    M, N, K = 192, 128, 80
    A = rng.integers(-9, 10, (M, K)).astype(np.float64)
    Bm = rng.integers(-9, 10, (K, N)).astype(np.float64)
    dA, dB, dC = _lib.DeviceBuffer.from_array(A), _lib.DeviceBuffer.from_array(Bm), _lib.DeviceBuffer(M * N * 8)
    L = _lib.lib()
    _lib.check(L.mfs_grid_gemm_dev(M, N, K, dA.ptr, dB.ptr, dC.ptr, None))
    _lib.check(L.mfs_device_synchronize())
    assert np.array_equal(dC.to_array((M, N)), A @ Bm)
    assert L.mfs_grid_gemm_dev(M, N, 70, dA.ptr, dB.ptr, dC.ptr, None) == -1
    assert L.mfs_grid_gemm_dev(M, N, K, dA.ptr, dB.ptr, dA.ptr, None) == -1
    for buf in (dA, dB, dC):
        buf.free()


# ---- error codes
def test_argument_errors_are_codes_with_messages():
    L = _lib.lib()
    n, T, B = 8, 3, 2
    xs = np.linspace(-1., 1., n)
    good = dict(n=n, T=T, B=B, S=2, power=1, xs=xs, m=0.9 * xs, sd=np.full(n, 0.3), kind=_lib.LIK['gaussian'], n_lik=3,
                lik=np.array([1., 0., 0.1]), init=np.ones(n), ys=np.zeros((B, T)))

    def call(**kw):
        a = dict(good, **kw)
        nell, fn = np.empty(max(a['B'], 1)), np.empty(max(a['B'], 1), dtype=np.int32)
        rc = L.mfs_grid_filter_1d(a['n'], a['T'], a['B'], a['S'], a['power'], _lib.ptr(a['xs']), _lib.ptr(a['m']),
                                  _lib.ptr(a['sd']), a['kind'], a['n_lik'], _lib.ptr(a['lik']), 0, _lib.ptr(a['init']), 0,
                                  _lib.ptr(a['ys']), None, None, None, _lib.ptr(nell), _lib.ptr(fn), 0, None)
        return rc, L.mfs_last_error().decode(), nell, fn

    bad_sd = [np.where(np.arange(n) == 3, v, 0.3) for v in (0., -0.3, np.nan, np.inf)]
    einval = [dict(n=1), dict(T=0), dict(B=0), dict(xs=xs[::-1].copy()), dict(xs=np.where(np.arange(n) == 4, xs[3], xs)),
              dict(kind=_lib.LIK['bearing_gaussian']), dict(kind=-1)] + [dict(sd=s) for s in bad_sd]
    for kw in einval:
        rc, msg, _, _ = call(**kw)
        assert rc == -1 and 'mfs_grid_filter_1d' in msg, (kw, rc, msg)
    rc, msg, _, _ = call(n=8193)
    assert rc == -2 and '8192' in msg
    rc, msg, nell, fn = call()      # and the library still works
    assert rc == 0 and np.isfinite(nell).all() and list(fn) == [-1, -1]
