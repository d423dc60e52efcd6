"""The characteristic functions of the grid filter's posteriors on the device (mfs_grid_filter_1d_cf) and of given densities
(mfs_cf_from_pdf_1d) against the exactly summed restatement of characteristic_from_pdf (tests/grid_cf_ref.py), against closed
forms, and against themselves (bits).

In the filter tests the restatement is applied to the pdfs the device returned from the same call, so that the cf is judged
apart from filter parity.  The bound per real and imaginary part is derived in tests/grid_cf_ref.py,
2 (n + 2 max|z x| + 8) 2^-53 sum_i w_i |p_i|; every test prints its worst error / bound ratio.
"""
import math

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats
from mfs_amd.classical_filters_smoothers.brute_force import brute_force_filter, GridFilterCFResult, GridFilterResult
from mfs_amd.one_dim.moments import characteristic_from_pdf
from tests import brute_force_ref as R
from tests import grid_cf_ref as G

pytestmark = pytest.mark.gpu

DT, T = 0.2, 3


def _gauss_pdf(y, x):
    return stats.norm_pdf(y, x, math.sqrt(R.OU_R))


def _case(n, B, uneven=False, T_=T):
    """The linear-Gaussian model of tests/brute_force_ref.py: B replicates with their own initial Normal."""
    rng = np.random.default_rng(1000 * n + B)
    xs = np.linspace(-3., 3., n)
    if uneven:
        xs = np.sort(xs + rng.uniform(-0.4, 0.4, n) * (xs[1] - xs[0]))
        assert np.all(np.diff(xs) > 0) and np.ptp(np.diff(xs)) > 0.01
    mu0, sd0 = 0.1 * np.arange(B) - 0.3, 0.5 + 0.02 * np.arange(B)
    init_ps = np.exp(-0.5 * ((xs[None, :] - mu0[:, None]) / sd0[:, None]) ** 2) / (math.sqrt(2 * math.pi) * sd0[:, None])
    ys = np.stack([R.ou_data(T_, rng, DT) for _ in range(B)])
    return xs, init_ps, ys


def _zs(m):
    """Uneven, not symmetric, both signs, magnitudes from 1e-3 to ~6 (|z x| up to ~18)."""
    k = np.arange(m)
    return np.where(k % 2 == 0, 1., -0.83) * (1e-3 + 6. * ((k * 0.6180339887498949) % 1.) ** 2) + 0.01 * k / m


def _filter(xs, init_ps, ys, zs=None, route='power', S=3, **kw):
    return brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, DT, S, 'chapman-tme-2',
                              return_summaries=True, route=route, zs=zs, **kw)


def _check_against_restatement(res, xs, zs, what):
    ratio = G.worst_ratio(res.cfs, G.cf_ref(res.pdfs, xs, zs), G.cf_bound(res.pdfs, xs, zs))
    print(f'{what}: worst |cf error| / bound {ratio:.3f}')
    assert ratio <= 1., f'{what}: cf error {ratio:.3f} x the bound'
    return ratio


# ---- 1. shape sweep: K padding of 16 and tile of 64 in n, the two halves of the table and the M padding in m, a second
# 64-column tile in B; one axis at a time (n = 65, m = 33, B = 3 is the point the three sweeps share)
SWEEP = [(n, 33, 3) for n in (2, 15, 16, 17, 63, 64, 65, 130)] + [(65, m, 3) for m in (1, 31, 32, 64, 65)] + \
        [(65, 33, B) for B in (1, 65)]


@pytest.mark.parametrize('route', ['power', 'stepwise'])
@pytest.mark.parametrize('n, m, B', SWEEP)
def test_shape_sweep_against_restatement(n, m, B, route):
    xs, init_ps, ys = _case(n, B)
    zs = _zs(m)
    res = _filter(xs, init_ps, ys, zs, route)
    assert isinstance(res, GridFilterCFResult)
    assert res.cfs.shape == (B, T, m) and res.cfs.dtype == np.complex128 and res.pdfs.shape == (B, T, n)
    _check_against_restatement(res, xs, zs, f'n={n} m={m} B={B} {route}')


@pytest.mark.parametrize('route', ['power', 'stepwise'])
def test_uneven_grid_and_no_replicate_axis(route):
    xs, init_ps, ys = _case(65, 3, uneven=True)
    zs = _zs(33)
    res = _filter(xs, init_ps, ys, zs, route)
    _check_against_restatement(res, xs, zs, f'uneven xs {route}')
    one = _filter(xs, init_ps[1], ys[1], zs, route)
    assert one.cfs.shape == (T, 33) and one.pdfs.shape == (T, 65) and one.nell.shape == ()
    lean = _filter(xs, init_ps, ys, zs, route, return_pdfs=False)      # the intended use: the pdfs never leave the device
    assert lean.pdfs is None
    npt.assert_array_equal(lean.cfs, res.cfs)
    only = brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, DT, 3, 'chapman-tme-2', route=route,
                              zs=zs)                                    # zs implies return_summaries
    assert isinstance(only, GridFilterCFResult)
    npt.assert_array_equal(only.cfs, res.cfs)


# ---- 2. the other outputs do not know about zs; bits are reproducible and do not depend on the batch
@pytest.mark.parametrize('route', ['power', 'stepwise'])
def test_unchanged_outputs_and_bits(route):
    xs, init_ps, ys = _case(65, 3)
    zs = _zs(33)
    plain = _filter(xs, init_ps, ys, None, route)
    assert isinstance(plain, GridFilterResult) and len(plain) == 5
    with_cf = _filter(xs, init_ps, ys, zs, route)
    again = _filter(xs, init_ps, ys, zs, route)
    for name in GridFilterResult._fields:
        npt.assert_array_equal(getattr(with_cf, name), getattr(plain, name), err_msg=f'{name} depends on zs')
    for a, b in zip(with_cf, again):
        npt.assert_array_equal(a, b, err_msg='two identical calls differ')
    for b in range(3):
        one = _filter(xs, init_ps[b:b + 1], ys[b:b + 1], zs, route)
        npt.assert_array_equal(one.pdfs[0], with_cf.pdfs[b], err_msg='pdfs depend on the batch')
        npt.assert_array_equal(one.cfs[0], with_cf.cfs[b], err_msg='cfs depend on the batch')


def test_output_blocks_of_several_steps():
    """T = 40 steps of 700 frequencies for 300 replicates are 134 MB of pairs: they leave in blocks of 19, 19 and 2 steps
    through two buffers.  The bits are those of the same replicates in a batch whose output is one block."""
    n, m, B, T_ = 16, 700, 300, 40
    xs, init_ps, ys = _case(n, B, T_=T_)
    zs = np.linspace(-2., 2., m)
    big = _filter(xs, init_ps, ys, zs, 'power')
    small = _filter(xs, init_ps[:3], ys[:3], zs, 'power')
    npt.assert_array_equal(big.cfs[:3], small.cfs)
    _check_against_restatement(GridFilterCFResult(big.pdfs[-2:], None, None, None, None, big.cfs[-2:]), xs, zs, 'blocks')


# ---- 3. structure
def test_structure_mass_symmetry_and_modulus():
    xs, init_ps, ys = _case(130, 3)
    half = np.abs(_zs(16)) + 0.05
    zs = np.concatenate([[0.], half, -half])
    res = _filter(xs, init_ps, ys, zs, 'power')
    w = R.trapz_weights(xs)
    mass = res.pdfs @ w
    bound = G.cf_bound(res.pdfs, xs, zs)
    print(f'max |cf(0) - mass| {np.abs(res.cfs[..., 0] - mass).max():.2e}, max |cf(0) - 1| {np.abs(res.cfs[..., 0] - 1).max():.2e}')
    npt.assert_allclose(res.cfs[..., 0].real, 1., rtol=0, atol=1e-13)
    npt.assert_array_equal(res.cfs[..., 0].imag, 0.)
    assert (np.abs(res.cfs[..., 0].real - mass) <= bound[..., 0]).all()
    plus, minus = res.cfs[..., 1:17], res.cfs[..., 17:]
    d = minus - np.conj(plus)
    ratio = max(np.abs(d.real / bound).max(), np.abs(d.imag / bound).max())
    print(f'cf(-z) against conj cf(z): worst difference / bound {ratio:.3f}')
    assert ratio <= 2.
    assert (np.abs(res.cfs) <= (mass * (1 + 1e-13))[..., None]).all()


# ---- 4. analytic pin of the standalone entry
def test_normal_density_pin_of_characteristic_from_pdf():
    mu, sigma, xs, ps, zs = G.normal_pin_case()
    dev = characteristic_from_pdf(zs, ps, xs)
    exact = np.exp(1j * zs * mu - 0.5 * zs ** 2 * sigma ** 2)
    ratio = G.worst_ratio(dev, G.cf_ref(ps, xs, zs), G.cf_bound(ps, xs, zs))
    print(f'N(mu, sigma^2) pin: max |err| {np.abs(dev - exact).max():.3e}; against the restatement {ratio:.3f} x the bound')
    npt.assert_allclose(dev, exact, rtol=0, atol=1e-12)
    assert ratio <= 1.


# ---- 5. Kalman pin through the filter
def test_kalman_pin_of_the_filter_cfs():
    """Model and grid of test_kalman_pin_on_the_device_power_route: xs = linspace(-5, 5, 1000), 20 sub-steps, chapman-tme-3,
    T = 100.  That grid is kept: on it the restatements alone stay within half the tolerance
    (tests/test_host_grid_cf.py::test_restatements_meet_the_kalman_pin_within_half_its_tolerance)."""
    xs, init_ps, ys, S = R.kalman_setting()
    res = brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, init_ps, xs, ys, R.OU_DT, S, 'chapman-tme-3',
                             return_pdfs=False, route='power', zs=G.KALMAN_ZS)
    true_m, true_v, _ = R.kalman(ys)
    exact = np.exp(1j * G.KALMAN_ZS[None, :] * true_m[:, None] - 0.5 * G.KALMAN_ZS[None, :] ** 2 * true_v[:, None])
    ratio = np.abs(res.cfs - exact) / G.kalman_cf_tolerance(G.KALMAN_ZS, true_m, true_v)
    print(f'Kalman cf pin: worst |err| / tolerance {ratio.max():.3f}, max |err| {np.abs(res.cfs - exact).max():.3e}')
    assert res.pdfs is None and res.cfs.shape == (100, G.KALMAN_ZS.shape[0])
    assert ratio.max() <= 1.


# ---- 6. NaN rule
@pytest.mark.parametrize('route', ['power', 'stepwise'])
def test_nan_poisons_the_cfs_of_one_replicate_only(route):
    n, B, S = 64, 4, 2
    xs, init_ps, ys = _case(n, B, T_=12)
    zs = _zs(33)
    clean = _filter(xs, init_ps, ys, zs, route, S=S)
    ys = ys.copy()
    ys[2, 5] = 1e4            # the likelihood underflows to zero on the whole grid
    res = _filter(xs, init_ps, ys, zs, route, S=S)
    assert list(res.first_nan) == [-1, -1, 5, -1] and list(clean.first_nan) == [-1] * 4
    assert np.isnan(res.cfs[2, 5:].real).all() and np.isnan(res.cfs[2, 5:].imag).all()
    assert np.isfinite(res.cfs[2, :5].real).all() and np.isfinite(res.cfs[2, :5].imag).all()
    npt.assert_array_equal(res.cfs[2, :5], clean.cfs[2, :5])
    npt.assert_array_equal(res.cfs[[0, 1, 3]], clean.cfs[[0, 1, 3]])
    _check_against_restatement(res, xs, zs, f'nan rule {route}')


# ---- 7. the standalone entry: shapes, a NaN row, chunks of rows
def test_characteristic_from_pdf_shapes_and_nan_row():
    rng = np.random.default_rng(7)
    n = 37
    xs = np.sort(rng.uniform(-2., 2., n))
    zs = _zs(5)
    worst = 0.
    for shape in ((n,), (5, n), (2, 3, n)):
        ps = rng.random(shape)
        for z in (zs, zs[3]):
            dev = characteristic_from_pdf(z, ps, xs)
            assert dev.shape == shape[:-1] + np.shape(z) and dev.dtype == np.complex128
            worst = max(worst, G.worst_ratio(dev.reshape(shape[:-1] + (-1,)), G.cf_ref(ps, xs, z), G.cf_bound(ps, xs, z)))
    ps = rng.random((5, n))
    clean = characteristic_from_pdf(zs, ps, xs)
    ps[3, 11] = np.nan
    dev = characteristic_from_pdf(zs, ps, xs)
    assert np.isnan(dev[3].real).all() and np.isnan(dev[3].imag).all()
    npt.assert_array_equal(dev[[0, 1, 2, 4]], clean[[0, 1, 2, 4]])
    worst = max(worst, G.worst_ratio(dev, G.cf_ref(ps, xs, zs), G.cf_bound(ps, xs, zs)))
    print(f'standalone shapes: worst |cf error| / bound {worst:.3f}')
    assert worst <= 1.


def test_characteristic_from_pdf_row_chunks(monkeypatch):
    """130 rows in one chunk (three 64-row tiles), and with MFS_HOST_CHUNKS = 3 in chunks of 64, 64 and 2 rows: the same bits,
    a NaN row in the middle chunk staying where it is."""
    rng = np.random.default_rng(8)
    n, count = 65, 130
    xs = np.linspace(-2., 2., n)
    zs = _zs(33)
    ps = rng.random((count, n))
    ps[70, 3] = np.nan
    monkeypatch.delenv('MFS_HOST_CHUNKS', raising=False)
    whole = characteristic_from_pdf(zs, ps, xs)
    monkeypatch.setenv('MFS_HOST_CHUNKS', '3')
    chunked = characteristic_from_pdf(zs, ps, xs)
    npt.assert_array_equal(chunked, whole)
    assert np.isnan(whole[70].real).all() and np.isfinite(np.delete(whole, 70, axis=0).real).all()
    ratio = G.worst_ratio(whole, G.cf_ref(ps, xs, zs), G.cf_bound(ps, xs, zs))
    print(f'row chunks: worst |cf error| / bound {ratio:.3f}')
    assert ratio <= 1.
    # the filter's posteriors through the standalone entry: the same table entries, the same order of summation
    fx, init_ps, ys = _case(65, 3)
    res = _filter(fx, init_ps, ys, zs, 'power')
    npt.assert_array_equal(characteristic_from_pdf(zs, res.pdfs, fx), res.cfs)


# ---- 8. C-level argument errors
def test_argument_errors_are_codes_with_messages():
    L = _lib.lib()
    n, T_, B, nz = 8, 3, 2, 4
    xs = np.linspace(-1., 1., n)
    m_, sd, lik, init, ys = 0.9 * xs, np.full(n, 0.3), np.array([1., 0., 0.1]), np.ones(n), np.zeros((B, T_))
    zs = np.linspace(-1., 1., nz)
    cfs = np.empty((B, T_, nz), dtype=np.complex128)
    nell, fn = np.empty(B), np.empty(B, dtype=np.int32)

    def filt(nz_, zs_, cfs_):
        rc = L.mfs_grid_filter_1d_cf(n, T_, B, 2, 1, _lib.ptr(xs), _lib.ptr(m_), _lib.ptr(sd), _lib.LIK['gaussian'], 3,
                                     _lib.ptr(lik), 0, _lib.ptr(init), 0, _lib.ptr(ys), nz_, _lib.ptr(zs_), None, None, None,
                                     _lib.ptr(cfs_), _lib.ptr(nell), _lib.ptr(fn), 0, None)
        return rc, L.mfs_last_error().decode()

    ps, out = np.ones((B, n)), np.empty((B, nz), dtype=np.complex128)

    def alone(nz_, zs_, out_, n_=n, count=B, xs_=xs, ps_=ps):
        rc = L.mfs_cf_from_pdf_1d(n_, count, nz_, _lib.ptr(xs_), _lib.ptr(zs_), _lib.ptr(ps_), _lib.ptr(out_), 0, None)
        return rc, L.mfs_last_error().decode()

    bad_z = [np.where(np.arange(nz) == 2, v, zs) for v in (np.nan, np.inf)]
    for fn_, name in ((filt, 'mfs_grid_filter_1d_cf'), (alone, 'mfs_cf_from_pdf_1d')):
        buf = cfs if fn_ is filt else out
        for args in [(-1, zs, buf), (nz, None, buf), (nz, zs, None)] + [(nz, z, buf) for z in bad_z]:
            rc, msg = fn_(*args)
            assert rc == -1 and name in msg, (name, args[0], rc, msg)
        rc, msg = fn_(8193, np.zeros(8193), buf)
        assert rc == -2 and '8192' in msg and name in msg
        rc, msg = fn_(0, None, None)
        assert rc == 0, msg
    for kw in (dict(n_=1), dict(count=-1), dict(xs_=xs[::-1].copy()), dict(xs_=None), dict(ps_=None)):
        rc, msg = alone(nz, zs, out, **kw)
        assert rc == -1 and 'mfs_cf_from_pdf_1d' in msg, (kw, rc, msg)
    rc, msg = alone(nz, zs, out, n_=8193)
    assert rc == -2 and '8192' in msg
    rc, msg = filt(nz, zs, cfs)        # and the library still works
    assert rc == 0 and np.isfinite(nell).all() and list(fn) == [-1, -1]
    assert np.isfinite(cfs.real).all() and np.abs(cfs).max() <= 1 + 1e-12
