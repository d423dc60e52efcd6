"""`cf1d_fast_kernel` over its whole envelope: all 31 instantiations N = 2..32 against exact arithmetic,
and the geometry of the launch bit for bit.

Accuracy.  tests/golden/cf_exact.npz (tests/golden/make_cf_exact.py, pinned by tests/test_host_characteristic_ref.py) holds
phi(z) = sum_n w_n exp(i z x_n) of the exact-arithmetic N-point rule on fp64 moments of Gaussian mixtures in three presentations
(scaled / central / raw), a mean = 1000 case per order, and N-atom discrete laws.  Per case the device is held to

    max_z |device - exact|  <=  K max(e_ref, floor),      floor = (N + max|z x_n|) 2^-53,

with e_ref = max_z |fp64 NumPy oracle - exact| computed at test time on the same inputs.  Nothing else is typed in: K is the
smallest power of two that is at least four times the worst ratio device_err / max(e_ref, floor) observed on an MI355X on the
committed fixture (the factor 4 leaves room for another draw of the same family).  The device's rule is not LAPACK's
algorithm (square-root-free Cholesky, Laguerre on the characteristic polynomial), so the ratio cannot be derived; on the narrow
grid, where the oracle sits at one floor, a ratio above 64 would be a defect of the kernel and not a number to adopt.

Measured ratios device_err / max(e_ref, floor), worst case per order (MI355X, the committed fixture; printed by
test_measured_ratios_table with -s):
    narrow    N=2: 0.53  3: 0.38  4: 0.36  5: 0.50  6: 0.28  7: 0.45  8: 0.45  9: 0.33  10: 0.28  11: 0.27  12: 0.27  13: 0.32
              14: 0.30  15: 0.31  16: 0.25  17: 0.31  18: 0.14  19: 0.23  20: 0.47  21: 0.20  22: 0.20  23: 0.28  24: 0.45
              25: 0.22  26: 0.17  27: 0.24  28: 0.25  29: 0.27  30: 0.19  31: 0.37  32: 0.26
    wide      N=2: 0.69  3: 0.38  4: 0.50  5: 1.63  6: 1.42  7: 4.26  8: 2.89  9: 15.47  10: 6.35  11: 3.71  12: 13.87
    discrete  N=2: 0.43  3: 0.41  4: 0.64  5: 0.33  6: 0.41  7: 1.06  8: 1.16  9: 0.20  10: 0.52  11: 0.64  12: 0.78
Worst 15.47 (wide grid, N = 9); 4 x 15.47 = 61.9, so K = 64.  On the narrow grid the device is never above 0.53: it sits at the
floor like the oracle, at every order and also at mean = 1000.

Geometry (bit for bit): a row does not depend on the batch it sits in (counts 1, F - 1, F, F + 1, 3 F + 2 around the F = 64 / G
filters of a block), on nz (1, G - 1, G, G + 1, 2 G + 3, 257: the z loop strides by G), on NULL against all-zero `mean` /
all-one `scale` in the C entry, or on a poisoned neighbour in its wave."""
import ctypes as C
import functools

import mpmath as mp
import numpy as np
import pytest

from mfs_amd import _lib
from mfs_amd.one_dim import moments, quadtures
from oracle import exact_mp
from tests import cf_exact_ref as R

pytestmark = pytest.mark.gpu

K = 64.
MFS_EINVAL, MFS_EUNSUPPORTED = -1, -2      # include/mfs_hip.h
EDGE_ORDERS = (2, 7, 8, 15, 16, 31, 32)    # both sides of every change of the lane-group width
_ratios = {}


def group_lanes(N):
    """Lanes per moment vector (csrc/registry.hpp, default_group): the N + 1 rows of the extended Hankel matrix must fit."""
    return 8 if N <= 7 else 16 if N <= 15 else 32 if N <= 31 else 64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def c_entry(N, ms, mean, scale, zs, out=None, count=None, nz=None):
    """mfs_characteristic_1d itself: (return code, out); None is passed as NULL."""
    count = ms.shape[0] if count is None else count
    nz = zs.shape[0] if nz is None else nz
    if out is None:
        out = np.full((max(count, 0), max(nz, 0)), np.nan + 0j, dtype=np.complex128)
    rc = _lib.lib().mfs_characteristic_1d(N, count, _lib.ptr(ms), _lib.ptr(mean), _lib.ptr(scale), nz, _lib.ptr(zs),
                                          out.ctypes.data_as(C.c_void_p), 0, None)
    return rc, out


@functools.lru_cache(maxsize=None)
def device_values(N):
    """{case id: device cf on the case's grid}: one call per presentation and grid, the vectors' grids side by side."""
    out = {}
    for grid in R.GRIDS:
        for kind in R.KINDS + ('discrete',):
            cs = R.cases(N, grid, kind)
            if not cs:
                continue
            z = np.concatenate([c.z for c in cs])
            ms = np.stack([c.ms for c in cs])
            args = [np.array([c.mean for c in cs])] if cs[0].mean is not None else []
            args += [np.array([c.scale for c in cs])] if cs[0].scale is not None else []
            cf = moments.characteristic_fn(z, ms, *args)
            assert cf.shape == (len(cs), z.shape[0]) and cf.dtype == np.complex128
            for b, c in enumerate(cs):
                out[c.id] = cf[b, 33 * b:33 * (b + 1)].copy()
    return out


def split_error(c, dev):
    """For a failure message: the device's own rule, evaluated in 50-digit arithmetic, against the device's cf -- what the
    evaluation (sincos, the z sum) contributes, apart from the rule."""
    w, x = quadtures.moment_quadrature(c.ms, 0. if c.mean is None else c.mean, 1. if c.scale is None else c.scale)
    mp.mp.dps = 50
    own = np.array([complex(mp.fsum(mp.mpf(float(wi)) * mp.expj(mp.mpf(float(z)) * mp.mpf(float(xi))) for wi, xi in zip(w, x)))
                    for z in c.z])
    return float(np.abs(dev - own).max())


def check_case(c, dev):
    err = float(np.abs(dev - c.exact).max())
    denom = max(R.e_ref(c), c.floor)
    ratio = err / denom
    key = (c.N, c.grid)
    _ratios[key] = max(_ratios.get(key, 0.), ratio)
    if not ratio <= K:       # (also catches NaN)
        pytest.fail(f'{c.id}: |device - exact| = {err:.3e} = {ratio:.1f} x max(e_ref {R.e_ref(c):.2e}, floor {c.floor:.2e}), K = {K:g}; '
                    f'of that |device cf - sum w exp(i z x) on the device\'s own rule| = {split_error(c, dev):.3e} (evaluation), '
                    f'the rest is the rule')
    if c.closed is not None:
        gap = float(np.abs(c.exact - c.closed).max())
        assert np.abs(dev - c.closed).max() <= K * denom + gap, c.id
    return ratio


@pytest.mark.parametrize('N', R.ORDERS)
def test_every_order_against_exact_arithmetic(N):
    dev = device_values(N)
    cs = R.cases(N)
    assert len(cs) == (34 if N <= 12 else 16) and set(dev) == {c.id for c in cs}
    worst = {}
    for c in cs:
        worst[c.grid] = max(worst.get(c.grid, 0.), check_case(c, dev[c.id]))
    print(f'N = {N}: worst device_err / max(e_ref, floor): ' + ', '.join(f'{g} {r:.2f}' for g, r in worst.items()))


def test_measured_ratios_table():
    """The table of the module docstring and of DESIGN.md section 4 (after the test above; prints with -s)."""
    for grid in R.GRIDS:
        print(grid, ' '.join(f'{N}: {r:.2f}' for (N, g), r in sorted(_ratios.items()) if g == grid))
    if _ratios:
        print(f'worst {max(_ratios.values()):.2f}, narrow {max(r for (_, g), r in _ratios.items() if g == "narrow"):.2f}, K = {K:g}')
    assert all(r <= K for r in _ratios.values())


@pytest.mark.parametrize('N', R.ORDERS)
def test_zero_frequency_and_large_phase(N):
    dev = device_values(N)
    for c in R.cases(N):
        at0 = dev[c.id][16]
        assert c.z[16] == 0.0
        assert at0.imag == 0.0, c.id
        assert abs(at0.real - 1.) <= 4 * N * R.U53, f'{c.id}: phi(0) - 1 = {at0.real - 1.:.3e}'
    large = R.cases(N, 'narrow', 'large')
    assert len(large) == 1 and large[0].mean == 1000. and large[0].zx > 3900.     # floor ~ 4.5e-13: the rounding of z * x
    check_case(large[0], dev[large[0].id])


# ---------------------------------------------------------------------------------------------------------------------
# geometry, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
Z33 = np.linspace(-2., 2., 33)


@functools.lru_cache(maxsize=None)
def single_rows(N):
    ms, mean, scale = R.vectors(N)
    rows = np.stack([moments.characteristic_fn(Z33, ms[v], mean[v], scale[v]) for v in range(5)])
    assert rows.shape == (5, 33) and np.all(np.isfinite(rows))
    return rows


@pytest.mark.parametrize('N', EDGE_ORDERS)
def test_rows_do_not_depend_on_the_batch(N):
    F = 64 // group_lanes(N)
    ms, mean, scale = R.vectors(N)
    alone = single_rows(N)
    counts = sorted({n for n in (1, F - 1, F, F + 1, 3 * F + 2) if n > 0})
    assert counts[-1] == 3 * F + 2
    for count in counts:
        idx = np.arange(count) % 5
        cf = moments.characteristic_fn(Z33, ms[idx], mean[idx], scale[idx])
        assert cf.shape == (count, 33)
        assert np.array_equal(bits(cf), bits(alone[idx])), f'count = {count}'
        again = moments.characteristic_fn(Z33, ms[idx], mean[idx], scale[idx])
        assert np.array_equal(bits(cf), bits(again)), f'count = {count}: two calls differ'


@pytest.mark.parametrize('N', EDGE_ORDERS)
def test_values_do_not_depend_on_the_number_of_frequencies(N):
    G = group_lanes(N)
    ms, mean, scale = R.vectors(N)
    z = np.linspace(-2., 2., 257)
    assert np.array_equal(z[::8], Z33)
    full = moments.characteristic_fn(z, ms, mean, scale)
    assert full.shape == (5, 257) and np.all(np.isfinite(full))
    np.testing.assert_array_equal(bits(full[:, ::8]), bits(single_rows(N)))      # the same z values at other positions
    for nz in sorted({1, G - 1, G, G + 1, 2 * G + 3}):
        cf = moments.characteristic_fn(z[:nz], ms, mean, scale)
        assert cf.shape == (5, nz)
        assert np.array_equal(bits(cf), bits(full[:, :nz])), f'nz = {nz}'
    one = moments.characteristic_fn(float(z[3]), ms, mean, scale)                # scalar z: shape ms.shape[:-1]
    assert one.shape == (5,) and np.array_equal(bits(one), bits(full[:, 3]))
    single = moments.characteristic_fn(float(z[3]), ms[1], mean[1], scale[1])
    assert np.ndim(single) == 0 and np.array_equal(bits(np.array([single])), bits(full[1:2, 3]))
    idx = np.arange(6) % 5                                                       # a leading shape of (2, 3) round-trips
    lead = moments.characteristic_fn(z[:G + 1], ms[idx].reshape(2, 3, 2 * N), mean[idx].reshape(2, 3), scale[idx].reshape(2, 3))
    assert lead.shape == (2, 3, G + 1)
    assert np.array_equal(bits(lead.reshape(6, G + 1)), bits(full[idx, :G + 1]))
    assert moments.characteristic_fn(float(z[3]), ms[idx].reshape(2, 3, 2 * N), mean[idx].reshape(2, 3)).shape == (2, 3)


@pytest.mark.parametrize('N', [7, 16, 32])
def test_null_mean_and_scale_in_the_c_entry(N):
    raw = np.stack([c.ms for c in R.cases(N, 'narrow', 'raw')])
    cen = R.cases(N, 'narrow', 'central')
    cms, cmean = np.stack([c.ms for c in cen]), np.array([c.mean for c in cen])
    zeros, ones = np.zeros(5), np.ones(5)
    rc, base = c_entry(N, raw, zeros, ones, Z33)
    assert rc == _lib.MFS_OK and np.all(np.isfinite(base))
    for mean, scale in ((None, None), (None, ones), (zeros, None)):
        rc, out = c_entry(N, raw, mean, scale, Z33)
        assert rc == _lib.MFS_OK
        assert np.array_equal(bits(out), bits(base)), (mean is None, scale is None)
    rc, with_ones = c_entry(N, cms, cmean, ones, Z33)
    rc2, with_null = c_entry(N, cms, cmean, None, Z33)
    assert rc == rc2 == _lib.MFS_OK and np.all(np.isfinite(with_ones))
    assert np.array_equal(bits(with_null), bits(with_ones))
    assert not np.array_equal(bits(with_ones), bits(c_entry(N, cms, None, None, Z33)[1]))     # the mean is read when given


def ldl_pivots(ms, dps=100):
    """Pivots of the square-root-free Cholesky of the Hankel matrix of `ms` in `dps`-digit arithmetic."""
    mp.mp.dps = dps
    n = len(ms) // 2
    m = [mp.mpf(float(v)) for v in ms]
    L = [[mp.mpf(0)] * n for _ in range(n)]
    d = []
    for j in range(n):
        d.append(m[2 * j] - mp.fsum(L[j][k] ** 2 * d[k] for k in range(j)))
        for i in range(j + 1, n):
            L[i][j] = (m[i + j] - mp.fsum(L[i][k] * L[j][k] * d[k] for k in range(j))) / d[j]
    return d


@pytest.mark.parametrize('N', [3, 8, 16, 32])
def test_poison_stays_in_its_row(N):
    F = 64 // group_lanes(N)
    count = 2 * F + 1
    ia, ib = F // 2, F + (F + 1) // 2               # inside the first and the second wave (F = 1: rows 0 and 2)
    assert 0 <= ia < ib < count
    # raw presentation: at N = 3 halving m_4 turns the last pivot negative for the raw moments of laws 2 and 3 only (standardised,
    # the pivot stays near 2 > m_4 / 2 ~ 1.5), so law 2 sits in row ib at every order
    raw = sorted(R.cases(N, 'narrow', 'raw'), key=lambda c: c.vec)
    idx = np.arange(count) % 5
    idx[ib] = 2
    ms = np.stack([raw[v].ms for v in idx])
    mean, scale = np.zeros(count), np.ones(count)
    rc, clean = c_entry(N, ms, mean, scale, Z33)
    assert rc == _lib.MFS_OK and np.all(np.isfinite(clean))
    bad = ms.copy()
    bad[ia, 2] = -bad[ia, 2]                        # m_2 negated: the second pivot m_2 - m_1^2 is negative
    bad[ib, 2 * N - 2] *= 0.5                       # m_{2N-2} halved: enters the last pivot only
    piv_clean, piv = ldl_pivots(ms[ib]), ldl_pivots(bad[ib])
    assert all(p > 0 for p in piv_clean) and all(p > 0 for p in piv[:-1]) and piv[-1] < 0
    assert piv[:-1] == piv_clean[:-1]
    assert exact_mp.moment_quadrature([mp.mpf(float(v)) for v in bad[ib]]) is None
    assert exact_mp.moment_quadrature([mp.mpf(float(v)) for v in bad[ia]]) is None
    rc, out = c_entry(N, bad, mean, scale, Z33)
    assert rc == _lib.MFS_OK
    for i in (ia, ib):
        assert not np.any(np.isfinite(out[i].real)) and not np.any(np.isfinite(out[i].imag)), f'row {i}'
    keep = np.setdiff1d(np.arange(count), [ia, ib])
    assert np.array_equal(bits(out[keep]), bits(clean[keep]))


def test_error_codes_and_empty_calls():
    N = 7
    ms, mean, scale = R.vectors(N)
    L = _lib.lib()
    for n_bad in (1, 33, 0, -3):
        wrong = np.ones((5, max(2 * n_bad, 2)))
        rc, _ = c_entry(n_bad, wrong, None, None, Z33)
        assert rc == MFS_EUNSUPPORTED and L.mfs_last_error(), n_bad
    assert c_entry(N, ms, mean, scale, Z33, count=-1)[0] == MFS_EINVAL
    assert c_entry(N, ms, mean, scale, Z33, nz=-1)[0] == MFS_EINVAL
    sentinel = np.full((5, 33), 7.25 - 3.5j)
    out = sentinel.copy()
    assert c_entry(N, None, mean, scale, Z33, out=out, count=5)[0] == MFS_EINVAL
    assert c_entry(N, ms, mean, scale, None, out=out, nz=33)[0] == MFS_EINVAL
    assert L.mfs_characteristic_1d(N, 5, _lib.ptr(ms), _lib.ptr(mean), _lib.ptr(scale), 33, _lib.ptr(Z33), None, 0, None) == MFS_EINVAL
    assert c_entry(N, ms, mean, scale, Z33, out=out, count=0)[0] == _lib.MFS_OK
    assert c_entry(N, ms, mean, scale, Z33, out=out, nz=0)[0] == _lib.MFS_OK
    assert c_entry(N, None, None, None, None, out=out, count=0, nz=0)[0] == _lib.MFS_OK
    assert np.array_equal(bits(out), bits(sentinel))            # nothing above wrote to the output
    rc, out = c_entry(N, ms, mean, scale, Z33, out=out)         # and the same buffers do work
    assert rc == _lib.MFS_OK and np.array_equal(bits(out), bits(single_rows(N)))
    assert moments.characteristic_fn(Z33, np.empty((0, 2 * N))).shape == (0, 33)
    assert moments.characteristic_fn(np.empty(0), ms, mean, scale).shape == (5, 0)
    for m2 in (7, 2, 66, 1):                                    # an odd moment count, N = 1, N = 33
        with pytest.raises(ValueError):
            moments.characteristic_fn(Z33, np.ones((5, m2)))
