"""tests/nd_support.py without a library or a GPU: what assert_moments, first_bad, initial and same_bits accept and refuse."""
import math

import numpy as np
import numpy.testing as npt
import pytest

from tests.nd_support import assert_moments, first_bad, initial, same_bits, second, tables

RTOL = 1e-6
MEAN = {2: np.array([0.4, -0.7]), 3: np.array([0.4, -0.7, 1.1])}
SD = {2: np.array([0.5, 0.25]), 3: np.array([0.5, 0.25, 0.32])}


def _index(mi, n):
    return int(np.where((mi == np.asarray(n)).all(axis=1))[0][0])


def _table(d):
    """(mi, a (T, z) table of central moments): three steps of a product law whose standard deviations grow by 10 % a step --
    every odd moment is exactly 0 and the natural magnitude of moment n at step t is prod_k sd_k(t)^{n_k} -- and a fourth
    step that is NaN throughout, as a poisoned replicate's is."""
    mi, _ = tables(d, 2)
    rows = [initial(mi, MEAN[d], np.diag((SD[d] * 1.1 ** t) ** 2))['cms'] for t in range(3)]
    return mi, np.stack(rows + [np.full(mi.shape[0], np.nan)])


def _natural(d, t, n):
    return float(np.prod((SD[d] * 1.1 ** t) ** np.asarray(n)))


def _refused(got, ref, mi):
    with pytest.raises(AssertionError):
        assert_moments(got, ref, mi, RTOL)


@pytest.mark.parametrize('d', [2, 3])
def test_equal_tables_with_nans_in_equal_places_pass(d):
    mi, ref = _table(d)
    assert np.isnan(ref).any() and np.isfinite(ref[:3]).all()
    assert_moments(ref.copy(), ref, mi, RTOL)
    assert_moments(ref.copy(), ref, mi, 0.)


@pytest.mark.parametrize('d', [2, 3])
def test_a_nan_against_a_number_and_a_nan_in_another_place_fail(d):
    mi, ref = _table(d)
    got = ref.copy()
    got[0, _index(mi, 2 * np.eye(d, dtype=int)[0])] = np.nan
    _refused(got, ref, mi)
    _refused(ref, got, mi)
    moved = ref.copy()
    moved[[2, 3]] = ref[[3, 2]]            # the NaN row one step early, numbers where the reference is NaN
    _refused(moved, ref, mi)


@pytest.mark.parametrize('d', [2, 3])
def test_one_moment_off_by_two_rtol_fails(d):
    mi, ref = _table(d)
    j = second(mi)[d - 1]
    assert abs(ref[1, j]) == pytest.approx(_natural(d, 1, mi[j]))      # a moment that is its own denominator, not the floor
    got = ref.copy()
    got[1, j] *= 1. + 2e-6
    _refused(got, ref, mi)
    got[1, j] = ref[1, j] * (1. + 0.5e-6)
    assert_moments(got, ref, mi, RTOL)


@pytest.mark.parametrize('d', [2, 3])
def test_the_floor_of_a_moment_whose_reference_is_zero(d):
    """The denominator of moment n is max(|ref|, 1e-2 natural + 1e-300) with natural = prod_k sigma_k^{n_k}.  For an odd
    moment of a symmetric law ref = 0, so the error is |got| / (1e-2 natural): at rtol = 1e-6 the assertion accepts
    |got| <= 1e-6 * 1e-2 natural = 1e-8 natural and nothing larger.  1e-9 of the natural magnitude passes (error 1e-7);
    2e-2 of it fails (error 2, which is 2e6 rtol); 0.9e-8 and 1.1e-8 pin the figure from both sides."""
    mi, ref = _table(d)
    n = 3 * np.eye(d, dtype=int)[0]
    j, t = _index(mi, n), 2
    assert ref[t, j] == 0.
    nat = _natural(d, t, n)
    for frac, passes in ((1e-9, True), (2e-2, False), (0.9e-8, True), (1.1e-8, False), (-0.9e-8, True), (-1.1e-8, False)):
        got = ref.copy()
        got[t, j] = frac * nat
        if passes:
            assert_moments(got, ref, mi, RTOL)
        else:
            _refused(got, ref, mi)


def test_first_bad_takes_the_earliest_step_over_moments_means_and_scales():
    T, z = 6, 10
    r = {'m': np.ones((T, z)), 'mean': np.zeros((T, 2)), 'nell': 1.}
    assert first_bad(r) == -1
    r['m'][3:] = np.nan
    assert first_bad(r) == 3
    r['mean'][2:, 1] = np.inf              # the mean goes one step before the moments
    assert first_bad(r) == 2
    r['scale'] = np.ones((T, 2))
    r['scale'][1, 0] = np.nan
    assert first_bad(r) == 1
    assert first_bad({'m': np.ones((T, z))}) == -1


def _normal_moment(m, s, n, central):
    """E[(X - c)^n] of X ~ N(m, s^2) about c = m or 0, by the binomial sum over the central moments (k - 1)!! s^k."""
    cen = [0. if k % 2 else s ** k * math.prod(range(k - 1, 0, -2)) for k in range(n + 1)]
    return cen[n] if central else sum(math.comb(n, k) * m ** (n - k) * cen[k] for k in range(n + 1))


@pytest.mark.parametrize('d,N', [(2, 2), (2, 4), (3, 2), (3, 3)])
def test_initial_is_the_normal_law_in_the_order_of_the_tables(d, N):
    mi, _ = tables(d, N)
    mean = MEAN[d]
    L = np.tril(0.1 + 0.05 * np.arange(d * d).reshape(d, d))
    cov = L @ L.T                                                   # correlated
    st = initial(mi, mean, cov)
    assert list(st) == ['rms', 'cms', 'scms', 'mean', 'scale']
    assert all(st[k].shape == (mi.shape[0],) for k in ('rms', 'cms', 'scms'))
    eye = np.eye(d, dtype=int)
    zero = _index(mi, 0 * eye[0])
    assert st['rms'][zero] == pytest.approx(1., rel=1e-15) and st['cms'][zero] == pytest.approx(1., rel=1e-15)
    for i in range(d):
        assert st['rms'][_index(mi, eye[i])] == pytest.approx(mean[i], rel=1e-13)
        assert abs(st['cms'][_index(mi, eye[i])]) <= 1e-18
        assert st['scms'][_index(mi, 2 * eye[i])] == pytest.approx(1., rel=1e-13)
        for j in range(d):
            assert st['cms'][_index(mi, eye[i] + eye[j])] == pytest.approx(cov[i, j], rel=1e-13)
            assert st['rms'][_index(mi, eye[i] + eye[j])] == pytest.approx(cov[i, j] + mean[i] * mean[j], rel=1e-13)
    npt.assert_array_equal(st['mean'], mean)
    npt.assert_allclose(st['scale'], np.sqrt(np.diag(cov)), rtol=1e-15)
    npt.assert_allclose(st['scms'], st['cms'] / np.prod(st['scale'] ** mi, axis=-1), rtol=1e-15)
    # every entry, where the law is a product: entry z is the moment of multi-index mi[z] (Kan's alternating sum of terms of
    # size <= 1 leaves a few ulp of 1 where the moment is 0)
    st = initial(mi, mean, np.diag(SD[d] ** 2))
    for key, central in (('rms', False), ('cms', True)):
        want = [math.prod(_normal_moment(mean[k], SD[d][k], int(n[k]), central) for k in range(d)) for n in mi]
        npt.assert_allclose(st[key], want, rtol=1e-12, atol=1e-15)


def _result():
    m = np.arange(24, dtype=np.float64).reshape(2, 3, 4) / 7.
    m[1, 1:] = np.nan                                               # a replicate poisoned at step 1
    mean = np.array([[[0.5, -0.25]] * 3, [[1.5, 0.]] + [[np.nan, np.nan]] * 2])
    return {'m': m, 'mean': mean, 'nell': np.array([3.25, np.nan]), 'fn': np.array([-1, 1], dtype=np.int32)}


def test_same_bits_accepts_equal_results_and_refuses_a_flipped_bit_and_a_missing_key():
    same_bits(_result(), _result())
    raw = {k: v for k, v in _result().items() if k != 'mean'}
    same_bits(raw, dict(raw))                                       # a raw-mode result has no means on either side
    flipped = _result()
    flipped['m'].view(np.uint64)[0, 0, 1] ^= 1
    assert np.allclose(flipped['m'], _result()['m'], rtol=1e-15, equal_nan=True)      # a comparison of values would pass
    for a, b in ((_result(), flipped), (flipped, _result()), (_result(), raw), (raw, _result())):
        with pytest.raises(AssertionError):
            same_bits(a, b)
