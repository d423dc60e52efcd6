"""tests/one_dim_support.py itself, on the CPU and without the library: what run_oracle returns against oracle/one_dim.py called
directly, what assert_moments and the two poison checks accept and refuse, that the paired models are cached, and that a
missing fixture fails with its hint.  A shared helper that got weaker would fail here, not pass silently everywhere else."""
import math

import numpy as np
import pytest

from mfs_amd import synth
from oracle import one_dim as o
from tests.one_dim_support import (MODES, assert_moments, assert_poisoned_after, assert_poisoned_from, benes, load_golden,
                                   ou_gaussian, run_oracle, well)

N, T, B = 3, 4, 2


def _direct(mode, m, ys, stable):
    """The oracle's filter of `mode` on each replicate, every argument written out."""
    f, s0 = m.ofns, math.sqrt(m.ic.variance)
    if mode == 'raw':
        return [o.moment_filter_rms(f[0], m.opmf, m.oic.rms, y, stable=stable) for y in ys]
    if mode == 'central':
        return [o.moment_filter_cms(f[1], f[3], m.opmf, m.oic.cms, m.oic.mean, y, stable=stable) for y in ys]
    return [o.moment_filter_scms(f[2], f[4], m.opmf, m.oic.scms, m.oic.mean, s0, y, stable=stable) for y in ys]


@pytest.mark.parametrize('stable', [False, True])
@pytest.mark.parametrize('mode', MODES)
def test_run_oracle_is_the_direct_call_stacked(mode, stable):
    m = benes(N, 'tme', 2)
    ys, _ = synth.benes_bernoulli_batch(B, T, m.dt, seed=1)
    run = run_oracle(mode, m, ys, stable=stable)
    ref = _direct(mode, m, ys, stable)
    assert run.moments.shape == (B, T, 2 * N) and run.nell.shape == (B,) and run.first_nan is None
    assert (run.means is None) == (mode == 'raw') and (run.scales is None) == (mode != 'scaled')
    present = [x for x in run[:4] if x is not None]
    assert len(present) == len(ref[0])
    for k, x in enumerate(present):
        assert np.all(np.isfinite(x)) and x.shape[:2] == ((B,) if k == len(present) - 1 else (B, T))
        for b in range(B):
            assert np.array_equal(x[b], ref[b][k]), (mode, k, b)        # finite, so equal values are equal bits


def _normal_central(v):
    return np.array([[1., 0., s, 0., 3. * s * s, 0.] for s in v])


def test_assert_moments():
    ref = _normal_central([0.5, 1., 2., 1.5])
    assert_moments(ref.copy(), ref)
    got = ref.copy()
    got[2, 4] *= 1. + 2e-6                                   # an even order, relative
    with pytest.raises(AssertionError, match='max scaled error'):
        assert_moments(got, ref)
    got = ref.copy()
    got[1, 2] = np.nan
    with pytest.raises(AssertionError, match='NaN pattern'):
        assert_moments(got, ref)
    # an odd order is zero here: its floor is 1e-3 of the larger neighbouring column maximum, 3 * 2^2 of order 4
    floor = 1e-3 * 12.
    got = ref.copy()
    got[1, 3] = 0.9e-6 * floor
    assert_moments(got, ref)
    got[1, 3] = 2e-6 * floor
    with pytest.raises(AssertionError, match='max scaled error'):
        assert_moments(got, ref)
    with pytest.raises(AssertionError):
        assert_moments(ref[:, :4], ref)


def _poisoned():
    """(moments (3, 5, 4), means (3, 5), nell (3,), first_nan): replicate 0 lives, 1 is poisoned at step 2, 2 at step 0."""
    first_nan = np.array([-1, 2, 0])
    means = np.arange(15, dtype=float).reshape(3, 5)
    moments = np.ones((3, 5, 4))
    nell = np.array([1.5, np.nan, np.nan])
    means[1, 2:], means[2, :], moments[1, 2:], moments[2, :] = np.nan, np.nan, np.nan, np.nan
    return moments, means, nell, first_nan


@pytest.mark.parametrize('edit,strict,lenient', [
    (None, True, True),
    ('finite at the poisoned step', False, True),
    ('finite after the poisoned step', False, False),
    ('finite moments after the poisoned step', False, False),
    ('NaN before the poisoned step', False, False),
    ('finite NLL of a poisoned replicate', False, False),
])
def test_the_two_poison_checks(edit, strict, lenient):
    moments, means, nell, first_nan = _poisoned()
    if edit == 'finite at the poisoned step':
        means[1, 2], moments[1, 2] = 0.3, 0.3
    elif edit == 'finite after the poisoned step':
        means[1, 3] = 0.3
    elif edit == 'finite moments after the poisoned step':
        moments[1, 4, 1] = 0.3
    elif edit == 'NaN before the poisoned step':
        means[1, 1] = np.nan
    elif edit == 'finite NLL of a poisoned replicate':
        nell[1] = 2.
    for check, accepts in ((assert_poisoned_from, strict), (assert_poisoned_after, lenient)):
        if accepts:
            check(moments, means, nell, first_nan)
        else:
            with pytest.raises(AssertionError):
                check(moments, means, nell, first_nan)
    if edit is None:
        assert_poisoned_from(None, means, nell, first_nan)       # a run without a moments buffer


def test_paired_models_are_cached():
    assert benes(N, 'tme', 2) is benes(N, 'tme', 2) and benes(N, 'tme', 2) is not benes(N, 'tme', 3)
    assert benes(N).start.cms.shape == (2 * N,) and benes(N + 1).start.cms.shape == (2 * N + 2,)
    assert benes(N).ofns is benes(N).ofns
    assert well(N, 2.5) is well(N, 2.5) and well(N, 2.5) is not well(N, 3.5)
    assert well(N, (1., 2.), 'euler', None, (3., 4.)) is well(N, (1., 2.), 'euler', None, (3., 4.))
    assert ou_gaussian(N) is ou_gaussian(N) and ou_gaussian(N).start.cms.shape != ou_gaussian(N + 1).start.cms.shape


def test_load_golden(tmp_path):
    with pytest.raises(pytest.fail.Exception, match='absent.npz is missing: run the generator'):
        load_golden(str(tmp_path), 'absent.npz', 'run the generator')
    np.savez(tmp_path / 'there.npz', x=np.arange(3))
    assert np.array_equal(load_golden(str(tmp_path), 'there.npz', 'unused')['x'], np.arange(3))
