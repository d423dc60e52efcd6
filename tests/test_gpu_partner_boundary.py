"""The step boundary of the partner-wave variant (csrc/filter1d_partner.hpp): the sixteen-step measurement window of the main
wave, the partner's flag word that the main wave acts on inside the next step (and, for the last step, behind the loop), the
eigenvalue loop that freezes only x of a converged lane, and the poison flag taken from a running minimum of the pivots.  None
of them changes a floating-point operation that feeds an output, so every check is equality of bits -- moments, means, NLL,
NaN positions and first_nan -- against the one-wave build (MFS_FAST_PARTNER=0), through the plan API of the C ABI.

Orders N = 14, 15 and the three (model, transition) pairs with a fixed-traits build.  The inputs are the recipes that
tests/test_gpu_fast_partner.py uses (tests/plan_api.py).  The one-wave reference of a set of inputs is computed once, in one
launch, and shared."""
import math

import numpy as np
import pytest

from tests.one_dim_support import assert_poisoned_from
from tests.plan_api import (COMBOS, MID_RUN, MID_RUN_B, assert_same_bits, bernoulli_ys, combo_model, one_wave_build,
                            partner_inputs as _inputs, partner_variant as _partner)

pytestmark = pytest.mark.gpu

CASES = [(combo, N) for combo in sorted(COMBOS) for N in (14, 15)]

_REFERENCES = {}


def _one_wave(monkeypatch, key, combo, N, ys, m0):
    """The one-wave build's outputs on these inputs, whole T in one launch, with moments: computed once per `key`, never
    modified (NLL-only and chunked runs of the variant are compared with the parts of it they produce)."""
    if key not in _REFERENCES:
        out = one_wave_build(monkeypatch, combo, N, ys, m0)
        for x in out:
            if x is not None:
                x.setflags(write=False)
        _REFERENCES[key] = out
    return _REFERENCES[key]


# ---- 1. window edges: launches that end inside the first window, on its last step, on and just behind a window start; the
# guard of the window load meets t_end in the first, second, third and fourth window.  B = 5: a partial wave and three pairs of
# waves without filters; B = 17: a second workgroup.  Replicate 1 is poisoned at step 0, so its flag is acted on in step 1.
@pytest.mark.parametrize('B', [5, 17])
@pytest.mark.parametrize('combo,N', CASES)
def test_window_edges(combo, N, B, monkeypatch):
    for nt in (1, 15, 16, 17, 33, 48):
        ys, m0 = _inputs(combo, N, B, nt)
        variant = _partner(monkeypatch, combo, N, ys, m0)
        assert_same_bits(variant, _one_wave(monkeypatch, ('window', combo, N, B, nt), combo, N, ys, m0))
        assert variant.first_nan[1] == 0 and (np.delete(variant.first_nan, 1) != 0).all()
        assert_poisoned_from(variant.moments, variant.means, variant.nell, variant.first_nan)


# ---- 2. chunk edges: windows are counted from the start of a launch, so with chunks of 1, 7, 16 and 17 steps window starts
# fall before, on and behind chunk starts and the guard of the window load meets t_end inside a window (T = 40 = 5 x 7 + 5 =
# 2 x 16 + 8 = 2 x 17 + 6); with chunks of one step every flag is acted on behind the loop
@pytest.mark.parametrize('moments_out', [True, False])
@pytest.mark.parametrize('combo,N', CASES)
def test_chunk_edges(combo, N, moments_out, monkeypatch):
    nt = 40
    ys, m0 = _inputs(combo, N, 6, nt)
    reference = _one_wave(monkeypatch, ('chunk', combo, N), combo, N, ys, m0)
    part = reference if moments_out else reference[1:]
    for chunk in (0, 1, 7, 16, 17):
        out = _partner(monkeypatch, combo, N, ys, m0, chunk=chunk, moments_out=moments_out)
        assert_same_bits(out if moments_out else out[1:], part)


# ---- 3. the late flag: replicates poisoned mid-run next to live ones.  The (N, T, seed) triples are those of
# test_gpu_fast_partner.test_poisoning_mid_run (Benes-Bernoulli, TME-3, B = 6).  The CPU oracle (oracle/c), re-run for this
# file, gives the first poisoned steps ORACLE_FIRST_NAN.  They say where to look, not what the device must return: a pivot that
# fails is a difference of nearly equal numbers, and the one-wave build's own elimination fails one step earlier on replicate 2
# of N = 14, poisons its replicate 5 at step 178 and keeps replicate 2 of N = 15 alive.  So the steps the checks use are the one-wave build's first_nan of the same
# run, and the oracle's list only has to agree with it on the replicates both poison, to a step.
# For every poisoned replicate the run is repeated in chunks of p + 1 steps (the poisoned step p is the last step of a launch:
# the flag that governs it is acted on behind the loop, and the next launch opens dead) and of p steps (p is the first step of a
# launch: the flag comes from the partner's opening elimination of the carried moments).
ORACLE_FIRST_NAN = {14: [166, 157, 206, -1, 213, -1], 15: [-1, -1, 118, 219, -1, 91]}


def _mid_run(N, monkeypatch):
    nt, seed = MID_RUN[N]
    ys = bernoulli_ys(N, nt, seed, MID_RUN_B)
    m0 = np.tile(combo_model('benes_tme3', N)[0].cms, (ys.shape[0], 1))
    reference = _one_wave(monkeypatch, ('mid', N), 'benes_tme3', N, ys, m0)
    first_nan = reference.first_nan
    # the precondition: replicates poisoned mid-run next to replicates that live to T, in the first wave (replicates 0..3)
    assert ((first_nan[:4] > 0) & (first_nan[:4] < nt - 1)).any() and (first_nan[:4] < 0).any(), first_nan
    both = (first_nan >= 0) & (np.array(ORACLE_FIRST_NAN[N]) >= 0)
    assert both.sum() >= 2 and (np.abs(first_nan - ORACLE_FIRST_NAN[N])[both] <= 1).all(), first_nan
    return nt, ys, m0, reference


@pytest.mark.parametrize('N', [14, 15])
def test_late_flag_mid_run(N, monkeypatch):
    nt, ys, m0, reference = _mid_run(N, monkeypatch)
    variant = _partner(monkeypatch, 'benes_tme3', N, ys, m0)
    np.testing.assert_array_equal(variant.first_nan, reference.first_nan)      # neither a step early nor a step late
    assert_poisoned_from(variant.moments, variant.means, variant.nell, variant.first_nan)
    assert_same_bits(variant, reference)
    assert_same_bits(_partner(monkeypatch, 'benes_tme3', N, ys, m0, moments_out=False)[1:], reference[1:])


@pytest.mark.parametrize('N', [14, 15])
def test_late_flag_at_chunk_edges(N, monkeypatch):
    nt, ys, m0, reference = _mid_run(N, monkeypatch)
    for p in sorted({int(p) for p in reference.first_nan if p >= 0}):
        for chunk in (p + 1, p):      # p = chunk - 1: the last step of the first launch; p = chunk: the first step of the second
            out = _partner(monkeypatch, 'benes_tme3', N, ys, m0, chunk=chunk)
            assert_poisoned_from(out.moments, out.means, out.nell, out.first_nan)
            assert_same_bits(out, reference)


@pytest.mark.parametrize('N', [14, 15])
def test_late_flag_leaves_live_neighbours_alone(N, monkeypatch):
    """The live replicates of the mid-run batches share their wave with replicates that die: each of them alone in a launch
    gives the bits it gives in the batch, which are the one-wave build's."""
    nt, ys, m0, reference = _mid_run(N, monkeypatch)
    batch = _partner(monkeypatch, 'benes_tme3', N, ys, m0)
    live = [b for b in range(ys.shape[0]) if reference.first_nan[b] < 0]
    for b in live:
        assert np.isfinite(batch.moments[b]).all() and np.isfinite(batch.means[b]).all() and np.isfinite(batch.nell[b])
        alone = _partner(monkeypatch, 'benes_tme3', N, ys[b:b + 1], m0[b:b + 1])
        assert_same_bits(alone, batch.rows(slice(b, b + 1)))
        assert_same_bits(alone, reference.rows(slice(b, b + 1)))


# ---- 4. the values of the poison flag: start moments whose Hankel matrix has its first pivot that is not > 0 at position 0,
# in the middle and at N - 1, pivots that are exactly zero, negative, NaN and infinite.  The moments of the standard normal
# law, m_2j = (2j - 1)!!, are integers below 2^53 with pivots d_k = k!; d_k is m_2k minus a function of the lower moments, so
# m_2k - 2 k! leaves the pivots before k alone and makes pivot k = -k!, and m_2k - k! makes it zero up to rounding.  (Through
# the plan API such moments reach the cold rule of step 0, whose elimination flags them pivot by pivot; what the running
# minimum then sees is the NaN they leave behind.  Non-positive pivots inside a run are those of the mid-run tests above.)
def _flag_moments(N):
    normal = np.array([0. if n % 2 else float(np.prod(np.arange(n - 1, 0, -2, dtype=np.float64))) for n in range(2 * N)])
    assert normal[0] == 1. and normal[4] == 3. and normal[2 * N - 2] < 2. ** 53
    rows, names = [], []

    def add(name, edit):
        m = normal.copy()
        edit(m)
        rows.append(m)
        names.append(name)

    mid = N // 2
    add('live', lambda m: None)
    add('pivot 0 zero', lambda m: m.__setitem__(0, 0.))
    add('pivot 0 negative', lambda m: m.__setitem__(0, -1.))
    add('point mass: pivot 1 exactly zero', lambda m: m.__setitem__(slice(1, None), 0.))
    add('middle pivot negative', lambda m: m.__setitem__(2 * mid, m[2 * mid] - 2. * math.factorial(mid)))
    add('last pivot negative', lambda m: m.__setitem__(2 * N - 2, m[2 * N - 2] - 2. * math.factorial(N - 1)))
    add('NaN moment: pivot 3 NaN', lambda m: m.__setitem__(6, np.nan))
    add('inf moment: pivot 3 inf', lambda m: m.__setitem__(6, np.inf))
    add('-inf moment: pivot 3 -inf', lambda m: m.__setitem__(6, -np.inf))
    add('NaN in the last row only', lambda m: m.__setitem__(2 * N - 1, np.nan))
    add('live again', lambda m: None)
    return np.array(rows), names


@pytest.mark.parametrize('combo,N', CASES)
def test_poison_flag_values(combo, N, monkeypatch):
    nt = 20
    m0, names = _flag_moments(N)
    ys = _inputs(combo, N, len(names), nt, poison=False)[0]
    reference = _one_wave(monkeypatch, ('flags', combo, N), combo, N, ys, m0)
    variant = _partner(monkeypatch, combo, N, ys, m0)
    np.testing.assert_array_equal(variant.first_nan, reference.first_nan, err_msg=str(names))
    assert_same_bits(variant, reference)
    first_nan = dict(zip(names, variant.first_nan))
    # m_{2N-1} enters only the last row of the extended matrix: no pivot, a NaN Jacobi entry -- whatever the one-wave build says
    expected_zero = [n for n in names if not n.startswith('live') and n != 'NaN in the last row only']
    assert all(first_nan[n] == 0 for n in expected_zero), first_nan
    assert first_nan['live'] != 0 and first_nan['live again'] != 0, first_nan
    assert_same_bits(_partner(monkeypatch, combo, N, ys, m0, chunk=7), reference)


# ---- 5. the last step's mean is stored behind the loop
@pytest.mark.parametrize('combo,N', CASES)
def test_last_step_mean(combo, N, monkeypatch):
    for nt in (2, 17):
        ys, m0 = _inputs(combo, N, 5, nt)
        reference = _one_wave(monkeypatch, ('window', combo, N, 5, nt), combo, N, ys, m0)
        for chunk in (0, 1):
            means = _partner(monkeypatch, combo, N, ys, m0, chunk=chunk).means
            assert_same_bits([means[:, -1]], [reference.means[:, -1]])
            assert np.isnan(means[1, -1]) and np.isfinite(np.delete(means[:, -1], 1)).all()
