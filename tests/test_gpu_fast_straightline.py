"""The update-half eigenvalue iteration of the specialised one-wave builds of the fast 1-D kernel (csrc/filter1d_fast.hpp,
kSlEigLoop: first Laguerre evaluation outside the loop, then a loop with a wave-uniform exit in which groups that have
converged ride along) against the generic build of the same kernel, through the plan API of the C ABI.  The change removes
control flow -- never a floating-point operation that feeds an output -- so every comparison is equality of bits, NaNs included.

Shapes: N = 14, 15 (sixteen lanes per filter: four replicates per wave) and 16 (thirty-two: two per wave); B = 6 leaves a
partial last wave; T <= 300, in one launch and in chunks of 16.  The models are the three (model, transition) pairs with a
fixed-traits build and Benes-Bernoulli with TME-2 tables (4 operator terms), a specialised shape with run-time traits."""
import numpy as np
import pytest

from mfs_amd._lib import BUILD, TRAITS as TRAITS_CODE
from tests.plan_api import (COMBOS, MID_RUN, assert_same_bits, bernoulli_ys, build_switches, run_central, start, three_builds,
                            unlike_replicates)

pytestmark = pytest.mark.gpu

ONE_WAVE, ONE_WAVE_SPEC, RUNTIME = BUILD['fast_one_wave'], BUILD['fast_one_wave_spec'], TRAITS_CODE['runtime']
B = 6
# what the default plan must report per model: the three fixed-traits pairs, and the run-time-traits specialised shape
TRAITS = dict(COMBOS, benes_tme2=RUNTIME)
assert TRAITS['benes_tme3'] == TRAITS_CODE['central_tanh_bernoulli']
assert TRAITS['ou_normal'] == TRAITS_CODE['central_identity_gaussian']


def _three_builds(monkeypatch, combo, N, ys, m0, **kw):
    """The default plan, the run-time-traits specialised build and the generic build agree on every output.  Returns the
    default plan's and the generic build's outputs."""
    (report_d, default), (report_r, runtime), (report_g, generic) = \
        three_builds(monkeypatch, lambda: run_central(combo, N, ys, m0, **kw))
    assert report_d[:2] == (ONE_WAVE_SPEC, TRAITS[combo])
    assert report_r[:2] == (ONE_WAVE_SPEC, RUNTIME)
    assert report_g[:2] == (ONE_WAVE, RUNTIME)
    assert_same_bits(default, generic)
    assert_same_bits(runtime, generic)
    return default, generic


# ---- 1. three builds agree, whole and chunked; 4. the NLL-only call on the same inputs
@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(TRAITS))
def test_three_builds_agree(combo, N, monkeypatch):
    ys, m0 = bernoulli_ys(N, 48, 3100 + N, B), start(combo, N, B)
    whole, _ = _three_builds(monkeypatch, combo, N, ys, m0)
    assert np.isfinite(whole.moments[:, 0]).all()
    chunked, _ = _three_builds(monkeypatch, combo, N, ys, m0, chunk=16)
    assert_same_bits(chunked, whole)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(TRAITS))
def test_nll_only_call(combo, N, monkeypatch):
    """out_moments = NULL: the three builds agree, and means, NLL and first_nan are those of the call with moments."""
    ys, m0 = bernoulli_ys(N, 48, 3100 + N, B), start(combo, N, B)
    nll_only, _ = _three_builds(monkeypatch, combo, N, ys, m0, moments_out=False)
    with build_switches(monkeypatch):
        _, full = run_central(combo, N, ys, m0)
    assert_same_bits(nll_only[1:], full[1:])
    chunked, _ = _three_builds(monkeypatch, combo, N, ys, m0, moments_out=False, chunk=16)
    assert_same_bits(chunked, nll_only)


# ---- 2. a replicate does not depend on its wave neighbours
@pytest.mark.parametrize('combo,N', [('ou_normal', 14), ('ou_normal', 15), ('benes_tme3', 15)])
def test_replicate_does_not_depend_on_its_wave_neighbours(combo, N, monkeypatch):
    """Groups that have converged ride along with the slowest group of their wave, and a poisoned group sits the iteration
    out: the outputs of a replicate are the same in two different slot orders of one wave and alone in a wave (B = 1)."""
    T = 64
    ys, m0 = unlike_replicates(combo, N, T)
    together = {}
    with build_switches(monkeypatch):
        for order in ([0, 1, 2, 3], [3, 2, 0, 1]):
            report, out = run_central(combo, N, ys[order], m0[order])
            assert report[:2] == (ONE_WAVE_SPEC, TRAITS[combo])
            together[tuple(order)] = out.rows(np.argsort(order))
        first, second = together.values()
        # first_nan: replicate 3 is poisoned at step 0, the others not there
        assert first.first_nan[3] == 0 and (first.first_nan[:3] != 0).all()
        assert_same_bits(first, second)
        for r in range(4):
            report, alone = run_central(combo, N, ys[r:r + 1], m0[r:r + 1])
            assert report[:2] == (ONE_WAVE_SPEC, TRAITS[combo])
            assert_same_bits(alone, first.rows(slice(r, r + 1)))
    # and the generic build computes the same wave
    with build_switches(monkeypatch, MFS_FAST_BUILD='generic'):
        report_g, generic = run_central(combo, N, ys, m0)
    assert report_g.build == ONE_WAVE
    assert_same_bits(first, generic)


# ---- 3. poisoning mid-run: the (N, T, seed) triples of plan_api.MID_RUN
@pytest.mark.parametrize('N', [14, 15, 16])
def test_poisoning_mid_run(N, monkeypatch):
    T, seed = MID_RUN[N]
    ys, m0 = bernoulli_ys(N, T, seed, B), start('benes_tme3', N, B)
    default, generic = _three_builds(monkeypatch, 'benes_tme3', N, ys, m0)
    # the precondition, on the generic build: some wave has a replicate poisoned mid-run next to one that lives to T
    first_nan = generic.first_nan
    per_wave = 64 // (16 if N <= 15 else 32)
    waves = [first_nan[i:i + per_wave] for i in range(0, B, per_wave)]
    assert any(((w > 0) & (w < T - 1)).any() and (w < 0).any() for w in waves), first_nan
    for b in range(B):
        if first_nan[b] >= 0:
            assert np.isfinite(generic.moments[b, :first_nan[b]]).all() and np.isnan(generic.moments[b, first_nan[b]:]).all()
    chunked, _ = _three_builds(monkeypatch, 'benes_tme3', N, ys, m0, chunk=16)
    assert_same_bits(chunked, default)
    nll_only, _ = _three_builds(monkeypatch, 'benes_tme3', N, ys, m0, moments_out=False)
    assert_same_bits(nll_only[1:], default[1:])
