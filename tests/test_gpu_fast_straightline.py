"""The update-half eigenvalue iteration of the specialised one-wave builds of the fast 1-D kernel (csrc/filter1d_fast.hpp,
kSlEigLoop: first Laguerre evaluation outside the loop, then a loop with a wave-uniform exit in which groups that have
converged ride along) against the generic build of the same kernel, through the plan API of the C ABI.  The change removes
control flow -- never a floating-point operation that feeds an output -- so every comparison is equality of bits, NaNs included.

Shapes: N = 14, 15 (sixteen lanes per filter: four replicates per wave) and 16 (thirty-two: two per wave); B = 6 leaves a
partial last wave; T <= 300, in one launch and in chunks of 16.  The models are the three (model, transition) pairs with a
fixed-traits build and Benes-Bernoulli with TME-2 tables (4 operator terms), a specialised shape with run-time traits."""
import ctypes as C
import functools

import numpy as np
import pytest

from mfs_amd import _lib, synth
from mfs_amd.one_dim import filtering, moments, ss_models
from tests.test_gpu_fast_traits import (COMBOS, IDENTITY_GAUSSIAN, ONE_WAVE, ONE_WAVE_SPEC, RUNTIME, TANH_BERNOULLI,
                                        _assert_identical, _model)

pytestmark = pytest.mark.gpu

B = 6
# what the default plan must report per model: the three fixed-traits pairs, and the run-time-traits specialised shape
TRAITS = dict(COMBOS, benes_tme2=RUNTIME)
assert TRAITS['benes_tme3'] == TANH_BERNOULLI and TRAITS['ou_normal'] == IDENTITY_GAUSSIAN


@functools.lru_cache(maxsize=None)
def _traced(combo, N):
    """(ic, tables, lik, dt) in central mode; traced once per session."""
    if combo != 'benes_tme2':
        return _model(combo, N)
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli(N)
    fns = moments.sde_cond_moments_tme(drift, dispersion, dt, 2)
    tables, lik = filtering.trace_model('central', fns[1], fns[3], pmf)
    return ic, tables, lik, dt


def _run(combo, N, ys, m0, *, chunk=0, moments_out=True):
    """One central-mode plan run on (B, T) measurements and (B, 2N) start moments:
    ((moments, means, nell, first_nan), build, traits)."""
    ic, tables, lik, _ = _traced(combo, N)
    nb, T = ys.shape
    L = _lib.lib()
    model, keep = filtering.build_model_struct(tables, lik, nb)
    plan = C.c_void_p()
    _lib.check(L.mfs_plan_1d_create(C.byref(plan), C.byref(model), 1, N, T, nb, 0, chunk, 0))
    build, traits = C.c_int(-1), C.c_int(-1)
    _lib.check(L.mfs_plan_1d_kernel_build(plan, C.byref(build)))
    _lib.check(L.mfs_plan_1d_kernel_traits(plan, C.byref(traits)))
    d_m0 = _lib.DeviceBuffer.from_array(np.ascontiguousarray(m0))
    d_mean0 = _lib.DeviceBuffer.from_array(np.full(nb, ic.mean))
    d_ys = _lib.DeviceBuffer.from_array(np.ascontiguousarray(ys))
    d_mom = _lib.DeviceBuffer(nb * T * 2 * N * 8) if moments_out else None
    d_means, d_nell, d_fn = _lib.DeviceBuffer(nb * T * 8), _lib.DeviceBuffer(nb * 8), _lib.DeviceBuffer(nb * 4)
    stream = C.c_void_p()
    _lib.check(L.mfs_stream_create(C.byref(stream)))
    _lib.check(L.mfs_plan_1d_run(plan, d_m0.ptr, 1, d_mean0.ptr, None, d_ys.ptr, d_mom.ptr if d_mom else None, d_means.ptr,
                                 None, d_nell.ptr, d_fn.ptr, stream))
    _lib.check(L.mfs_stream_synchronize(stream))
    out = (d_mom.to_array((nb, T, 2 * N)) if d_mom else np.zeros(0), d_means.to_array((nb, T)), d_nell.to_array((nb,)),
           d_fn.to_array((nb,), np.int32))
    _lib.check(L.mfs_plan_1d_destroy(plan))
    _lib.check(L.mfs_stream_destroy(stream))
    del keep
    return out, build.value, traits.value


def _three_builds(monkeypatch, combo, N, ys, m0, **kw):
    """The default plan, the run-time-traits specialised build and the generic build agree on every output.  Returns the
    default plan's and the generic build's outputs."""
    monkeypatch.delenv('MFS_FAST_BUILD', raising=False)
    monkeypatch.delenv('MFS_FAST_TRAITS', raising=False)
    default, build_d, traits_d = _run(combo, N, ys, m0, **kw)
    monkeypatch.setenv('MFS_FAST_TRAITS', 'runtime')
    runtime, build_r, traits_r = _run(combo, N, ys, m0, **kw)
    monkeypatch.delenv('MFS_FAST_TRAITS')
    monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
    generic, build_g, traits_g = _run(combo, N, ys, m0, **kw)
    monkeypatch.delenv('MFS_FAST_BUILD')
    assert (build_d, traits_d) == (ONE_WAVE_SPEC, TRAITS[combo])
    assert (build_r, traits_r) == (ONE_WAVE_SPEC, RUNTIME)
    assert (build_g, traits_g) == (ONE_WAVE, RUNTIME)
    _assert_identical(default, generic)
    _assert_identical(runtime, generic)
    return default, generic


def _start(combo, N, nb):
    return np.tile(_traced(combo, N)[0].cms, (nb, 1))


@functools.lru_cache(maxsize=None)
def _bernoulli_ys(N, T, seed):
    return synth.benes_bernoulli_batch(B, T, ss_models.benes_bernoulli(N)[0], seed=seed)[0]


@pytest.fixture(autouse=True)
def _default_rule(monkeypatch):
    monkeypatch.delenv('MFS_PREDICT_RULE', raising=False)


# ---- 1. three builds agree, whole and chunked; 4. the NLL-only call on the same inputs
@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(TRAITS))
def test_three_builds_agree(combo, N, monkeypatch):
    ys, m0 = _bernoulli_ys(N, 48, 3100 + N), _start(combo, N, B)
    whole, _ = _three_builds(monkeypatch, combo, N, ys, m0)
    assert np.isfinite(whole[0][:, 0]).all()
    chunked, _ = _three_builds(monkeypatch, combo, N, ys, m0, chunk=16)
    _assert_identical(chunked, whole)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(TRAITS))
def test_nll_only_call(combo, N, monkeypatch):
    """out_moments = NULL: the three builds agree, and means, NLL and first_nan are those of the call with moments."""
    ys, m0 = _bernoulli_ys(N, 48, 3100 + N), _start(combo, N, B)
    nll_only, _ = _three_builds(monkeypatch, combo, N, ys, m0, moments_out=False)
    full, _, _ = _run(combo, N, ys, m0)
    _assert_identical(nll_only[1:], full[1:])
    chunked, _ = _three_builds(monkeypatch, combo, N, ys, m0, moments_out=False, chunk=16)
    _assert_identical(chunked, nll_only)


# ---- 2. a replicate does not depend on its wave neighbours
def _unlike_replicates(combo, N, T):
    """One wave of four unlike replicates: (ys (4, T), m0 (4, 2N)).  0: ordinary measurements; 1: a surprise mid-run, which
    moves the posterior away from the prediction the eigenvalue iteration starts from, so this group needs more evaluations
    than its neighbours; 2: near-constant measurements; 3: a point-mass start, poisoned at step 0 (the second pivot of the first
    rule is 0, not > 0) -- as test_gpu_fast_traits.test_poisoned_group_next_to_live_groups builds it."""
    rng = np.random.default_rng(3200 + N)
    ys = np.empty((4, T))
    if combo == 'ou_normal':
        dt, ell, sigma = 0.1, 1., 0.5
        F, q = np.exp(-dt / ell), sigma * np.sqrt(1 - np.exp(-2 * dt / ell))
        x = np.empty(T)
        x[0] = sigma * rng.standard_normal()
        for t in range(1, T):
            x[t] = F * x[t - 1] + q * rng.standard_normal()
        ys[0] = x + rng.standard_normal(T)
        ys[1] = ys[0][::-1]
        ys[1, T // 2] = 9.                              # nine standard deviations of the measurement noise
        ys[2] = 0.25 + 1e-9 * rng.standard_normal(T)
        ys[3] = ys[0]
    else:
        full = synth.benes_bernoulli_batch(4, T, ss_models.benes_bernoulli(N)[0], seed=3300 + N)[0]
        ys[0] = full[0]
        ys[1, :T // 2], ys[1, T // 2:] = 1., 0.         # a long run of ones, then only zeros
        ys[2] = 0.
        ys[3] = full[3]
    m0 = _start(combo, N, 4)
    m0[3, 1:] = 0.
    return ys, m0


@pytest.mark.parametrize('combo,N', [('ou_normal', 14), ('ou_normal', 15), ('benes_tme3', 15)])
def test_replicate_does_not_depend_on_its_wave_neighbours(combo, N, monkeypatch):
    """Groups that have converged ride along with the slowest group of their wave, and a poisoned group sits the iteration
    out: the outputs of a replicate are the same in two different slot orders of one wave and alone in a wave (B = 1)."""
    monkeypatch.delenv('MFS_FAST_BUILD', raising=False)
    monkeypatch.delenv('MFS_FAST_TRAITS', raising=False)
    T = 64
    ys, m0 = _unlike_replicates(combo, N, T)
    together = {}
    for order in ([0, 1, 2, 3], [3, 2, 0, 1]):
        out, build, traits = _run(combo, N, ys[order], m0[order])
        assert (build, traits) == (ONE_WAVE_SPEC, TRAITS[combo])
        inverse = np.argsort(order)
        together[tuple(order)] = [x[inverse] for x in out]
    first, second = together.values()
    assert first[3][3] == 0 and (first[3][:3] != 0).all()      # first_nan: replicate 3 is poisoned at step 0, the others not there
    _assert_identical(first, second)
    for r in range(4):
        alone, build, traits = _run(combo, N, ys[r:r + 1], m0[r:r + 1])
        assert (build, traits) == (ONE_WAVE_SPEC, TRAITS[combo])
        _assert_identical(alone, [x[r:r + 1] for x in first])
    # and the generic build computes the same wave
    monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
    generic, build_g, _ = _run(combo, N, ys, m0)
    assert build_g == ONE_WAVE
    _assert_identical(first, generic)


# ---- 3. poisoning mid-run
# (N, T, seed) chosen with the CPU oracle (oracle/c) on Benes-Bernoulli, TME-3, B = 6: first poisoned steps
#   N = 14: [166, 157, 206, -, 213, -]    N = 15: [-, -, 118, 219, -, 91]    N = 16: [149, -, 123, -, 72, 121]
# so every wave (four replicates at N = 14, 15; two at N = 16) holds replicates that are poisoned mid-run, in whichever half
# of a step their pivot fails, next to replicates that live to T.
MID_RUN = {14: (300, 2943), 15: (300, 2952), 16: (200, 2966)}


@pytest.mark.parametrize('N', [14, 15, 16])
def test_poisoning_mid_run(N, monkeypatch):
    T, seed = MID_RUN[N]
    ys, m0 = _bernoulli_ys(N, T, seed), _start('benes_tme3', N, B)
    default, generic = _three_builds(monkeypatch, 'benes_tme3', N, ys, m0)
    # the precondition, on the generic build: some wave has a replicate poisoned mid-run next to one that lives to T
    first_nan = generic[3]
    per_wave = 64 // (16 if N <= 15 else 32)
    waves = [first_nan[i:i + per_wave] for i in range(0, B, per_wave)]
    assert any(((w > 0) & (w < T - 1)).any() and (w < 0).any() for w in waves), first_nan
    for b in range(B):
        if first_nan[b] >= 0:
            assert np.isfinite(generic[0][b, :first_nan[b]]).all() and np.isnan(generic[0][b, first_nan[b]:]).all()
    chunked, _ = _three_builds(monkeypatch, 'benes_tme3', N, ys, m0, chunk=16)
    _assert_identical(chunked, default)
    nll_only, _ = _three_builds(monkeypatch, 'benes_tme3', N, ys, m0, moments_out=False)
    _assert_identical(nll_only[1:], default[1:])
