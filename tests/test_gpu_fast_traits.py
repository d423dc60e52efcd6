"""The fixed-traits one-wave builds of the fast 1-D kernel (csrc/filter1d_fast.hpp, StepTraits: moment mode, u-map and
likelihood law compiled in, likelihood parameters in registers, output stores decided before the time loop) against the
same specialised build with run-time traits (MFS_FAST_TRAITS=runtime) and against the generic build
(MFS_FAST_BUILD=generic), through the plan API of the C ABI.  The traits remove branches, LDS reads and dead code -- never a
floating-point operation that feeds an output -- so every comparison here is equality of bits, NaNs included.

Shapes: N = 14, 15 (sixteen lanes per filter) and 16 (thirty-two); B = 6 leaves a partial last wave, so the `b >= B` exit is
live; T = 40 in one launch and in chunks of 16 (16 + 16 + 8) and of 24 (24 + 16: the plan takes one chunk length, so these two
stand for "16 + 24") -- both cross the 16-step measurement window and pass the posterior atoms through the carry."""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats, synth
from mfs_amd.one_dim import filtering, moments, ss_models
from mfs_amd.utils import GaussianSum1D

pytestmark = pytest.mark.gpu

ONE_WAVE, ONE_WAVE_SPEC, FAST = 2, 3, 1                        # MFS_BUILD_* of include/mfs_hip.h
RUNTIME, TANH_BERNOULLI, IDENTITY_GAUSSIAN = 0, 1, 2           # MFS_TRAITS_*
T, B = 40, 6
MODES = {'raw': 0, 'central': 1, 'scaled': 2}
# the (model, transition) pairs that have a fixed-traits build, and the traits code each must report
COMBOS = {'benes_tme3': TANH_BERNOULLI, 'benes_tme_normal3': TANH_BERNOULLI, 'ou_normal': IDENTITY_GAUSSIAN}


@functools.lru_cache(maxsize=None)
def _model(combo, N, mode='central'):
    """(ic, tables, lik, dt) of one model in one moment mode; traced once per session."""
    if combo.startswith('benes'):
        dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli(N)
        if combo == 'benes_tme3':
            fns = moments.sde_cond_moments_tme(drift, dispersion, dt, 3)
        else:
            fns = moments.sde_cond_moments_tme_normal(drift, dispersion, dt, 3, N)
    else:   # the OU / Gaussian workload of the benchmark's config 3
        dt, ell, sigma = 0.1, 1., 0.5
        F, Sigma = np.exp(-dt / ell), sigma ** 2 * (1 - np.exp(-2 * dt / ell))
        ic = GaussianSum1D.new(means=[0.], variances=[sigma ** 2], weights=[1.], N=N)
        pmf = lambda y, x: stats.norm_pdf(y, x, 1.)   # noqa: E731
        fns = moments.sde_cond_moments_normal(lambda x: F * x, lambda x: Sigma)
    mean_fn = fns[3] if mode == 'central' else fns[4] if mode == 'scaled' else None
    tables, lik = filtering.trace_model(mode, fns[MODES[mode]], mean_fn, pmf)
    return ic, tables, lik, dt


@functools.lru_cache(maxsize=None)
def _ys(N):
    """One set of Bernoulli measurements per order, shared by every model (a Gaussian law accepts 0 / 1 as well)."""
    dt = ss_models.benes_bernoulli(N)[0]
    return synth.benes_bernoulli_batch(B, T, dt, seed=2600 + N)[0]


def _plan_run(combo, N, *, mode='central', chunk=0, moments_out=True, poison=False):
    """One run of a plan on device-resident buffers: ((moments | None, means, nell, first_nan), build, traits)."""
    ic, tables, lik, _ = _model(combo, N, mode)
    L = _lib.lib()
    model, keep = filtering.build_model_struct(tables, lik, B)
    plan = C.c_void_p()
    _lib.check(L.mfs_plan_1d_create(C.byref(plan), C.byref(model), MODES[mode], N, T, B, 0, chunk, 0))
    build, traits = C.c_int(-1), C.c_int(-1)
    _lib.check(L.mfs_plan_1d_kernel_build(plan, C.byref(build)))
    _lib.check(L.mfs_plan_1d_kernel_traits(plan, C.byref(traits)))
    m0 = np.tile({'raw': ic.rms, 'central': ic.cms, 'scaled': ic.scms}[mode], (B, 1))
    if poison:
        # replicate 1: a point mass (m_0 = 1, every other central moment 0): the second pivot of the first rule is 0, not > 0,
        # so this group is poisoned at step 0 while the groups next to it in the wave (replicates 0, 2, 3) stay alive
        m0[1, 1:] = 0.
    d_m0 = _lib.DeviceBuffer.from_array(m0)
    d_mean0 = _lib.DeviceBuffer.from_array(np.full(B, ic.mean))
    d_scale0 = _lib.DeviceBuffer.from_array(np.full(B, np.sqrt(ic.variance)))
    d_ys = _lib.DeviceBuffer.from_array(_ys(N))
    d_mom = _lib.DeviceBuffer(B * T * 2 * N * 8) if moments_out else None
    d_means, d_scales = _lib.DeviceBuffer(B * T * 8), _lib.DeviceBuffer(B * T * 8)
    d_nell, d_fn = _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 4)
    for buf in (d_means, d_scales):
        _lib.check(L.mfs_memset(buf.ptr, 0, B * T * 8, None))       # raw mode writes no means, central mode no scales
    _lib.check(L.mfs_device_synchronize())
    stream = C.c_void_p()
    _lib.check(L.mfs_stream_create(C.byref(stream)))
    _lib.check(L.mfs_plan_1d_run(plan, d_m0.ptr, 1, d_mean0.ptr, d_scale0.ptr, d_ys.ptr, d_mom.ptr if d_mom else None,
                                 d_means.ptr, d_scales.ptr, d_nell.ptr, d_fn.ptr, stream))
    _lib.check(L.mfs_stream_synchronize(stream))
    out = (d_mom.to_array((B, T, 2 * N)) if d_mom else np.zeros(0), d_means.to_array((B, T)), d_scales.to_array((B, T)),
           d_nell.to_array((B,)), d_fn.to_array((B,), np.int32))
    _lib.check(L.mfs_plan_1d_destroy(plan))
    _lib.check(L.mfs_stream_destroy(stream))
    del keep
    return out, build.value, traits.value


def _assert_identical(a, b):
    """Bit for bit: the same NaN positions (a poisoned replicate is NaN-filled from its first bad step on) and the same bit
    patterns everywhere else."""
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        if x.dtype == np.float64:
            nx, ny = np.isnan(x), np.isnan(y)
            npt.assert_array_equal(nx, ny)
            npt.assert_array_equal(x.view(np.int64)[~nx], y.view(np.int64)[~ny])
        else:
            npt.assert_array_equal(x, y)


def _differs(a, b):
    return any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _three_builds(monkeypatch, combo, N, **kw):
    """The same run on the fixed-traits build, the run-time-traits specialised build and the generic build."""
    monkeypatch.delenv('MFS_FAST_BUILD', raising=False)
    monkeypatch.delenv('MFS_FAST_TRAITS', raising=False)
    fixed = _plan_run(combo, N, **kw)
    monkeypatch.setenv('MFS_FAST_TRAITS', 'runtime')
    runtime = _plan_run(combo, N, **kw)
    monkeypatch.delenv('MFS_FAST_TRAITS')
    monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
    generic = _plan_run(combo, N, **kw)
    monkeypatch.delenv('MFS_FAST_BUILD')
    return fixed, runtime, generic


def _check_three(monkeypatch, combo, N, **kw):
    (fixed, build_f, traits_f), (runtime, build_r, traits_r), (generic, build_g, traits_g) = \
        _three_builds(monkeypatch, combo, N, **kw)
    assert (build_f, traits_f) == (ONE_WAVE_SPEC, COMBOS[combo])
    assert (build_r, traits_r) == (ONE_WAVE_SPEC, RUNTIME)
    assert (build_g, traits_g) == (ONE_WAVE, RUNTIME)
    _assert_identical(fixed, runtime)
    _assert_identical(fixed, generic)
    return fixed


@pytest.fixture(autouse=True)
def _default_rule(monkeypatch):
    monkeypatch.delenv('MFS_PREDICT_RULE', raising=False)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_fixed_traits_equal_runtime_traits_and_generic(combo, N, monkeypatch):
    """Moments, means, NLL and first_nan of the three builds, in one launch; the fixed-traits build chunked equals itself
    in one launch."""
    fixed = _check_three(monkeypatch, combo, N)
    assert np.isfinite(fixed[0][:, 0]).all()                        # the first step of every replicate is a real number
    assert not fixed[2].any()                                       # central mode: the scales buffer is left alone
    for chunk in (16, 24):
        chunked, build_c, traits_c = _plan_run(combo, N, chunk=chunk)
        assert (build_c, traits_c) == (ONE_WAVE_SPEC, COMBOS[combo])
        _assert_identical(chunked, fixed)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_nll_only_call(combo, N, monkeypatch):
    """out_moments = NULL: means, NLL and first_nan of the three builds agree, and are those of the call with moments."""
    nll_only = _check_three(monkeypatch, combo, N, moments_out=False)
    full, _, _ = _plan_run(combo, N)
    _assert_identical(nll_only[1:], full[1:])
    chunked, _, _ = _plan_run(combo, N, moments_out=False, chunk=16)
    _assert_identical(chunked, nll_only)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_poisoned_group_next_to_live_groups(combo, N, monkeypatch):
    """A replicate whose start makes a pivot non-positive at the first step shares its wave with live replicates."""
    fixed = _check_three(monkeypatch, combo, N, poison=True)
    first_nan = fixed[4]
    assert first_nan[1] == 0 and (np.delete(first_nan, 1) != 0).all()
    assert np.isnan(fixed[0][1]).all() and np.isnan(fixed[3][1])
    clean, _, _ = _plan_run(combo, N)
    _assert_identical([np.delete(x, 1, axis=0) for x in fixed], [np.delete(x, 1, axis=0) for x in clean])
    chunked, _, _ = _plan_run(combo, N, poison=True, chunk=16)
    _assert_identical(chunked, fixed)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_recomputed_predict_rule(combo, N, monkeypatch):
    """MFS_PREDICT_RULE=recompute: the predict half runs the full rule in every build."""
    monkeypatch.setenv('MFS_PREDICT_RULE', 'recompute')
    _check_three(monkeypatch, combo, N)


@pytest.mark.parametrize('mode', ['raw', 'scaled'])
def test_other_modes_keep_runtime_traits(mode, monkeypatch):
    """Raw and scaled plans have no fixed-traits build: they report run-time traits, run, and equal the generic build."""
    monkeypatch.delenv('MFS_FAST_BUILD', raising=False)
    monkeypatch.delenv('MFS_FAST_TRAITS', raising=False)
    spec, build_s, traits_s = _plan_run('benes_tme3', 15, mode=mode)
    assert (build_s, traits_s) == (ONE_WAVE_SPEC, RUNTIME)
    monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
    generic, build_g, traits_g = _plan_run('benes_tme3', 15, mode=mode)
    assert (build_g, traits_g) == (ONE_WAVE, RUNTIME)
    _assert_identical(spec, generic)
    assert spec[2].any() == (mode == 'scaled') and spec[1].any() == (mode == 'scaled')


def test_order_without_a_one_wave_build_keeps_runtime_traits(monkeypatch):
    """N = 13 has no one-wave build, hence no traits build; neither switch changes what it runs."""
    monkeypatch.delenv('MFS_FAST_BUILD', raising=False)
    monkeypatch.delenv('MFS_FAST_TRAITS', raising=False)
    a, build_a, traits_a = _plan_run('benes_tme3', 13)
    monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
    b, build_b, traits_b = _plan_run('benes_tme3', 13)
    assert (build_a, traits_a) == (FAST, RUNTIME) and (build_b, traits_b) == (FAST, RUNTIME)
    _assert_identical(a, b)


@pytest.mark.parametrize('N', [14, 15, 16])
def test_each_traits_build_computes_its_own_model(N, monkeypatch):
    """Would a wrong law or u-map be compiled in, or two registrations be swapped: the OU / Gaussian and the Benes /
    Bernoulli plans (both normal-closure tables, the same table shape) fed the same measurements differ from each other,
    and each equals its own run-time-traits result."""
    monkeypatch.delenv('MFS_FAST_BUILD', raising=False)
    monkeypatch.delenv('MFS_FAST_TRAITS', raising=False)
    ou, _, traits_ou = _plan_run('ou_normal', N)
    benes, _, traits_benes = _plan_run('benes_tme_normal3', N)
    assert (traits_ou, traits_benes) == (IDENTITY_GAUSSIAN, TANH_BERNOULLI)
    assert _differs(ou[:1], benes[:1]) and _differs(ou[3:4], benes[3:4])
    monkeypatch.setenv('MFS_FAST_TRAITS', 'runtime')
    ou_r, _, traits_ou_r = _plan_run('ou_normal', N)
    benes_r, _, traits_benes_r = _plan_run('benes_tme_normal3', N)
    assert (traits_ou_r, traits_benes_r) == (RUNTIME, RUNTIME)
    _assert_identical(ou, ou_r)
    _assert_identical(benes, benes_r)
