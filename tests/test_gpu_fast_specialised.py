"""The specialised one-wave builds of the fast 1-D kernel (coefficient table in registers, live rows only, straight-line
halves: csrc/filter1d_fast.hpp, SPEC) against the generic build of the same kernel, through the plan API of the C ABI.
The specialisation removes loads, dead rows and branches -- never a floating-point operation that feeds an output -- so
every comparison here is equality, NaNs included.  MFS_FAST_BUILD=generic is the A/B switch (read at plan creation)."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, synth
from mfs_amd.one_dim import filtering, moments, ss_models

pytestmark = pytest.mark.gpu

DENSE, FAST, ONE_WAVE, ONE_WAVE_SPEC = 0, 1, 2, 3   # MFS_BUILD_* of include/mfs_hip.h


def _plan_run(N, T, B, chunk, ys, ic, tables, lik):
    """One run of a plan on device-resident buffers: (moments, means, nell, first_nan), and the build the plan picked."""
    L = _lib.lib()
    model, keep = filtering.build_model_struct(tables, lik, B)
    plan = C.c_void_p()
    _lib.check(L.mfs_plan_1d_create(C.byref(plan), C.byref(model), 1, N, T, B, 0, chunk, 0))
    build = C.c_int(-1)
    _lib.check(L.mfs_plan_1d_kernel_build(plan, C.byref(build)))
    d_m0 = _lib.DeviceBuffer.from_array(ic.cms)
    d_mean0 = _lib.DeviceBuffer.from_array(np.array([ic.mean]))
    d_ys = _lib.DeviceBuffer.from_array(ys)
    d_mom, d_means = _lib.DeviceBuffer(B * T * 2 * N * 8), _lib.DeviceBuffer(B * T * 8)
    d_nell, d_fn = _lib.DeviceBuffer(B * 8), _lib.DeviceBuffer(B * 4)
    stream = C.c_void_p()
    _lib.check(L.mfs_stream_create(C.byref(stream)))
    _lib.check(L.mfs_plan_1d_run(plan, d_m0.ptr, 0, d_mean0.ptr, None, d_ys.ptr, d_mom.ptr, d_means.ptr, None, d_nell.ptr,
                                 d_fn.ptr, stream))
    _lib.check(L.mfs_stream_synchronize(stream))
    out = (d_mom.to_array((B, T, 2 * N)), d_means.to_array((B, T)), d_nell.to_array((B,)), d_fn.to_array((B,), np.int32))
    _lib.check(L.mfs_plan_1d_destroy(plan))
    _lib.check(L.mfs_stream_destroy(stream))
    del keep
    return out, build.value


def _benes(N, family, order):
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli(N)
    if family == 'tme':
        _, c, _, mu, _ = moments.sde_cond_moments_tme(drift, dispersion, dt, order)
    else:
        _, c, _, mu, _ = moments.sde_cond_moments_tme_normal(drift, dispersion, dt, order, N)
    tables, lik = filtering.trace_model('central', c, mu, pmf)
    return dt, ic, tables, lik


def _assert_identical(a, b):
    """Bit for bit: the same NaN positions (poisoned replicates are NaN-filled from their first bad step on) and the same
    bit patterns everywhere else."""
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        if x.dtype == np.float64:
            nx, ny = np.isnan(x), np.isnan(y)
            npt.assert_array_equal(nx, ny)
            npt.assert_array_equal(x.view(np.int64)[~nx], y.view(np.int64)[~ny])
        else:
            npt.assert_array_equal(x, y)


def _both_builds(monkeypatch, N, T, B, chunk, ys, ic, tables, lik):
    monkeypatch.delenv('MFS_FAST_BUILD', raising=False)
    default, build_default = _plan_run(N, T, B, chunk, ys, ic, tables, lik)
    monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
    generic, build_generic = _plan_run(N, T, B, chunk, ys, ic, tables, lik)
    monkeypatch.delenv('MFS_FAST_BUILD')
    return default, build_default, generic, build_generic


@pytest.mark.parametrize('family,order', [('tme', 3), ('tme', 2), ('tme', 1), ('tme_normal', 3)])
def test_specialised_build_equals_generic_build(family, order, monkeypatch):
    """Headline shape in small: N = 15, sixteen lanes per filter, at most one wave per SIMD.  TME-3 is the headline's table
    (6 operator terms + variance); TME-2 / TME-1 / TME-normal-3 are the other specialised shapes.  300 steps poison a good
    part of the replicates at N = 15, and those must stop at the same step with the same numbers before it."""
    N, T, B = 15, 300, 48
    monkeypatch.delenv('MFS_PREDICT_RULE', raising=False)
    dt, ic, tables, lik = _benes(N, family, order)
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=1500 + order)
    spec, build_spec, generic, build_generic = _both_builds(monkeypatch, N, T, B, 0, ys, ic, tables, lik)
    assert build_spec == ONE_WAVE_SPEC and build_generic == ONE_WAVE
    _assert_identical(spec, generic)
    if family == 'tme' and order == 3:
        assert (spec[3] >= 0).any() and (spec[3] < 0).any()     # the case really has poisoned and surviving replicates
    # chunked (the atoms travel in the carry) and with the reference's literal predict-half rule
    chunked, build_chunked = _plan_run(N, T, B, 70, ys, ic, tables, lik)
    assert build_chunked == ONE_WAVE_SPEC
    _assert_identical(chunked, spec)
    monkeypatch.setenv('MFS_PREDICT_RULE', 'recompute')
    spec_r, build_spec_r, generic_r, build_generic_r = _both_builds(monkeypatch, N, T, B, 0, ys, ic, tables, lik)
    assert build_spec_r == ONE_WAVE_SPEC and build_generic_r == ONE_WAVE
    _assert_identical(spec_r, generic_r)


@pytest.mark.parametrize('N', [14, 16])
def test_other_orders_with_a_one_wave_build(N, monkeypatch):
    """N = 14 (sixteen lanes) and N = 16 (thirty-two lanes) are the other two orders that have one-wave builds."""
    T, B = 120, 24
    monkeypatch.delenv('MFS_PREDICT_RULE', raising=False)
    dt, ic, tables, lik = _benes(N, 'tme', 3)
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=1600 + N)
    spec, build_spec, generic, build_generic = _both_builds(monkeypatch, N, T, B, 0, ys, ic, tables, lik)
    assert build_spec == ONE_WAVE_SPEC and build_generic == ONE_WAVE
    _assert_identical(spec, generic)


def test_shapes_and_batches_outside_the_specialised_set_run_the_generic_builds(monkeypatch):
    """TME-4 (8 operator terms) has no specialised build; a batch of more than one wave per SIMD runs the two-wave build;
    N = 13 has no one-wave build at all.  All still run, pick what they picked before, and do not react to the switch."""
    monkeypatch.delenv('MFS_PREDICT_RULE', raising=False)
    N, T = 15, 60
    dt, ic, tables, lik = _benes(N, 'tme', 4)
    ys, _ = synth.benes_bernoulli_batch(32, T, dt, seed=1700)
    a, build_a, b, build_b = _both_builds(monkeypatch, N, T, 32, 0, ys, ic, tables, lik)
    assert build_a == ONE_WAVE and build_b == ONE_WAVE
    _assert_identical(a, b)

    # more than one wave per SIMD: the grid exceeds 4 waves per compute unit
    L = _lib.lib()
    props = C.create_string_buffer(256)
    _lib.check(L.mfs_device_name(0, props, 256))
    cus = int(props.value.decode().rsplit(',', 1)[1].split()[0])     # "... (arch, <n> CUs)"
    B_big = 4 * (4 * cus + 8)                                   # four filters per wave at sixteen lanes per filter
    dt, ic, tables, lik = _benes(N, 'tme', 3)
    T_big = 24
    ys_big, _ = synth.benes_bernoulli_batch(B_big, T_big, dt, seed=1701)
    big, build_big, big_g, build_big_g = _both_builds(monkeypatch, N, T_big, B_big, 0, ys_big, ic, tables, lik)
    assert build_big == FAST and build_big_g == FAST
    _assert_identical(big, big_g)

    dt, ic, tables, lik = _benes(13, 'tme', 3)
    ys13, _ = synth.benes_bernoulli_batch(16, T, dt, seed=1702)
    c, build_c, d, build_d = _both_builds(monkeypatch, 13, T, 16, 0, ys13, ic, tables, lik)
    assert build_c == FAST and build_d == FAST
    _assert_identical(c, d)
