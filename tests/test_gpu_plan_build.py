"""Which kernel build a 1-D plan picks (csrc/capi_1d.hip: pick_slot for the path and lane group, resolve_launch for the
build), read back through mfs_plan_1d_kernel_build and mfs_plan_1d_geometry.  The expected codes are written down from
those rules: a dense slot runs the dense build; a fast slot runs, with at most four blocks per compute unit, the
specialised one-wave build if the plain kernel has one for the table shape (N = 14..16, 2 / 4 / 6 operator terms or a
Normal closure, degree <= 3, MFS_FAST_BUILD != generic), else the generic one-wave build if the order has one
(N = 14..16), else -- and always above four blocks per compute unit -- the two-wave fast build."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest
import torch

from mfs_amd import _lib, synth
from mfs_amd.one_dim import filtering, moments, ss_models

pytestmark = pytest.mark.gpu

DENSE, FAST, ONE_WAVE, ONE_WAVE_SPEC = 0, 1, 2, 3   # MFS_BUILD_* of include/mfs_hip.h
T = 2


def _benes(N, order):
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli(N)
    _, c, _, mu, _ = moments.sde_cond_moments_tme(drift, dispersion, dt, order)
    tables, lik = filtering.trace_model('central', c, mu, pmf)
    return dt, ic, tables, lik


def _model(N, order, B, n_terms=None):
    """(mfs_model_1d, keep-alive).  n_terms: the same model with its operator table re-declared as one of that many terms
    (zero rows; such a plan is created and asked for its build, never run)."""
    _, _, tables, lik = _benes(N, order)
    model, keep = filtering.build_model_struct(tables, lik, B)
    if n_terms is not None:
        coef = np.zeros((n_terms + 1, model.degree + 1))
        model.n_terms, model.n_rows, model.coef = n_terms, n_terms + 1, coef.ctypes.data_as(_lib.c_double_p)
        keep = (keep, coef)
    return model, keep


def _create(model, N, B, stable=0):
    plan = C.c_void_p()
    _lib.check(_lib.lib().mfs_plan_1d_create(C.byref(plan), C.byref(model), 1, N, T, B, stable, 0, 0))
    return plan


def _describe(plan):
    """(build, lanes per filter, filters per block, grid)"""
    L = _lib.lib()
    build, G, fpb, grid, lds = (C.c_int(-1) for _ in range(5))
    _lib.check(L.mfs_plan_1d_kernel_build(plan, C.byref(build)))
    _lib.check(L.mfs_plan_1d_geometry(plan, C.byref(G), C.byref(fpb), C.byref(grid), C.byref(lds)))
    return build.value, G.value, fpb.value, grid.value


def _four_blocks_per_cu_plus_one(fpb):
    return torch.cuda.get_device_properties(0).multi_processor_count * 4 * fpb + 1


# id: (N, TME order, operator terms re-declared, environment, stable, batch (None: just above four blocks per compute
#      unit), expected build, expected lanes per filter)
CASES = {
    'N7_no_wide_build_plain_fast_at_G8': (7, 3, None, {}, 0, 8, FAST, 8),
    'N15_two_terms_specialised_one_wave': (15, 1, None, {}, 0, 8, ONE_WAVE_SPEC, 16),
    'N15_two_terms_generic_switch_one_wave': (15, 1, None, {'MFS_FAST_BUILD': 'generic'}, 0, 8, ONE_WAVE, 16),
    'N15_two_terms_stable_extended_never_spec': (15, 1, None, {}, 1, 8, ONE_WAVE, 16),
    'N15_five_terms_no_spec_shape_one_wave': (15, 1, 5, {}, 0, 8, ONE_WAVE, 16),
    'N15_two_terms_above_four_blocks_per_cu_two_wave': (15, 1, None, {}, 0, None, FAST, 16),
    'N15_dense_solver': (15, 1, None, {'MFS_SOLVER': 'dense'}, 0, 8, DENSE, 16),
    'N20_G32_no_wide_build': (20, 3, None, {}, 0, 8, FAST, 32),
}


@pytest.mark.parametrize('case', list(CASES))
def test_plan_picks_the_build(case, monkeypatch):
    N, order, n_terms, env, stable, B, want_build, want_G = CASES[case]
    for name in ('MFS_SOLVER', 'MFS_LANES_PER_FILTER', 'MFS_FAST_BUILD'):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if B is None:
        B = _four_blocks_per_cu_plus_one(64 // want_G)
    model, keep = _model(N, order, B, n_terms)
    if N == 15 and n_terms is None:
        assert model.n_terms == 2 and model.degree <= 3      # the table shape the case is about
    plan = _create(model, N, B, stable)
    try:
        build, G, fpb, grid = _describe(plan)
    finally:
        _lib.check(_lib.lib().mfs_plan_1d_destroy(plan))
    del keep
    print(f'{case}: build {build}, G {G}, filters per block {fpb}, grid {grid}')
    assert build == want_build
    assert G == want_G
    if want_build != DENSE:
        assert fpb == 64 // G           # blocks of the fast path are single waves
    assert grid == -(-B // fpb)
    if case == 'N15_two_terms_above_four_blocks_per_cu_two_wave':
        assert grid == 4 * torch.cuda.get_device_properties(0).multi_processor_count + 1


def _run(N, B, ys, ic, model):
    """One run of a plan on device-resident buffers: (moments, means, nell, first_nan), and the build the plan picked."""
    L = _lib.lib()
    plan = _create(model, N, B)
    build = _describe(plan)[0]
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
    return out, build


def test_the_two_one_wave_builds_give_the_same_bits(monkeypatch):
    """The specialised and the generic one-wave build of the N = 15 two-term model on the same seeded inputs: equal bit
    for bit, NaNs included (the specialisation removes loads, dead rows and branches, never an operation that feeds an
    output)."""
    N, B = 15, 8
    for name in ('MFS_SOLVER', 'MFS_LANES_PER_FILTER', 'MFS_FAST_BUILD', 'MFS_PREDICT_RULE'):
        monkeypatch.delenv(name, raising=False)
    dt, ic, _, _ = _benes(N, 1)
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=1815)
    model, keep = _model(N, 1, B)
    spec, build_spec = _run(N, B, ys, ic, model)
    monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
    generic, build_generic = _run(N, B, ys, ic, model)
    del keep
    assert build_spec == ONE_WAVE_SPEC and build_generic == ONE_WAVE
    for x, y in zip(spec, generic):
        assert x.shape == y.shape and x.dtype == y.dtype
        if x.dtype == np.float64:
            nx, ny = np.isnan(x), np.isnan(y)
            npt.assert_array_equal(nx, ny)
            npt.assert_array_equal(x.view(np.int64)[~nx], y.view(np.int64)[~ny])
        else:
            npt.assert_array_equal(x, y)
    assert np.isfinite(spec[2]).all()       # two steps poison nothing: the comparison is of numbers
