"""Which kernel build a 1-D plan picks (csrc/capi_1d.hip: pick_slot for the path and lane group, resolve_launch for the
build), read back through mfs_plan_1d_kernel_build and mfs_plan_1d_geometry.  The expected codes are written down from
those rules: a dense slot runs the dense build; a fast slot runs, with at most four blocks per compute unit, the
specialised one-wave build if the plain kernel has one for the table shape (N = 14..16, 2 / 4 / 6 operator terms or a
Normal closure, degree <= 3, MFS_FAST_BUILD != generic), else the generic one-wave build if the order has one
(N = 14..16), else -- and always above four blocks per compute unit -- the two-wave fast build."""
import numpy as np
import pytest
import torch

from mfs_amd import _lib, synth
from mfs_amd._lib import BUILD
from mfs_amd.one_dim import filtering
from tests.plan_api import assert_same_bits, benes, build_switches, run_plan_1d

pytestmark = pytest.mark.gpu

DENSE, FAST, ONE_WAVE, ONE_WAVE_SPEC = (BUILD[k] for k in ('dense', 'fast', 'fast_one_wave', 'fast_one_wave_spec'))
T = 2


def _model(N, order, B, n_terms=None):
    """(mfs_model_1d, keep-alive).  n_terms: the same model with its operator table re-declared as one of that many terms
    (zero rows; such a plan is created and asked for its build, never run)."""
    _, _, tables, lik = benes(N, 'tme', order)
    model, keep = filtering.build_model_struct(tables, lik, B)
    if n_terms is not None:
        coef = np.zeros((n_terms + 1, model.degree + 1))
        model.n_terms, model.n_rows, model.coef = n_terms, n_terms + 1, coef.ctypes.data_as(_lib.c_double_p)
        keep = (keep, coef)
    return model, keep


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
    if B is None:
        B = _four_blocks_per_cu_plus_one(64 // want_G)
    model, keep = _model(N, order, B, n_terms)
    if N == 15 and n_terms is None:
        assert model.n_terms == 2 and model.degree <= 3      # the table shape the case is about
    with build_switches(monkeypatch, **env):
        report, _ = run_plan_1d((model, keep), N, T, B, stable=stable, runs=0)
    build, G, fpb, grid = report.build, report.lanes_per_filter, report.filters_per_block, report.grid
    print(f'{case}: build {build}, G {G}, filters per block {fpb}, grid {grid}')
    assert build == want_build
    assert G == want_G
    if want_build != DENSE:
        assert fpb == 64 // G           # blocks of the fast path are single waves
    assert grid == -(-B // fpb)
    if case == 'N15_two_terms_above_four_blocks_per_cu_two_wave':
        assert grid == 4 * torch.cuda.get_device_properties(0).multi_processor_count + 1


def test_the_two_one_wave_builds_give_the_same_bits(monkeypatch):
    """The specialised and the generic one-wave build of the N = 15 two-term model on the same seeded inputs: equal bit
    for bit, NaNs included (the specialisation removes loads, dead rows and branches, never an operation that feeds an
    output)."""
    N, B = 15, 8
    dt, ic, _, _ = benes(N, 'tme', 1)
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=1815)
    model = _model(N, 1, B)
    with build_switches(monkeypatch):
        report_spec, (spec,) = run_plan_1d(model, N, T, B, m0=ic.cms, mean0=ic.mean, ys=ys)
    with build_switches(monkeypatch, MFS_FAST_BUILD='generic'):
        report_generic, (generic,) = run_plan_1d(model, N, T, B, m0=ic.cms, mean0=ic.mean, ys=ys)
    assert report_spec.build == ONE_WAVE_SPEC and report_generic.build == ONE_WAVE
    assert_same_bits(spec, generic)
    assert np.isfinite(spec.nell).all()       # two steps poison nothing: the comparison is of numbers
