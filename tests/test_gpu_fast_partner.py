"""The partner-wave variant of the fixed-traits one-wave builds of the fast 1-D kernel (csrc/filter1d_partner.hpp: 512-thread
workgroups, four main waves that run a step's critical path and four partner waves that form the posterior moments, decide the
poisoning and accumulate the likelihood) against the one-wave build it stands in for (MFS_FAST_PARTNER=0), through the plan
API of the C ABI.  The variant moves work between waves -- never a floating-point operation that feeds an output -- so every
comparison is equality of bits, NaN positions and first_nan included.

Shapes: N = 14, 15 (the orders with sixteen lanes per filter), T = 40.  B = 6 is a partial main wave and three pairs of waves
without filters, which must still meet every barrier; B = 17 is a second workgroup with one filter.  Models: the three
(model, transition) pairs with a fixed-traits build."""
import ctypes as C

import numpy as np
import pytest

from mfs_amd import _lib
from mfs_amd.one_dim import filtering
from tests.test_gpu_fast_straightline import MID_RUN, _bernoulli_ys, _unlike_replicates
from tests.test_gpu_fast_traits import COMBOS, ONE_WAVE, ONE_WAVE_SPEC, RUNTIME, _assert_identical, _model

pytestmark = pytest.mark.gpu

T = 40
FILTERS_PER_WORKGROUP = 16


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ('MFS_PREDICT_RULE', 'MFS_FAST_BUILD', 'MFS_FAST_TRAITS', 'MFS_FAST_PARTNER'):
        monkeypatch.delenv(name, raising=False)


def _run(combo, N, ys, m0, *, chunk=0, moments_out=True):
    """One central-mode plan run on (B, T) measurements and (B, 2N) start moments:
    ((moments, means, nell, first_nan), (build, traits, partner), (filters per block, grid))."""
    ic, tables, lik, _ = _model(combo, N)
    nb, nt = ys.shape
    L = _lib.lib()
    model, keep = filtering.build_model_struct(tables, lik, nb)
    plan = C.c_void_p()
    _lib.check(L.mfs_plan_1d_create(C.byref(plan), C.byref(model), 1, N, nt, nb, 0, chunk, 0))
    build, traits, partner = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(L.mfs_plan_1d_kernel_build(plan, C.byref(build)))
    _lib.check(L.mfs_plan_1d_kernel_traits(plan, C.byref(traits)))
    _lib.check(L.mfs_plan_1d_kernel_partner(plan, C.byref(partner)))
    fpb, grid = C.c_int(-1), C.c_int(-1)
    _lib.check(L.mfs_plan_1d_geometry(plan, None, C.byref(fpb), C.byref(grid), None))
    d_m0 = _lib.DeviceBuffer.from_array(np.ascontiguousarray(m0))
    d_mean0 = _lib.DeviceBuffer.from_array(np.full(nb, ic.mean))
    d_ys = _lib.DeviceBuffer.from_array(np.ascontiguousarray(ys))
    d_mom = _lib.DeviceBuffer(nb * nt * 2 * N * 8) if moments_out else None
    d_means, d_nell, d_fn = _lib.DeviceBuffer(nb * nt * 8), _lib.DeviceBuffer(nb * 8), _lib.DeviceBuffer(nb * 4)
    stream = C.c_void_p()
    _lib.check(L.mfs_stream_create(C.byref(stream)))
    _lib.check(L.mfs_plan_1d_run(plan, d_m0.ptr, 1, d_mean0.ptr, None, d_ys.ptr, d_mom.ptr if d_mom else None, d_means.ptr,
                                 None, d_nell.ptr, d_fn.ptr, stream))
    _lib.check(L.mfs_stream_synchronize(stream))
    out = (d_mom.to_array((nb, nt, 2 * N)) if d_mom else np.zeros(0), d_means.to_array((nb, nt)), d_nell.to_array((nb,)),
           d_fn.to_array((nb,), np.int32))
    _lib.check(L.mfs_plan_1d_destroy(plan))
    _lib.check(L.mfs_stream_destroy(stream))
    del keep
    return out, (build.value, traits.value, partner.value), (fpb.value, grid.value)


def _partner(combo, N, ys, m0, **kw):
    """The default plan: it must be the partner-wave variant, reported as the fixed-traits one-wave build."""
    out, which, (fpb, grid) = _run(combo, N, ys, m0, **kw)
    assert which == (ONE_WAVE_SPEC, COMBOS[combo], 1)
    assert (fpb, grid) == (FILTERS_PER_WORKGROUP, -(-ys.shape[0] // FILTERS_PER_WORKGROUP))
    return out


def _one_wave(monkeypatch, combo, N, ys, m0, **kw):
    monkeypatch.setenv('MFS_FAST_PARTNER', '0')
    out, which, (fpb, _) = _run(combo, N, ys, m0, **kw)
    monkeypatch.delenv('MFS_FAST_PARTNER')
    assert which == (ONE_WAVE_SPEC, COMBOS[combo], 0) and fpb == 4
    return out


def _inputs(combo, N, nb, nt=T, poison=True):
    """Bernoulli measurements (a Gaussian law accepts 0 / 1 as well) and the model's start moments; replicate 1 starts from a
    point mass, so it is poisoned at step 0 -- in the cold rule of the main wave -- next to live replicates."""
    from mfs_amd import synth
    from mfs_amd.one_dim import ss_models
    ys = synth.benes_bernoulli_batch(nb, nt, ss_models.benes_bernoulli(N)[0], seed=4100 + 16 * N + nb)[0]
    m0 = np.tile(_model(combo, N)[0].cms, (nb, 1))
    if poison and nb > 1:
        m0[1, 1:] = 0.
    return ys, m0


# ---- 1. builds agree
@pytest.mark.parametrize('B', [6, 17])
@pytest.mark.parametrize('N', [14, 15])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_builds_agree(combo, N, B, monkeypatch):
    ys, m0 = _inputs(combo, N, B)
    variant = _partner(combo, N, ys, m0)
    reference = _one_wave(monkeypatch, combo, N, ys, m0)
    _assert_identical(variant, reference)
    first_nan = variant[3]
    assert first_nan[1] == 0 and (np.delete(first_nan, 1) != 0).all()
    assert np.isfinite(variant[0][0]).all()
    if (combo, N, B) == ('benes_tme3', 15, 17):
        monkeypatch.setenv('MFS_FAST_BUILD', 'generic')
        generic, which, _ = _run(combo, N, ys, m0)
        assert which == (ONE_WAVE, RUNTIME, 0)
        _assert_identical(variant, generic)


# ---- 2. chunk carry: every launch starts from a carried state (the partner's opening elimination, its closing carry)
@pytest.mark.parametrize('chunk', [7, 1])
@pytest.mark.parametrize('N', [14, 15])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_chunk_carry(combo, N, chunk, monkeypatch):
    ys, m0 = _inputs(combo, N, 6)
    whole = _partner(combo, N, ys, m0)
    _assert_identical(_partner(combo, N, ys, m0, chunk=chunk), whole)
    _assert_identical(_one_wave(monkeypatch, combo, N, ys, m0, chunk=chunk), whole)


# ---- 3. NLL only
@pytest.mark.parametrize('N', [14, 15])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_nll_only(combo, N, monkeypatch):
    ys, m0 = _inputs(combo, N, 6)
    nll_only = _partner(combo, N, ys, m0, moments_out=False)
    _assert_identical(nll_only, _one_wave(monkeypatch, combo, N, ys, m0, moments_out=False))
    _assert_identical(nll_only[1:], _partner(combo, N, ys, m0)[1:])
    _assert_identical(_partner(combo, N, ys, m0, moments_out=False, chunk=7), nll_only)


# ---- 4. a replicate does not depend on its neighbours, its wave or its workgroup's other waves
@pytest.mark.parametrize('combo,N', [('ou_normal', 14), ('benes_tme_normal3', 14), ('benes_tme3', 15)])
def test_independence(combo, N, monkeypatch):
    ys, m0 = _unlike_replicates(combo, N, T)      # four unlike replicates; replicate 3 is poisoned at step 0
    first = _partner(combo, N, ys, m0)
    _assert_identical(first, _one_wave(monkeypatch, combo, N, ys, m0))
    assert first[3][3] == 0 and (first[3][:3] != 0).all()
    order = [3, 2, 0, 1]
    second = [x[np.argsort(order)] for x in _partner(combo, N, ys[order], m0[order])]
    _assert_identical(second, first)
    # the same four in wave 3 of the workgroup (slots 12..15), behind twelve copies of replicate 0 in waves 0..2
    pad = [0] * 12 + [0, 1, 2, 3]
    wave3 = [x[12:] for x in _partner(combo, N, ys[pad], m0[pad])]
    _assert_identical(wave3, first)
    for r in range(4):
        _assert_identical(_partner(combo, N, ys[r:r + 1], m0[r:r + 1]), [x[r:r + 1] for x in first])


# ---- 5. poisoning mid-run: the (N, T, seed) triples of test_gpu_fast_straightline.test_poisoning_mid_run, chosen with the CPU
# oracle so that replicates are poisoned at different steps next to live ones
@pytest.mark.parametrize('N', [14, 15])
def test_poisoning_mid_run(N, monkeypatch):
    nt, seed = MID_RUN[N]
    ys = _bernoulli_ys(N, nt, seed)
    m0 = np.tile(_model('benes_tme3', N)[0].cms, (ys.shape[0], 1))
    variant = _partner('benes_tme3', N, ys, m0)
    reference = _one_wave(monkeypatch, 'benes_tme3', N, ys, m0)
    first_nan = reference[3]
    assert ((first_nan > 0) & (first_nan < nt - 1)).any() and (first_nan < 0).any(), first_nan
    np.testing.assert_array_equal(variant[3], first_nan)      # neither a step early nor a step late
    for b in range(ys.shape[0]):
        if first_nan[b] >= 0:
            assert np.isfinite(variant[0][b, :first_nan[b]]).all() and np.isnan(variant[0][b, first_nan[b]:]).all()
            assert np.isfinite(variant[1][b, :first_nan[b]]).all() and np.isnan(variant[1][b, first_nan[b]:]).all()
    _assert_identical(variant, reference)
    _assert_identical(_partner('benes_tme3', N, ys, m0, chunk=16), variant)
    _assert_identical(_partner('benes_tme3', N, ys, m0, moments_out=False)[1:], variant[1:])


# ---- 6. the recompute rule on a plan created with the variant: the one-wave launcher, the same bits
@pytest.mark.parametrize('chunk', [0, 7])
@pytest.mark.parametrize('combo,N', [('benes_tme3', 15), ('ou_normal', 14)])
def test_recompute_rule(combo, N, chunk, monkeypatch):
    ys, m0 = _inputs(combo, N, 6)
    monkeypatch.setenv('MFS_PREDICT_RULE', 'recompute')
    variant = _partner(combo, N, ys, m0, chunk=chunk)
    _assert_identical(variant, _one_wave(monkeypatch, combo, N, ys, m0, chunk=chunk))



# ---- 7. the placement record: one for the library, and the kernels of every order reach it
def _placement():
    workgroups, mismatches = C.c_uint64(0), C.c_uint64(0)
    _lib.check(_lib.lib().mfs_partner_placement(C.byref(workgroups), C.byref(mismatches)))
    return workgroups.value, mismatches.value


@pytest.mark.parametrize('N', [14, 15])
def test_placement_record_counts_the_workgroups_of_each_order(N, monkeypatch):
    """Every workgroup of the variant adds itself to the record in its prologue, whichever translation unit its kernel comes
    from: B = 17 is two workgroups per launch, in one launch and in six (T = 40 in chunks of 7)."""
    ys, m0 = _inputs('benes_tme3', N, 17)
    before = _placement()
    _partner('benes_tme3', N, ys, m0)
    once = _placement()
    assert once[0] - before[0] == 2
    _partner('benes_tme3', N, ys, m0, chunk=7)
    chunked = _placement()
    assert chunked[0] - once[0] == 2 * 6
    assert 0 <= chunked[1] - before[1] <= chunked[0] - before[0]
    _one_wave(monkeypatch, 'benes_tme3', N, ys, m0)            # the one-wave build leaves the record alone
    assert _placement() == chunked
