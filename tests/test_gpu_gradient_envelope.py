"""The NLL gradient kernel (C entry mfs_filter_1d_grad, mfs_amd/csrc/filter1d_grad.hpp) over everything it ships: all 60
instantiations N = 2..16 x P = 1..4, both table kinds, both u-maps, the three likelihoods, the three moment modes, the
batching flags, the launch geometry, poisoned replicates and the entry point's error codes.

Reference for the derivative: Richardson-combined central differences of the CPU C port along random directions in table
space (tests/gradient_ref.py) -- every non-zero entry of every table row moves on its own, so a tangent dropped for one row
shows.  tests/test_host_gradient_ref.py proves without a GPU that this reference is good to 1e-7 of max_p |g_ref| for every
case run here; the device is held to 2e-6 of max_p |g_ref| per replicate, the NLL to rtol 1e-9 (N <= 8) / 1e-8 (N >= 9)
against the C port AND against the plain filter kernel on the same model struct."""
import ctypes as C
import dataclasses

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib
from tests import gradient_ref as G
from tests.plan_api import assert_same_bits

pytestmark = pytest.mark.gpu

MFS_EINVAL, MFS_EUNSUPPORTED = -1, -2


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same_bits(got, want, what):
    assert_same_bits(got, want, what, names=('nell', 'grad', 'first_nan'))


def _check_against_reference(case, outputs=None):
    """The assertions every case shares -> the worst |g - g_ref| / max_p |g_ref| over the replicates."""
    nell, grad, fn = G.device_grad(case) if outputs is None else outputs
    ref_nell, ref_grad = G.reference(case)
    plain_nell, plain_fn = G.device_plain(case)
    ratio = (np.abs(grad - ref_grad).max(axis=-1) / np.abs(ref_grad).max(axis=-1)).max()
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))      # noqa: E731
    print(f'{case.id}: gradient {ratio:.2e} of max|g_ref| (bound {G.GRAD_BOUND:.0e}); nell vs C port {rel(nell, ref_nell):.1e}, '
          f'vs plain kernel {rel(nell, plain_nell):.1e} (bound {G.nell_rtol(case.N):.0e})')
    # the contract of include/mfs_hip.h: no poisoning reported <=> finite NLL and finite gradient
    assert np.all(fn == -1) and np.all(plain_fn == -1), f'{case.id}: first_nan {fn} (plain kernel {plain_fn})'
    assert np.all(np.isfinite(nell)) and np.all(np.isfinite(grad)), f'{case.id}: {nell} {grad}'
    npt.assert_allclose(nell, ref_nell, rtol=G.nell_rtol(case.N), err_msg=case.id)
    npt.assert_allclose(nell, plain_nell, rtol=G.nell_rtol(case.N), err_msg=case.id)
    assert ratio <= G.GRAD_BOUND, f'{case.id}: |g - g_ref| = {ratio:.2e} max|g_ref|\n{grad}\n{ref_grad}'
    return ratio


# ---- 1: every instantiation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', range(2, 17))
def test_every_instantiation(N):
    """Model A (Benes, TME-3 operator tables in tanh x, Bernoulli-logistic), central mode, P = 1..4 at this N, B = 3."""
    cases = [c for c in G.EVERY_INSTANTIATION if c.N == N]
    assert [c.P for c in cases] == [1, 2, 3, 4]
    worst = max(_check_against_reference(c) for c in cases)
    print(f'N = {N}: worst gradient ratio {worst:.2e} of max|g_ref|, bound {G.GRAD_BOUND:.0e}')


# ---- 2: model x mode matrix -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.MATRIX, ids=lambda c: c.id)
def test_model_mode_matrix(case):
    _check_against_reference(case)


@pytest.mark.parametrize('case', G.POISON_AT_START, ids=lambda c: c.id)
def test_orders_without_a_rule_poison_in_the_first_step(case):
    """Model E at N = 15, 16 (gradient_ref._no_rule): NaN from step 0 on, on both kernels, as in the C port."""
    nell, grad, fn = G.device_grad(case)
    plain_nell, plain_fn = G.device_plain(case)
    assert np.all(fn == 0) and np.all(plain_fn == 0)
    assert np.all(np.isnan(nell)) and np.all(np.isnan(grad)) and np.all(np.isnan(plain_nell))


# ---- 3: batching flags ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.BATCHING, ids=lambda c: c.id)
def test_batching_flags(case):
    """Each replicate has its own base tables (scaled by 1 + 0.02 b) where the flag is on, and its own reference; the
    dcoef / dlik layouts are the header's ([B][P][...] when batched, [P][...] otherwise)."""
    x = G.inputs(case)
    if case.coef_batched:
        assert not np.array_equal(x.coef[0], x.coef[1]) and not np.array_equal(x.dcoef[0], x.dcoef[1])
    if case.lik_batched:
        assert not np.array_equal(x.lp[0], x.lp[1]) and not np.array_equal(x.dlik[0], x.dlik[1])
    if case.m0_batched:
        assert not np.array_equal(x.mean0[0], x.mean0[1]) and not np.array_equal(x.scale0[0], x.scale0[1])
    _check_against_reference(case)


# ---- 4: geometry and bit equality -------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.GEOMETRY, ids=lambda c: c.id)
def test_geometry_and_bit_equality(case):
    """Replicate b returns the same bits alone, in every batch (waves partly empty, exactly full, one filter over, several
    blocks), on a second run, and with the shared tables passed as batched ones: every sum in the kernel is a group shuffle
    or a fixed-order LDS loop, `warm` is per-lane state, and there are no atomics."""
    x = G.inputs(case)
    fpw = G.filters_per_wave(case.N)
    batches = G.geometry_batches(case.N)
    assert batches == (1, fpw - 1, fpw, fpw + 1, 2 * fpw + 3) and case.B == batches[-1]
    full = G.device_grad(case)
    _check_against_reference(case, full)
    _assert_same_bits(G.device_grad(case), full, 'second run')
    for nb in batches[:-1]:
        _assert_same_bits(G.device_grad(case, rows=np.arange(nb)), [o[:nb] for o in full], f'batch of {nb}')
    for b in range(case.B):
        _assert_same_bits(G.device_grad(case, rows=[b]), [o[b:b + 1] for o in full], f'replicate {b} alone')
    _assert_same_bits(G.device_grad(case, coef_batched=True, lik_batched=True, m0_batched=True), full, 'tables as batched')
    # a batch in another order: the replicate's place in the wave does not matter either
    perm = np.arange(case.B)[::-1]
    _assert_same_bits(G.device_grad(case, rows=perm), [o[perm] for o in full], 'reversed batch')


# ---- 5: poisoning -----------------------------------------------------------------------------------------------------
def _poison_check(case, x_clean, x_bad, victim, step):
    clean = G.device_grad(case, x_clean)
    assert np.all(clean[2] == -1) and np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[1]))
    nell, grad, fn = G.device_grad(case, x_bad)
    others = np.arange(case.B) != victim
    assert fn[victim] == step, fn
    assert np.isnan(nell[victim]) and np.all(np.isnan(grad[victim])), (nell, grad)
    _assert_same_bits([o[others] for o in (nell, grad, fn)], [o[others] for o in clean], 'neighbours of the poisoned replicate')
    return clean


def test_poisoned_start_vector_stays_in_its_replicate():
    """A start vector whose second central moment is negative, in replicate 2 of 5 (model A, N = 9): the Cholesky pivot of
    the first rule is not > 0."""
    case = G.Case('poison', 'A', 'central', 9, 2, 5, m0_batched=True, seed=13)
    x = G.inputs(case)
    m0 = x.m0.copy()
    m0[2, 2] = -m0[2, 2]
    _poison_check(case, x, dataclasses.replace(x, m0=m0), victim=2, step=0)


@pytest.mark.parametrize('N', [8, 9])
def test_likelihood_underflow_poisons_at_its_step(N):
    """Model D (Gaussian likelihood) with a measurement of 1e200 at step 11 of replicate 1: p_y underflows to 0 there, so the
    first failure is a non-finite quantity (nell = inf), not a pivot.  Both kernels report step 11."""
    case = G.Case('poison', 'D', 'scaled', N, 2, 3, T=16, seed=0)
    x = G.inputs(case)
    ys = x.ys.copy()
    ys[1, 11] = 1e200
    x_bad = dataclasses.replace(x, ys=ys)
    _poison_check(case, x, x_bad, victim=1, step=11)
    plain_nell, plain_fn = G.device_plain(case, x_bad)
    clean_nell, clean_fn = G.device_plain(case, x)
    assert list(plain_fn) == [-1, 11, -1] and list(clean_fn) == [-1, -1, -1]
    assert np.isnan(plain_nell[1])
    assert np.array_equal(_bits(plain_nell[[0, 2]]), _bits(clean_nell[[0, 2]]))


# ---- 6: long runs on the warm-start path ------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.LONG, ids=lambda c: c.id)
def test_long_runs_on_the_warm_start_path(case):
    """T = 300 (model A at N = 16: 75, the longest of 300, 150, 75 at which the reference meets its condition): after the
    first step every root starts from the one a step ago, and an error of the root search would accumulate."""
    _check_against_reference(case)


# ---- 7: error codes ---------------------------------------------------------------------------------------------------
def _entry_call(**over):
    """One call of the entry point on model A, N = 5, P = 2, B = 3 with arguments replaced by `over`.  Every buffer is large
    enough for every N and n_par passed here, so nothing is read out of bounds even if a check were missing."""
    case = G.Case('errors', 'A', 'central', 5, 2, 3)
    x = G.inputs(case)
    m, keep = G._model_struct(case, x.coef, x.lp, False, False)
    B, T = x.ys.shape
    dcoef = np.zeros((5,) + x.dcoef.shape[2:])
    dcoef[:2] = x.dcoef[0]
    dlik = np.zeros((5,) + x.dlik.shape[2:])
    dlik[:2] = x.dlik[0]
    m0 = np.zeros(64)
    m0[:2 * case.N] = x.m0[0]
    a = dict(dcoef=dcoef, dlik=dlik, n_par=2, mode=_lib.MODE['central'], N=case.N, T=T, B=B, m0=m0,
             mean0=np.ascontiguousarray(x.mean0[:1]), ys=np.ascontiguousarray(x.ys), nell=np.full((B,), -7.),
             grad=np.full((B, 5), -7.), fn=np.full((B,), -7, dtype=np.int32))
    a.update(over)
    rc = _lib.lib().mfs_filter_1d_grad(C.byref(m), _lib.ptr(a['dcoef']), _lib.ptr(a['dlik']), a['n_par'], a['mode'], a['N'],
                                       a['T'], a['B'], _lib.ptr(a['m0']), 0, _lib.ptr(a['mean0']), None, _lib.ptr(a['ys']),
                                       _lib.ptr(a['nell']), _lib.ptr(a['grad']), _lib.ptr(a['fn']), 0, None)
    del keep
    return rc, a


def _override_id(over):
    return ','.join(f'{k}={"NULL" if v is None else v}' for k, v in over.items())


@pytest.mark.parametrize('over, code', [
    (dict(N=1), MFS_EUNSUPPORTED), (dict(N=17), MFS_EUNSUPPORTED), (dict(n_par=0), MFS_EUNSUPPORTED),
    (dict(n_par=5), MFS_EUNSUPPORTED), (dict(mode=_lib.MODE['central'] | _lib.MODE_ODD_TAIL), MFS_EUNSUPPORTED),
    (dict(dcoef=None), MFS_EINVAL), (dict(dlik=None), MFS_EINVAL), (dict(grad=None), MFS_EINVAL),
    (dict(T=-1), MFS_EINVAL), (dict(B=-1), MFS_EINVAL)], ids=lambda v: _override_id(v) if isinstance(v, dict) else str(v))
def test_error_codes(over, code):
    rc, a = _entry_call(**over)
    assert rc == code
    assert _lib.lib().mfs_last_error().decode() != ''
    for out in ('nell', 'grad', 'fn'):       # a refused call writes nothing
        assert a[out] is None or np.all(a[out] == -7)


def test_empty_batch_and_optional_first_nan():
    rc, a = _entry_call(B=0)
    assert rc == _lib.MFS_OK
    assert np.all(a['nell'] == -7) and np.all(a['grad'] == -7) and np.all(a['fn'] == -7)
    rc, full = _entry_call()
    assert rc == _lib.MFS_OK and np.all(full['fn'] == -1)
    rc, a = _entry_call(fn=None)             # out_first_nan = NULL is accepted
    assert rc == _lib.MFS_OK
    assert np.array_equal(_bits(a['nell']), _bits(full['nell']))
    written = lambda r: r['grad'].ravel()[:3 * 2]      # noqa: E731  (out_grad is [B][n_par] with n_par = 2)
    assert np.array_equal(_bits(written(a)), _bits(written(full))) and np.all(full['grad'].ravel()[3 * 2:] == -7)
    assert np.all(np.isfinite(full['nell'])) and np.all(np.isfinite(written(full)))
