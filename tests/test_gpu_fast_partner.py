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
from mfs_amd._lib import BUILD, TRAITS
from tests.plan_api import (COMBOS, MID_RUN, MID_RUN_B, assert_same_bits, bernoulli_ys, build_switches, combo_model,
                            one_wave_build as _one_wave, partner_inputs, partner_variant as _partner, run_central,
                            unlike_replicates)

pytestmark = pytest.mark.gpu

T = 40
RECOMPUTE = {'MFS_PREDICT_RULE': 'recompute'}


def _inputs(combo, N, nb):
    return partner_inputs(combo, N, nb, T)


# ---- 1. builds agree
@pytest.mark.parametrize('B', [6, 17])
@pytest.mark.parametrize('N', [14, 15])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_builds_agree(combo, N, B, monkeypatch):
    ys, m0 = _inputs(combo, N, B)
    variant = _partner(monkeypatch, combo, N, ys, m0)
    reference = _one_wave(monkeypatch, combo, N, ys, m0)
    assert_same_bits(variant, reference)
    first_nan = variant.first_nan
    assert first_nan[1] == 0 and (np.delete(first_nan, 1) != 0).all()
    assert np.isfinite(variant.moments[0]).all()
    if (combo, N, B) == ('benes_tme3', 15, 17):
        with build_switches(monkeypatch, MFS_FAST_BUILD='generic'):
            report, generic = run_central(combo, N, ys, m0)
        assert report[:3] == (BUILD['fast_one_wave'], TRAITS['runtime'], 0)
        assert_same_bits(variant, generic)


# ---- 2. chunk carry: every launch starts from a carried state (the partner's opening elimination, its closing carry)
@pytest.mark.parametrize('chunk', [7, 1])
@pytest.mark.parametrize('N', [14, 15])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_chunk_carry(combo, N, chunk, monkeypatch):
    ys, m0 = _inputs(combo, N, 6)
    whole = _partner(monkeypatch, combo, N, ys, m0)
    assert_same_bits(_partner(monkeypatch, combo, N, ys, m0, chunk=chunk), whole)
    assert_same_bits(_one_wave(monkeypatch, combo, N, ys, m0, chunk=chunk), whole)


# ---- 3. NLL only
@pytest.mark.parametrize('N', [14, 15])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_nll_only(combo, N, monkeypatch):
    ys, m0 = _inputs(combo, N, 6)
    nll_only = _partner(monkeypatch, combo, N, ys, m0, moments_out=False)
    assert_same_bits(nll_only, _one_wave(monkeypatch, combo, N, ys, m0, moments_out=False))
    assert_same_bits(nll_only[1:], _partner(monkeypatch, combo, N, ys, m0)[1:])
    assert_same_bits(_partner(monkeypatch, combo, N, ys, m0, moments_out=False, chunk=7), nll_only)


# ---- 4. a replicate does not depend on its neighbours, its wave or its workgroup's other waves
@pytest.mark.parametrize('combo,N', [('ou_normal', 14), ('benes_tme_normal3', 14), ('benes_tme3', 15)])
def test_independence(combo, N, monkeypatch):
    ys, m0 = unlike_replicates(combo, N, T)      # four unlike replicates; replicate 3 is poisoned at step 0
    first = _partner(monkeypatch, combo, N, ys, m0)
    assert_same_bits(first, _one_wave(monkeypatch, combo, N, ys, m0))
    assert first.first_nan[3] == 0 and (first.first_nan[:3] != 0).all()
    order = [3, 2, 0, 1]
    second = _partner(monkeypatch, combo, N, ys[order], m0[order]).rows(np.argsort(order))
    assert_same_bits(second, first)
    # the same four in wave 3 of the workgroup (slots 12..15), behind twelve copies of replicate 0 in waves 0..2
    pad = [0] * 12 + [0, 1, 2, 3]
    wave3 = _partner(monkeypatch, combo, N, ys[pad], m0[pad]).rows(slice(12, None))
    assert_same_bits(wave3, first)
    for r in range(4):
        assert_same_bits(_partner(monkeypatch, combo, N, ys[r:r + 1], m0[r:r + 1]), first.rows(slice(r, r + 1)))


# ---- 5. poisoning mid-run: the (N, T, seed) triples of test_gpu_fast_straightline.test_poisoning_mid_run, chosen with the CPU
# oracle so that replicates are poisoned at different steps next to live ones
@pytest.mark.parametrize('N', [14, 15])
def test_poisoning_mid_run(N, monkeypatch):
    nt, seed = MID_RUN[N]
    ys = bernoulli_ys(N, nt, seed, MID_RUN_B)
    m0 = np.tile(combo_model('benes_tme3', N)[0].cms, (ys.shape[0], 1))
    variant = _partner(monkeypatch, 'benes_tme3', N, ys, m0)
    reference = _one_wave(monkeypatch, 'benes_tme3', N, ys, m0)
    first_nan = reference.first_nan
    assert ((first_nan > 0) & (first_nan < nt - 1)).any() and (first_nan < 0).any(), first_nan
    np.testing.assert_array_equal(variant.first_nan, first_nan)      # neither a step early nor a step late
    for b in range(ys.shape[0]):
        if first_nan[b] >= 0:
            assert np.isfinite(variant.moments[b, :first_nan[b]]).all() and np.isnan(variant.moments[b, first_nan[b]:]).all()
            assert np.isfinite(variant.means[b, :first_nan[b]]).all() and np.isnan(variant.means[b, first_nan[b]:]).all()
    assert_same_bits(variant, reference)
    assert_same_bits(_partner(monkeypatch, 'benes_tme3', N, ys, m0, chunk=16), variant)
    assert_same_bits(_partner(monkeypatch, 'benes_tme3', N, ys, m0, moments_out=False)[1:], variant[1:])


# ---- 6. the recompute rule on a plan created with the variant: the one-wave launcher, the same bits
@pytest.mark.parametrize('chunk', [0, 7])
@pytest.mark.parametrize('combo,N', [('benes_tme3', 15), ('ou_normal', 14)])
def test_recompute_rule(combo, N, chunk, monkeypatch):
    ys, m0 = _inputs(combo, N, 6)
    variant = _partner(monkeypatch, combo, N, ys, m0, chunk=chunk, env=RECOMPUTE)
    assert_same_bits(variant, _one_wave(monkeypatch, combo, N, ys, m0, chunk=chunk, env=RECOMPUTE))


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
    _partner(monkeypatch, 'benes_tme3', N, ys, m0)
    once = _placement()
    assert once[0] - before[0] == 2
    _partner(monkeypatch, 'benes_tme3', N, ys, m0, chunk=7)
    chunked = _placement()
    assert chunked[0] - once[0] == 2 * 6
    assert 0 <= chunked[1] - before[1] <= chunked[0] - before[0]
    _one_wave(monkeypatch, 'benes_tme3', N, ys, m0)            # the one-wave build leaves the record alone
    assert _placement() == chunked
