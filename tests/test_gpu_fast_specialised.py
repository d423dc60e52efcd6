"""The specialised one-wave builds of the fast 1-D kernel (coefficient table in registers, live rows only, straight-line
halves: csrc/filter1d_fast.hpp, SPEC) against the generic build of the same kernel, through the plan API of the C ABI.
The specialisation removes loads, dead rows and branches -- never a floating-point operation that feeds an output -- so
every comparison here is equality, NaNs included.  MFS_FAST_BUILD=generic is the A/B switch (read at plan creation)."""
import ctypes as C

import pytest

from mfs_amd import _lib, synth
from mfs_amd._lib import BUILD
from tests.plan_api import assert_same_bits, benes, build_switches, run_plan_1d

pytestmark = pytest.mark.gpu

FAST, ONE_WAVE, ONE_WAVE_SPEC = BUILD['fast'], BUILD['fast_one_wave'], BUILD['fast_one_wave_spec']


def _plan_run(monkeypatch, N, T, B, chunk, ys, ic, tables, lik, **env):
    """One run of a plan under the switches `env`, start state shared by the batch: (Outputs, the build the plan picked)."""
    with build_switches(monkeypatch, **env):
        report, (out,) = run_plan_1d((tables, lik), N, T, B, chunk=chunk, m0=ic.cms, mean0=ic.mean, ys=ys)
    return out, report.build


def _both_builds(monkeypatch, *args, **env):
    default, build_default = _plan_run(monkeypatch, *args, **env)
    generic, build_generic = _plan_run(monkeypatch, *args, MFS_FAST_BUILD='generic', **env)
    return default, build_default, generic, build_generic


@pytest.mark.parametrize('family,order', [('tme', 3), ('tme', 2), ('tme', 1), ('tme_normal', 3)])
def test_specialised_build_equals_generic_build(family, order, monkeypatch):
    """Headline shape in small: N = 15, sixteen lanes per filter, at most one wave per SIMD.  TME-3 is the headline's table
    (6 operator terms + variance); TME-2 / TME-1 / TME-normal-3 are the other specialised shapes.  300 steps poison a good
    part of the replicates at N = 15, and those must stop at the same step with the same numbers before it."""
    N, T, B = 15, 300, 48
    dt, ic, tables, lik = benes(N, family, order)
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=1500 + order)
    spec, build_spec, generic, build_generic = _both_builds(monkeypatch, N, T, B, 0, ys, ic, tables, lik)
    assert build_spec == ONE_WAVE_SPEC and build_generic == ONE_WAVE
    assert_same_bits(spec, generic)
    if family == 'tme' and order == 3:
        # the case really has poisoned and surviving replicates
        assert (spec.first_nan >= 0).any() and (spec.first_nan < 0).any()
    # chunked (the atoms travel in the carry) and with the reference's literal predict-half rule
    chunked, build_chunked = _plan_run(monkeypatch, N, T, B, 70, ys, ic, tables, lik)
    assert build_chunked == ONE_WAVE_SPEC
    assert_same_bits(chunked, spec)
    spec_r, build_spec_r, generic_r, build_generic_r = _both_builds(monkeypatch, N, T, B, 0, ys, ic, tables, lik,
                                                                    MFS_PREDICT_RULE='recompute')
    assert build_spec_r == ONE_WAVE_SPEC and build_generic_r == ONE_WAVE
    assert_same_bits(spec_r, generic_r)


@pytest.mark.parametrize('N', [14, 16])
def test_other_orders_with_a_one_wave_build(N, monkeypatch):
    """N = 14 (sixteen lanes) and N = 16 (thirty-two lanes) are the other two orders that have one-wave builds."""
    T, B = 120, 24
    dt, ic, tables, lik = benes(N, 'tme', 3)
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=1600 + N)
    spec, build_spec, generic, build_generic = _both_builds(monkeypatch, N, T, B, 0, ys, ic, tables, lik)
    assert build_spec == ONE_WAVE_SPEC and build_generic == ONE_WAVE
    assert_same_bits(spec, generic)


def test_shapes_and_batches_outside_the_specialised_set_run_the_generic_builds(monkeypatch):
    """TME-4 (8 operator terms) has no specialised build; a batch of more than one wave per SIMD runs the two-wave build;
    N = 13 has no one-wave build at all.  All still run, pick what they picked before, and do not react to the switch."""
    N, T = 15, 60
    dt, ic, tables, lik = benes(N, 'tme', 4)
    ys, _ = synth.benes_bernoulli_batch(32, T, dt, seed=1700)
    a, build_a, b, build_b = _both_builds(monkeypatch, N, T, 32, 0, ys, ic, tables, lik)
    assert build_a == ONE_WAVE and build_b == ONE_WAVE
    assert_same_bits(a, b)

    # more than one wave per SIMD: the grid exceeds 4 waves per compute unit
    L = _lib.lib()
    props = C.create_string_buffer(256)
    _lib.check(L.mfs_device_name(0, props, 256))
    cus = int(props.value.decode().rsplit(',', 1)[1].split()[0])     # "... (arch, <n> CUs)"
    B_big = 4 * (4 * cus + 8)                                   # four filters per wave at sixteen lanes per filter
    dt, ic, tables, lik = benes(N, 'tme', 3)
    T_big = 24
    ys_big, _ = synth.benes_bernoulli_batch(B_big, T_big, dt, seed=1701)
    big, build_big, big_g, build_big_g = _both_builds(monkeypatch, N, T_big, B_big, 0, ys_big, ic, tables, lik)
    assert build_big == FAST and build_big_g == FAST
    assert_same_bits(big, big_g)

    dt, ic, tables, lik = benes(13, 'tme', 3)
    ys13, _ = synth.benes_bernoulli_batch(16, T, dt, seed=1702)
    c, build_c, d, build_d = _both_builds(monkeypatch, 13, T, 16, 0, ys13, ic, tables, lik)
    assert build_c == FAST and build_d == FAST
    assert_same_bits(c, d)
