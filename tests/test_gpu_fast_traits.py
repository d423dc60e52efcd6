"""The fixed-traits one-wave builds of the fast 1-D kernel (csrc/filter1d_fast.hpp, StepTraits: moment mode, u-map and
likelihood law compiled in, likelihood parameters in registers, output stores decided before the time loop) against the
same specialised build with run-time traits (MFS_FAST_TRAITS=runtime) and against the generic build
(MFS_FAST_BUILD=generic), through the plan API of the C ABI.  The traits remove branches, LDS reads and dead code -- never a
floating-point operation that feeds an output -- so every comparison here is equality of bits, NaNs included.

Shapes: N = 14, 15 (sixteen lanes per filter) and 16 (thirty-two); B = 6 leaves a partial last wave, so the `b >= B` exit is
live; T = 40 in one launch and in chunks of 16 (16 + 16 + 8) and of 24 (24 + 16: the plan takes one chunk length, so these two
stand for "16 + 24") -- both cross the 16-step measurement window and pass the posterior atoms through the carry."""
import functools

import numpy as np
import pytest

from mfs_amd import synth
from mfs_amd._lib import BUILD, TRAITS
from mfs_amd.one_dim import ss_models
from tests.plan_api import COMBOS, Outputs, assert_same_bits, build_switches, combo_model, run_plan_1d, three_builds

pytestmark = pytest.mark.gpu

FAST, ONE_WAVE, ONE_WAVE_SPEC = BUILD['fast'], BUILD['fast_one_wave'], BUILD['fast_one_wave_spec']
RUNTIME, TANH_BERNOULLI, IDENTITY_GAUSSIAN = (TRAITS[k] for k in ('runtime', 'central_tanh_bernoulli',
                                                                  'central_identity_gaussian'))
T, B = 40, 6
OTHERS = np.arange(B) != 1      # the replicates next to the poisoned one


@functools.lru_cache(maxsize=None)
def _ys(N):
    """One set of Bernoulli measurements per order, shared by every model (a Gaussian law accepts 0 / 1 as well)."""
    dt = ss_models.benes_bernoulli(N)[0]
    return synth.benes_bernoulli_batch(B, T, dt, seed=2600 + N)[0]


def _run(combo, N, *, mode='central', chunk=0, moments_out=True, poison=False):
    """One run of a plan under the switches in force, start state per replicate, scale0 and a scales buffer passed in every
    mode, means and scales zeroed first (raw mode writes no means, central mode no scales): (Outputs, build, traits)."""
    ic, tables, lik, _ = combo_model(combo, N, mode)
    m0 = np.tile({'raw': ic.rms, 'central': ic.cms, 'scaled': ic.scms}[mode], (B, 1))
    if poison:
        # replicate 1: a point mass (m_0 = 1, every other central moment 0): the second pivot of the first rule is 0, not > 0,
        # so this group is poisoned at step 0 while the groups next to it in the wave (replicates 0, 2, 3) stay alive
        m0[1, 1:] = 0.
    report, (out,) = run_plan_1d((tables, lik), N, T, B, mode=mode, chunk=chunk, m0=m0, mean0=ic.mean,
                                 scale0=np.sqrt(ic.variance), ys=_ys(N), zero_fill=True,
                                 outputs=Outputs._fields[0 if moments_out else 1:])
    return out, report.build, report.traits


def _plan_run(monkeypatch, combo, N, env=None, **kw):
    with build_switches(monkeypatch, **(env or {})):
        return _run(combo, N, **kw)


def _differs(x, y):
    return not np.array_equal(x, y, equal_nan=True)


def _check_three(monkeypatch, combo, N, env=None, **kw):
    """The same run on the fixed-traits build, the run-time-traits specialised build and the generic build."""
    (fixed, build_f, traits_f), (runtime, build_r, traits_r), (generic, build_g, traits_g) = \
        three_builds(monkeypatch, lambda: _run(combo, N, **kw), **(env or {}))
    assert (build_f, traits_f) == (ONE_WAVE_SPEC, COMBOS[combo])
    assert (build_r, traits_r) == (ONE_WAVE_SPEC, RUNTIME)
    assert (build_g, traits_g) == (ONE_WAVE, RUNTIME)
    assert_same_bits(fixed, runtime)
    assert_same_bits(fixed, generic)
    return fixed


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_fixed_traits_equal_runtime_traits_and_generic(combo, N, monkeypatch):
    """Moments, means, NLL and first_nan of the three builds, in one launch; the fixed-traits build chunked equals itself
    in one launch."""
    fixed = _check_three(monkeypatch, combo, N)
    assert np.isfinite(fixed.moments[:, 0]).all()                   # the first step of every replicate is a real number
    assert not fixed.scales.any()                                   # central mode: the scales buffer is left alone
    for chunk in (16, 24):
        chunked, build_c, traits_c = _plan_run(monkeypatch, combo, N, chunk=chunk)
        assert (build_c, traits_c) == (ONE_WAVE_SPEC, COMBOS[combo])
        assert_same_bits(chunked, fixed)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_nll_only_call(combo, N, monkeypatch):
    """out_moments = NULL: means, NLL and first_nan of the three builds agree, and are those of the call with moments."""
    nll_only = _check_three(monkeypatch, combo, N, moments_out=False)
    full, _, _ = _plan_run(monkeypatch, combo, N)
    assert nll_only.moments is None
    assert_same_bits(nll_only[1:], full[1:])
    chunked, _, _ = _plan_run(monkeypatch, combo, N, moments_out=False, chunk=16)
    assert_same_bits(chunked, nll_only)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_poisoned_group_next_to_live_groups(combo, N, monkeypatch):
    """A replicate whose start makes a pivot non-positive at the first step shares its wave with live replicates."""
    fixed = _check_three(monkeypatch, combo, N, poison=True)
    assert fixed.first_nan[1] == 0 and (fixed.first_nan[OTHERS] != 0).all()
    assert np.isnan(fixed.moments[1]).all() and np.isnan(fixed.nell[1])
    clean, _, _ = _plan_run(monkeypatch, combo, N)
    assert_same_bits(fixed.rows(OTHERS), clean.rows(OTHERS))
    chunked, _, _ = _plan_run(monkeypatch, combo, N, poison=True, chunk=16)
    assert_same_bits(chunked, fixed)


@pytest.mark.parametrize('N', [14, 15, 16])
@pytest.mark.parametrize('combo', sorted(COMBOS))
def test_recomputed_predict_rule(combo, N, monkeypatch):
    """MFS_PREDICT_RULE=recompute: the predict half runs the full rule in every build."""
    _check_three(monkeypatch, combo, N, env={'MFS_PREDICT_RULE': 'recompute'})


@pytest.mark.parametrize('mode', ['raw', 'scaled'])
def test_other_modes_keep_runtime_traits(mode, monkeypatch):
    """Raw and scaled plans have no fixed-traits build: they report run-time traits, run, and equal the generic build."""
    spec, build_s, traits_s = _plan_run(monkeypatch, 'benes_tme3', 15, mode=mode)
    assert (build_s, traits_s) == (ONE_WAVE_SPEC, RUNTIME)
    generic, build_g, traits_g = _plan_run(monkeypatch, 'benes_tme3', 15, {'MFS_FAST_BUILD': 'generic'}, mode=mode)
    assert (build_g, traits_g) == (ONE_WAVE, RUNTIME)
    assert_same_bits(spec, generic)
    assert spec.scales.any() == (mode == 'scaled') and spec.means.any() == (mode == 'scaled')


def test_order_without_a_one_wave_build_keeps_runtime_traits(monkeypatch):
    """N = 13 has no one-wave build, hence no traits build; neither switch changes what it runs."""
    a, build_a, traits_a = _plan_run(monkeypatch, 'benes_tme3', 13)
    b, build_b, traits_b = _plan_run(monkeypatch, 'benes_tme3', 13, {'MFS_FAST_BUILD': 'generic'})
    assert (build_a, traits_a) == (FAST, RUNTIME) and (build_b, traits_b) == (FAST, RUNTIME)
    assert_same_bits(a, b)


@pytest.mark.parametrize('N', [14, 15, 16])
def test_each_traits_build_computes_its_own_model(N, monkeypatch):
    """Would a wrong law or u-map be compiled in, or two registrations be swapped: the OU / Gaussian and the Benes /
    Bernoulli plans (both normal-closure tables, the same table shape) fed the same measurements differ from each other,
    and each equals its own run-time-traits result."""
    ou, _, traits_ou = _plan_run(monkeypatch, 'ou_normal', N)
    benes, _, traits_benes = _plan_run(monkeypatch, 'benes_tme_normal3', N)
    assert (traits_ou, traits_benes) == (IDENTITY_GAUSSIAN, TANH_BERNOULLI)
    assert _differs(ou.moments, benes.moments) and _differs(ou.nell, benes.nell)
    runtime = {'MFS_FAST_TRAITS': 'runtime'}
    ou_r, _, traits_ou_r = _plan_run(monkeypatch, 'ou_normal', N, runtime)
    benes_r, _, traits_benes_r = _plan_run(monkeypatch, 'benes_tme_normal3', N, runtime)
    assert (traits_ou_r, traits_benes_r) == (RUNTIME, RUNTIME)
    assert_same_bits(ou, ou_r)
    assert_same_bits(benes, benes_r)
