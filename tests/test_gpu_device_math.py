"""The shared device layer against exact arithmetic: every routine of csrc/device_util.hpp and every likelihood form of
csrc/likelihood.hpp, run on arrays by mfs_device_math (csrc/device_math_inst.hip), against the mpmath references, cases and
derived bounds of tests/device_math_ref.py (the derivations are in that module's docstring).  Each test is one or a few small
launches and prints its worst error / bound ratio before it asserts ratio <= 1; DESIGN.md section 4 records the table."""
import math

import numpy as np
import pytest

from mfs_amd import _lib
from tests import device_math_ref as R

pytestmark = pytest.mark.gpu


def _report(name, ratio):
    worst = float(np.max(ratio)) if len(ratio) else 0.
    print(f'[device-math] {name}: worst error / bound = {worst:.3f} over {len(ratio)} cases')
    return worst


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    """Bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- elementary functions
@pytest.mark.parametrize('fn', ['exp', 'exp_sc'])
def test_fast_exp_on_reduction_boundaries_and_thresholds(fn):
    """Both forms at the doubles around (k + 1/2) ln 2 and k ln 2 for every k in [-1076, 1025], log-uniform small arguments,
    the overflow / underflow / subnormal thresholds and the specials; the two forms agree bit for bit."""
    g = R.exp_cases()
    got = R.call(fn, [g.x])[0]
    for name, idx in g.sets.items():
        assert _report(f'{fn}/{name}', R.ratios(got[idx], [g.exact[i] for i in idx], [g.bound[i] for i in idx])) <= 1.
    x = g.x.tolist()
    assert got[x.index(710.)] == np.inf and got[x.index(-745.5)] == 0.
    assert got[g.sets['thresholds'][0]] == 1. and got[g.sets['thresholds'][1]] == 1.       # +-0
    assert _same_bits(got, R.call('exp_sc' if fn == 'exp' else 'exp', [g.x])[0])


@pytest.mark.parametrize('fn', ['exp', 'exp_sc'])
def test_fast_exp_within_the_rounding_of_its_own_operations(fn):
    """The sharper bound of device_math_ref.exp_sharp_bounds (about 2 u of the result where |r| is largest): 4e-16 leaves room for
    a missing Taylor term, this does not."""
    g = R.exp_cases()
    idx, bound = R.exp_sharp_bounds()
    got = R.call(fn, [g.x])[0]
    assert _report(f'{fn}/own-operations', R.ratios(got[idx], [g.exact[i] for i in idx], bound)) <= 1.


def test_fast_tanh_over_every_binade_the_clamp_and_specials():
    g = R.tanh_cases()
    got = R.call('tanh', [g.x])[0]
    for name, idx in g.sets.items():
        assert _report(f'tanh/{name}', R.ratios(got[idx], [g.exact[i] for i in idx], [g.bound[i] for i in idx])) <= 1.
    paired = np.concatenate([g.sets[k] for k in ('binades', 'dense', 'clamp', 'specials')])
    pos, neg = got[paired[0::2]], got[paired[1::2]]
    assert np.all(_bits(pos) == _bits(-neg)), 'tanh is not exactly odd'
    assert np.all(np.abs(got[paired]) <= 1.)
    inf_p, inf_n, zero_p, zero_n = got[g.sets['specials']]
    assert (inf_p, inf_n) == (1., -1.)
    assert zero_p == 0. and not np.signbit(zero_p) and zero_n == 0. and np.signbit(zero_n)


@pytest.mark.parametrize('fn', ['log', 'log_sc'])
def test_fast_log_over_every_binade_and_around_one(fn):
    g = R.log_cases()
    got = R.call(fn, [g.x])[0]
    print(f'[device-math] {fn}(1) = {got[g.sets["one"][0]]!r}, {fn}(1 + 2^-52) = {got[g.sets["one"][1]]!r}')
    for name in ('binades', 'near_one', 'one'):
        idx = g.sets[name]
        assert _report(f'{fn}/{name}', R.ratios(got[idx], [g.exact[i] for i in idx], [g.bound[i] for i in idx])) <= 1.
    zero_p, zero_n, inf, neg, neg_inf, nan = got[g.sets['specials']]
    assert zero_p == -np.inf and zero_n == -np.inf and inf == np.inf
    assert not np.isfinite(neg) and not np.isfinite(neg_inf) and np.isnan(nan)
    assert _same_bits(got, R.call('log_sc' if fn == 'log' else 'log', [g.x])[0])


@pytest.mark.parametrize('fn', ['rcp_nr', 'rcp_sat', 'rsq_nr'])
def test_newton_reciprocals_over_every_binade(fn):
    """2^-52 relative on normal results, one spacing on subnormal ones, non-finite where 1 / v overflows (the Newton step turns
    the hardware's inf into NaN); the specials as documented: rcp_nr(+-inf) NaN, rcp_sat(+-inf) +-0 like a true divide."""
    g = R.rcp_cases('rsq' if fn == 'rsq_nr' else 'rcp')
    got = R.call(fn, [g.x])[0]
    for name in ('normal', 'subnormal'):
        idx = g.sets[name]
        assert _report(f'{fn}/{name}', R.ratios(got[idx], [g.exact[i] for i in idx], [g.bound[i] for i in idx])) <= 1.
    assert not np.any(np.isfinite(got[g.sets['overflow']]))
    sp = R.call(fn, [np.array([np.inf, -np.inf, 0., -0., np.nan, -1.])])[0]
    if fn == 'rcp_nr':
        assert np.all(np.isnan(sp[:2]))
    elif fn == 'rcp_sat':
        assert sp[0] == 0. and not np.signbit(sp[0]) and sp[1] == 0. and np.signbit(sp[1])
    assert not np.any(np.isfinite(sp[2:5]))
    if fn == 'rsq_nr':
        assert not np.any(np.isfinite(sp[[0, 1, 5]]))


def test_log_factorial_and_the_table_of_likelihood_fast():
    """Every integer 0..200 (the 32-term sum, Stirling from 33), then 1e3, 1e6, 1e9, 2^53, against loggamma(y + 1); the LDS table
    of the fast 1-D kernels holds the same bits for y <= 32."""
    g = R.lfac_cases()
    got = R.call('log_factorial', [g.x])[0]
    y = g.x
    for name, idx in (('sum', np.flatnonzero(y <= 32)), ('stirling', np.flatnonzero(y > 32))):
        assert _report(f'log_factorial/{name}', R.ratios(got[idx], [g.exact[i] for i in idx], [g.bound[i] for i in idx])) <= 1.
    assert got[0] == 0. and got[1] == 0.
    table = R.call('lfac_table', [np.arange(R.LFAC_MAX + 1.)])[0]
    assert _same_bits(table, got[:R.LFAC_MAX + 1])
    assert np.all(np.isnan(R.call('lfac_table', [np.array([-1., R.LFAC_MAX + 1.])])[0]))


def test_likelihood_fast_reads_its_table_up_to_32_and_switches_at_33():
    """The table form and lik_density<false> are the same arithmetic but for where log(y!) comes from: the same bits at every count
    0..40, so a lookup off by one entry, or a switch at the wrong count, shows."""
    y = np.arange(41.)
    for eta in (-3., 0.5, 4., 30.):
        ref = R.call('lik_density', [R.POISSON, eta, 0., y])[0]
        assert np.all(ref > 0.)
        for fn in ('likelihood_fast', 'likelihood_fast_regs'):
            assert _same_bits(R.call(fn, [R.POISSON, 1., 0., 0., 0., y, eta])[0], ref), (fn, eta)


# ---- polynomials and the 2 x 2 Cholesky factor
def test_horner_against_exact_rationals():
    g = R.horner_cases()
    got = R.call('horner', list(g.x))[0]
    assert _report('horner', R.frac_ratios(got, g.exact, g.bound)) <= 1.


def test_gf_poly2_and_its_gradient_against_exact_rationals():
    g = R.poly2_cases()
    val = R.call('poly2', list(g.x))[0]
    assert _report('gf_poly2', R.frac_ratios(val, g.exact[0], [b[0] for b in g.bound[0]])) <= 1.
    grad = R.call('poly2_grad', list(g.x))
    for k, name in enumerate(('value', 'd0', 'd1')):
        assert _report(f'gf_poly2_grad/{name}', R.frac_ratios(grad[k], g.exact[k], [b[1] for b in g.bound[k]])) <= 1.
    assert sorted(set(g.x[0])) == list(range(1, R.EXTENT_HI + 1))


def test_gf_chol2_accuracy_and_pivot_rules():
    g = R.chol2_cases()
    got = R.call('chol2', list(g.x))
    for k, name in enumerate(('l00', 'l10', 'l11')):
        assert _report(f'gf_chol2/{name}', R.ratios(got[k], g.exact[k], g.bound[k])) <= 1.
    assert np.all(got[3] == 1.)
    P = np.array([p for p, _ in R.CHOL2_RULES]).T
    rules = R.call('chol2', list(P))
    assert rules[3].tolist() == [ok for _, ok in R.CHOL2_RULES]
    assert rules[:3, 0].tolist() == [2., 1., 0.] and rules[:3, 1].tolist() == [1., 0., 0.]      # the legal zero second pivots


# ---- likelihood forms
REGIMES = [(R.BERNOULLI, 'working'), (R.POISSON, 'working'), (R.GAUSSIAN, 'working'), (R.GAUSSIAN, 'subnormal')]


def _form_result(form, g):
    if form.startswith('lik_density'):
        return R.call(form, R.density_columns(g))[0], g.density_exact, g.density_bound
    return R.call(form, R.form_columns(g))[0], g.form_exact, g.form_bound


@pytest.mark.parametrize('kind,regime', REGIMES, ids=[f'{R.KIND_NAME[k]}-{r}' for k, r in REGIMES])
@pytest.mark.parametrize('form', R.FORMS)
def test_likelihood_form_in_its_working_range(form, kind, regime):
    g = R.working_cases(kind, regime)
    got, exact, bound = _form_result(form, g)
    assert _report(f'{form}/{R.KIND_NAME[kind]}/{regime}', R.ratios(got, exact, bound)) <= 1.


@pytest.mark.parametrize('kind,regime', REGIMES, ids=[f'{R.KIND_NAME[k]}-{r}' for k, r in REGIMES])
def test_likelihood_forms_agree_within_the_sum_of_their_bounds(kind, regime):
    """All six instantiations on the same cases (lik_density on the fp64 link value, one legitimate evaluation of the link, so
    the full form's bound covers it)."""
    g = R.working_cases(kind, regime)
    got = {form: _form_result(form, g)[0] for form in R.FORMS}
    bound = np.array([float(b) for b in g.form_bound])
    worst = 0.
    for i, a in enumerate(R.FORMS):
        for b in R.FORMS[i + 1:]:
            worst = max(worst, float(np.max(np.abs(got[a] - got[b]) / (2. * bound))))
    assert _report(f'agreement/{R.KIND_NAME[kind]}/{regime}', np.array([worst])) <= 1.
    # the same arithmetic in both members of a pair
    assert _same_bits(got['lik_density'], got['lik_density_sc'])
    assert _same_bits(got['likelihood_fast'], got['likelihood_fast_regs'])


def test_bearing_factor_of_likelihood_joint_nd():
    g = R.bearing_cases()
    got = R.call('likelihood_joint_nd', g.cols)[0]
    assert _report('likelihood_joint_nd/bearing', R.ratios(got, g.exact, g.bound)) <= 1.
    other = R.call('likelihood_joint_nd', [np.array([R.BERNOULLI, R.POISSON, R.GAUSSIAN, 7.]), 1., 0., 0., 0., 0., 1., 1.])[0]
    assert np.all(np.isnan(other))


@pytest.mark.parametrize('form', R.FORMS)
def test_bernoulli_edges(form):
    """z = +-{37, 40, 700, 745, 800, 1e308} and an overflowing x^3, y in {0, 1, 0.5, 2, NaN}: y > 0.5 reads as 1, everything else
    (NaN included) as 0; where the reference formula's fp64 value is 0 or 1 the device's is exactly that, elsewhere it is
    within the derived bound."""
    e = R.bernoulli_edges()
    if form.startswith('lik_density'):
        got = R.call(form, [R.BERNOULLI, e.z, 0., e.y])[0]
    else:
        got = R.call(form, [R.BERNOULLI, *e.lp.T, e.y, e.x])[0]
    sharp = (e.expected == 0.) | (e.expected == 1.)
    assert sharp.sum() >= 40
    assert np.array_equal(got[sharp], e.expected[sharp])
    rest = np.flatnonzero(~sharp)
    exact, bound = [], []
    for i in rest:
        v, r = R.bernoulli_exact([e.z[i], 0., 0., 0.], 1. if e.y[i] > 0.5 else 0., 0., 0)
        exact.append(v)
        bound.append(2 * (r * v + R._subnormal_floor(v)))
    assert _report(f'{form}/bernoulli/edges', R.ratios(got[rest], exact, bound)) <= 1.


@pytest.mark.parametrize('form', R.FORMS)
def test_poisson_edges(form):
    """Links in [-745, -30]: finite and in [0, 1], and exactly 1 (y = 0) or 0 (y >= 1) once the rate has underflowed to 0; links
    >= 710 (rate inf): 0 at y = 0 and NaN at y >= 1, as the reference's xlogy form gives."""
    e = R.poisson_edges()
    if form.startswith('lik_density'):
        got = R.call(form, [R.POISSON, e.eta, 0., e.y])[0]
    else:
        got = R.call(form, [R.POISSON, 1., 0., 0., 0., e.y, e.eta])[0]
    print(f'[device-math] {form}/poisson/edges:', dict(zip(zip(e.eta.tolist(), e.y.tolist()), got.tolist())))
    unit = e.want == -1.
    assert np.all(np.isfinite(got[unit]) & (got[unit] >= 0.) & (got[unit] <= 1.))
    assert _same_bits(got[~unit], e.want[~unit])
    assert (e.want == 1.).sum() >= 6 and (e.want == 0.).sum() >= 20 and np.isnan(e.want).sum() >= 8


@pytest.mark.parametrize('form', R.FORMS)
def test_nan_measurement_or_state_poisons_poisson_and_gaussian(form):
    nan = np.nan
    for kind in (R.POISSON, R.GAUSSIAN):
        if form.startswith('lik_density'):
            got = R.call(form, [kind, np.array([nan, 0.5, nan]), 1.5, np.array([1., nan, nan])])[0]
        else:
            got = R.call(form, [kind, 1., 0.25, 1.5, 0., np.array([1., nan, nan, 0.]), np.array([nan, 0.5, nan, nan])])[0]
        assert np.all(np.isnan(got)), (form, kind, got)


# ---- the entry itself
@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_probe_shapes_and_repeatability(n):
    """One element, and one below / at / above a block: every element is written, nothing else is, and two calls give the same
    bits."""
    rng = np.random.default_rng(n)
    for fn, cols in (('exp', [rng.uniform(-5., 5., n)]),
                     ('chol2', [rng.uniform(2., 3., n), rng.uniform(-1., 1., n), rng.uniform(2., 3., n)]),
                     ('poly2_grad', [3., *rng.uniform(-1., 1., (2 + R.EXTENT_HI ** 2, n))]),
                     ('likelihood_fast', [R.POISSON, 0.7, 0., 0., 0., np.floor(rng.uniform(0., 40., n)), rng.uniform(-3., 3., n)])):
        a, b = R.call(fn, cols), R.call(fn, cols)
        assert a.shape == (R.SHAPE[fn][1], n) and np.all(np.isfinite(a)) and not np.any(a == -7.25)
        assert _same_bits(a, b)
        if n > 1:                                    # element i does not depend on n
            head = R.call(fn, [np.asarray(c)[..., :1] if np.ndim(c) else c for c in cols])
            assert _same_bits(head[:, 0], a[:, 0])


def test_entry_error_codes():
    L = _lib.lib()
    x, out = np.zeros((60, 4)), np.zeros((4, 4))

    def rc(fn, n, n_in, i, n_out, o):
        return L.mfs_device_math(fn, n, n_in, _lib.ptr(i) if i is not None else None, n_out, _lib.ptr(o) if o is not None else None, 0)
    for args, word in (((-1, 4, 1, x, 1, out), 'fn'), ((len(R.FN), 4, 1, x, 1, out), 'fn'), ((0, 0, 1, x, 1, out), 'n = 0'),
                       ((0, -3, 1, x, 1, out), 'n = -3'), ((0, 4, 2, x, 1, out), 'n_in'), ((0, 4, 1, x, 2, out), 'n_out'),
                       ((R.FN['chol2'], 4, 3, x, 3, out), 'n_out'), ((0, 4, 1, None, 1, out), 'NULL'),
                       ((0, 4, 1, x, 1, None), 'NULL')):
        assert rc(*args) == -1, args[:3]
        assert word in L.mfs_last_error().decode(), (args[:3], L.mfs_last_error())
    assert np.all(out == 0.)
    for name, code in R.FN.items():                   # every code has a kernel, with the shape the reference module lists
        n_in, n_out = R.SHAPE[name]
        cols = np.full((n_in, 3), 1.)
        res = np.full((n_out, 3), -7.25)
        assert L.mfs_device_math(code, 3, n_in, _lib.ptr(cols), n_out, _lib.ptr(res), 0) == 0, name
        assert not np.any(res == -7.25), name
