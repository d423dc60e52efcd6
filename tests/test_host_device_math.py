"""The reference side of tests/test_gpu_device_math.py (tests/device_math_ref.py), without a GPU: the mpmath evaluation agrees
with SciPy / NumPy at benign inputs, the case sets hold what they claim (every k, every binade, every count, every branch),
every working-range case meets the bound cap, and the edge tables expect what the reference's own formulas
(mfs_amd.stats) give."""
import math

import mpmath as mp
import numpy as np
import scipy.special
import scipy.stats

from mfs_amd import stats
from tests import device_math_ref as R


def _ulps(exact, ref):
    """|ref - exact| in spacings of the exact value, per element."""
    return np.array([float(abs(mp.mpf(float(r)) - e) / R.spacing(e)) for e, r in zip(exact, ref)])


def test_spacing_and_ratio_measure():
    assert R.spacing(mp.mpf(1)) == mp.mpf(2) ** -52 and R.spacing(mp.mpf(2) - mp.mpf(2) ** -60) == mp.mpf(2) ** -52
    assert R.spacing(mp.mpf(2) ** -1022) == R.TINY and R.spacing(mp.mpf(2) ** -1030) == R.TINY
    assert R.spacing(R.DBL_MAX) == R.SP_TOP
    e = [mp.mpf(1), mp.mpf(1), R.NAN, R.NAN, mp.inf, mp.inf, R.DBL_MAX, mp.mpf(1e300), mp.mpf(2) ** -1076]
    g = [1. + 2. ** -52, np.nan, np.nan, 1., np.inf, 1e308, np.inf, np.inf, 0.]
    b = [mp.mpf(2) ** -52] * 8 + [R.TINY]
    assert R.ratios(g, e, b).tolist() == [1., np.inf, 0., np.inf, 0., np.inf, 0., np.inf, 0.25]


def test_mpmath_reference_agrees_with_numpy_and_scipy_at_benign_inputs():
    rng = np.random.default_rng(7)
    g = R.exp_cases()
    idx = [i for i in g.sets['half'][::40] + g.sets['small'][::10] if abs(g.x[i]) < 700]
    assert _ulps([g.exact[i] for i in idx], np.exp(g.x[idx])).max() <= 4
    g = R.log_cases()
    idx = g.sets['binades'][::40]
    assert _ulps([g.exact[i] for i in idx], np.log(g.x[idx])).max() <= 4
    g = R.tanh_cases()
    idx = g.sets['dense'][::10]
    assert _ulps([g.exact[i] for i in idx], np.tanh(g.x[idx])).max() <= 4
    g = R.lfac_cases()
    idx = [i for i in range(len(g.x)) if g.x[i] >= 2]
    assert _ulps([g.exact[i] for i in idx], scipy.special.gammaln(g.x[idx] + 1.)).max() <= 4
    g = R.rcp_cases('rcp')
    idx = g.sets['normal'][::50]
    assert _ulps([g.exact[i] for i in idx], 1. / g.x[idx]).max() <= 0.5
    # the likelihood formulas, at a handful of benign points of each kind
    for _ in range(20):
        lp, x = rng.uniform(-1., 1., 4), rng.uniform(-1.5, 1.5)
        p = 1. / (1. + math.exp(-R.link_fp64(R.BERNOULLI, lp, x)))
        for y in (0., 1.):
            assert _ulps([R.form_exact(R.BERNOULLI, lp, y, x)[0]], [scipy.stats.bernoulli.pmf(y, p)]).max() <= 4
        eta, y = rng.uniform(0., 3.), float(rng.integers(0, 8))
        ref = scipy.stats.poisson.pmf(y, math.log1p(math.exp(eta)))
        assert abs(float(R.density_exact(R.POISSON, eta, 0., y)[0]) / ref - 1.) <= 40 * R.U      # pmf through exp(log): |t| ulps
        m, sd, yy = rng.uniform(-1., 1.), rng.uniform(0.5, 2.), rng.uniform(-2., 2.)
        assert _ulps([R.density_exact(R.GAUSSIAN, m, sd * sd, yy)[0]], [scipy.stats.norm.pdf(yy, m, sd)]).max() <= 4


def test_elementary_case_sets_hold_every_k_and_every_binade():
    ln2 = math.log(2.)
    g = R.exp_cases()
    for name, shift in (('half', 0.5), ('flip', 0.)):
        x = g.x[g.sets[name]].reshape(len(R.EXP_KS), 5)
        assert len(R.EXP_KS) == 2102 and np.all(np.abs(x / ln2 - (np.array(R.EXP_KS)[:, None] + shift)) < 1e-9)
        assert np.all(np.ptp(x, axis=1) > 0)
    assert len(g.sets['small']) == 4000 and np.abs(g.x[g.sets['small']]).min() < 1e-300
    t = g.x[g.sets['thresholds']]
    for lo, hi, c in ((t[2], t[3], -1075 * mp.ln(2)), (t[4], t[5], -1022 * mp.ln(2)), (t[6], t[7], mp.log(R.DBL_MAX))):
        assert mp.mpf(lo) < c < mp.mpf(hi) and float(np.nextafter(lo, np.inf)) == hi
    idx, sharp = R.exp_sharp_bounds()
    rel = [float(b / g.exact[i]) / R.U for i, b in zip(idx, sharp) if R.MIN_NORMAL < g.exact[i] < R.DBL_MAX]
    assert len(idx) == 25020 and min(rel) >= 1. and max(rel) <= 2.25 and max(rel) * R.U < R.E_EXP     # sharper than 4e-16 everywhere
    g = R.tanh_cases()
    e = np.frexp(g.x[g.sets['binades']][0::4])[1] - 1
    assert e.tolist() == list(R.TANH_ES) and len(g.sets['clamp']) == 10
    g = R.log_cases()
    x = g.x[g.sets['binades']].reshape(len(R.LOG_ES), 10)
    assert (np.frexp(x[:, 0])[1] - 1).tolist() == list(R.LOG_ES) and x[-1].max() == np.finfo(float).max
    assert np.all(x[60:, 3] / x[60:, 0] == np.nextafter(x[60:, 4] / x[60:, 0], 0.)) and np.all(np.abs(x[60:, 3] / x[60:, 0] - math.sqrt(2.)) < 1e-15)
    assert len(g.sets['near_one']) == 82
    for which, per in (('rcp', 2), ('rsq', 1)):
        g = R.rcp_cases(which)
        assert len(g.x) == per * 6 * len(R.RCP_ES) and (np.frexp(g.x[:6 * len(R.RCP_ES):6])[1] - 1).tolist() == list(R.RCP_ES)
    g = R.rcp_cases('rcp')
    assert len(g.sets['subnormal']) >= 20 and len(g.sets['overflow']) >= 100
    assert R.LFAC_YS[:201] == [float(y) for y in range(201)] and R.LFAC_YS[201:] == [1e3, 1e6, 1e9, 2. ** 53]
    assert float(R.lfac_bound(0.)) == 0. and float(R.lfac_bound(1.)) == 0.


def test_working_range_cases_meet_the_cap_and_cover_every_branch():
    for kind, regime in ((R.BERNOULLI, 'working'), (R.POISSON, 'working'), (R.GAUSSIAN, 'working'), (R.GAUSSIAN, 'subnormal')):
        g = R.working_cases(kind, regime)
        assert max(g.form_rel) <= R.CAP and max(g.density_rel) <= R.CAP, (kind, regime)
        assert min(g.form_rel) >= 2 * R.U and min(g.density_rel) >= 2 * R.U      # never tighter than one rounding, doubled
    g = R.working_cases(R.BERNOULLI)
    assert np.all(g.lp != 0.) and np.abs(g.eta).max() <= 30. and np.abs(g.eta).max() > 20.
    assert (g.y == 0.).sum() >= 50 and (g.y == 1.).sum() >= 100 and g.eta[g.y == 1.].min() < -20.
    g = R.working_cases(R.POISSON)
    assert g.eta.min() == -8. and g.eta.max() == 700.
    for y in R.POISSON_YS:
        assert (g.y == y).sum() >= 5, y
    g = R.working_cases(R.GAUSSIAN)
    z = np.abs(g.y - g.eta) / np.sqrt(g.var)
    assert z.max() <= 37. + 1e-9 and z.max() > 30. and g.var.min() < 1e-9 and g.var.max() > 1e9
    assert g.var.min() >= 1e-12 and g.var.max() <= 1e12
    g = R.working_cases(R.GAUSSIAN, 'subnormal')
    ex = np.array([float(e) for e in g.form_exact])
    assert g.var.min() >= 1. and (ex < 2.2e-308).all() and (ex > 0).sum() >= 20 and (ex < 1e-322).sum() >= 3
    assert max(R.bearing_cases().rel) <= R.CAP


def test_edge_tables_expect_what_the_reference_formulas_give():
    e = R.poisson_edges()
    with np.errstate(all='ignore'):
        ref = stats.poisson_pmf(e.y, e.rate)
    sharp = e.want != -1.
    assert np.array_equal(ref[sharp], e.want[sharp], equal_nan=True)
    assert np.all((ref[~sharp] >= 0.) & (ref[~sharp] <= 1.))
    assert set(e.eta[e.rate == 0.]) == {-36.8, -37., -40., -100., -700., -745.} and set(e.eta[np.isinf(e.rate)]) == {710., 800., np.inf}
    b = R.bernoulli_edges()
    binary = (b.y == 0.) | (b.y == 1.)
    with np.errstate(all='ignore'):
        ref = stats.bernoulli_pmf(b.y[binary], b.p[binary])
    want = b.expected[binary]
    sharp = (want == 0.) | (want == 1.)
    assert np.array_equal(ref[sharp], want[sharp])
    assert np.all(np.abs(ref[~sharp] / want[~sharp] - 1.) <= 8 * R.U)
    assert np.isinf(b.z[-4:]).all() and b.expected[-4:].tolist() == [0., 1., 1., 0.]
    # y = 0.5, 2 and NaN follow the device's documented rule, which the reference does not define: y > 0.5 reads as 1
    odd = b.expected[~binary]
    assert np.array_equal(odd, np.where(b.y[~binary] > 0.5, b.p[~binary], 1. - b.p[~binary]))
    with np.errstate(all='ignore'):
        assert np.isnan(stats.norm_pdf(np.nan, 0., 1.)) and np.isnan(stats.norm_pdf(0., np.nan, 1.))
        assert np.isnan(stats.poisson_pmf(np.nan, 1.)) and np.isnan(stats.poisson_pmf(0., np.nan))
