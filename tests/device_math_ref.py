"""Cases, exact references and error bounds for the shared device layer (csrc/device_util.hpp, csrc/likelihood.hpp) as
mfs_device_math runs it, shared by tests/test_gpu_device_math.py and tests/test_host_device_math.py.  Every reference is the
same formula on the same fp64 inputs in mpmath at 200 bits (polynomials: exact rationals); each group is computed once per
session (functools.lru_cache) and never written to.  Nothing here touches the GPU except `call`.

Error measure.  |got - exact| against a bound in absolute terms, reported as their ratio (<= 1 passes).  Results on the
subnormal grid are measured on that grid (spacing 2^-1074).  Where the exact result lies within 4 spacings of the overflow
threshold, +-inf is accepted beside the finite neighbour; towards underflow every bound below has a floor of one subnormal
spacing, which accepts either neighbour.

Bounds of the elementary routines (the project's own figures): fast_exp max(4e-16 |exact|, 2^-1074); fast_tanh 3e-16
absolute; fast_log 4e-16 max(|exact|, 1).  Newton reciprocals: 2^-52 |exact| on normal results (the last fma leaves under one
ulp), one spacing on subnormal ones.  log_factorial: 2^-53 (y + 2) ln y! for y <= 32 (one ulp per log, half an ulp per
addition), 4 * 2^-52 z ln z with z = y + 1 above.

Bounds of the likelihood forms: first-order propagation through the form's own operations, u = 2^-53 per +, x, fma, 2u per
reciprocal, rsqrt, sqrt or divide, the elementary bounds above per exp / log (E_e = 4e-16 relative, E_l = 4e-16 max(|log|, 1)
absolute; libm's are granted the same, and so is atan2), conditioning factors evaluated in mpmath at the case's inputs, the
total doubled.  The domain: var > 0 finite; y a non-negative integer-valued double for the Poisson law.

  Bernoulli.  z = l0 + x (l1 + x (l2 + x l3)): six operations, |dz| <= 6u Z, Z = sum |l_j| |x|^j (0 for lik_density, which
    takes z).  e = exp(-z): relative E_e + |dz|.  p = 1 / (1 + e): dp / p = (1 - p) de / e, plus u for the sum and 2u for the
    reciprocal: R_p = (1 - p)(E_e + |dz|) + 3u.  y > 0.5 returns p.  Otherwise q = 1 - p: |dq| <= p R_p + u q, so
    R_q = p R_p / q + u -- the logistic's p (1 - p) conditioning; for z >~ 10 the subtraction cancels and no fp64 form of this
    formula (the reference's included) keeps q, which is why the working range of y = 0 ends there (the bound cap below).
  Poisson.  eta = l0 x: |d eta| <= u |eta| (0 for lik_density).  E = exp(eta), s = 1 + E, rate = log s, sigma = E / s:
    |d rate| <= E_l max(rate, 1) + u + sigma (E_e + |d eta|).  L = log(rate): |dL| <= E_l max(|L|, 1) + |d rate| / rate (the
    softplus' 1 / rate).  t = y L - rate - log y!: |dt| <= y |dL| + u |y L| + |d rate| + u |y L - rate| + d(log y!) + u |t|
    (the y / rate conditioning is the first term).  pmf = exp(t): relative E_e + |dt|.
  Gaussian.  m = l0 x + l1, r = y - m: |dr| <= u |l0 x| + u |m| + u |r| (lik_density takes m: u |r|; the bearing factor adds
    atan2's E_l max(|m|, 1)).  a = -r^2 / (2 var): |da| <= |r| |dr| / var + 4u |a| (two products, 2u for the reciprocal or the
    divide).  exp(a): E_e + |da|; rsqrt(2 pi var): 3u; the product: u.  Relative E_e + |da| + 4u.
  Subnormal results (the last exp underflows gradually): one spacing is added before the doubling -- the exponential's own
    floor scaled by rsqrt(2 pi var) < 0.4 (sd >= 1) plus half a spacing of the product's rounding.

Condition on the reference alone: every working-range case has a doubled relative bound <= CAP = 1e-11.  The generators
draw candidates from a seeded stream and keep the first that meet it, so a case that misses is replaced, never skipped."""
import functools
import math
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np

mp.mp.prec = 200
mpf = mp.mpf
U = 2.0 ** -53
E_EXP = 4e-16
E_LOG = 4e-16
E_TANH = 3e-16
CAP = 1e-11
TINY = mpf(2) ** -1074
MIN_NORMAL = mpf(2) ** -1022
DBL_MAX = mpf(sys.float_info.max)
OVER = mpf(2) ** 1024
SP_TOP = mpf(2) ** 971          # fp64 spacing below the overflow threshold
NAN = 'nan'                     # marker in the exact lists

BERNOULLI, POISSON, GAUSSIAN, BEARING = 0, 1, 2, 3
MAX_LIK, MAX_DEGREE, EXTENT_HI, LFAC_MAX = 4, 15, 7, 32
FN = {'exp': 0, 'exp_sc': 1, 'tanh': 2, 'log': 3, 'log_sc': 4, 'rcp_nr': 5, 'rcp_sat': 6, 'rsq_nr': 7, 'log_factorial': 8,
      'horner': 9, 'poly2': 10, 'poly2_grad': 11, 'chol2': 12, 'likelihood': 13, 'likelihood_nd': 14, 'lik_density': 15,
      'lik_density_sc': 16, 'likelihood_joint_nd': 17, 'likelihood_fast': 18, 'likelihood_fast_regs': 19, 'lfac_table': 20}
SHAPE = {**{k: (1, 1) for k in ('exp', 'exp_sc', 'tanh', 'log', 'log_sc', 'rcp_nr', 'rcp_sat', 'rsq_nr', 'log_factorial',
                                'lfac_table')},
         'horner': (2 + MAX_DEGREE + 1, 1), 'poly2': (3 + EXTENT_HI ** 2, 1), 'poly2_grad': (3 + EXTENT_HI ** 2, 3),
         'chol2': (3, 4), 'lik_density': (4, 1), 'lik_density_sc': (4, 1), 'likelihood_joint_nd': (MAX_LIK + 4, 1),
         **{k: (MAX_LIK + 3, 1) for k in ('likelihood', 'likelihood_nd', 'likelihood_fast', 'likelihood_fast_regs')}}
FORMS = ('likelihood', 'likelihood_nd', 'lik_density', 'lik_density_sc', 'likelihood_fast', 'likelihood_fast_regs')


def call(fn, cols):
    """mfs_device_math on the columns `cols` ([n_in] arrays or scalars, broadcast together): the [n_out][n] result."""
    from mfs_amd import _lib
    cols = np.broadcast_arrays(*[np.asarray(c, dtype=np.float64) for c in cols])
    a = np.ascontiguousarray(np.stack([c.ravel() for c in cols]))
    n_in, n_out = SHAPE[fn]
    assert a.shape[0] == n_in, (fn, a.shape)
    out = np.full((n_out, a.shape[1]), -7.25)
    _lib.check(_lib.lib().mfs_device_math(FN[fn], a.shape[1], n_in, _lib.ptr(a), n_out, _lib.ptr(out), 0))
    return out


# ---- the error measure
def spacing(e):
    """fp64 spacing at the exact value e (the subnormal grid below 2^-1022)."""
    a = abs(e)
    if a < MIN_NORMAL:
        return TINY
    return mpf(2) ** (mp.frexp(a)[1] - 53)


def ratios(got, exact, bound):
    """|got - exact| / bound per element; inf for a wrong special.  exact: mpf, +-mp.inf or NAN; bound: mpf / float."""
    out = np.empty(len(exact))
    for i, (g, e, b) in enumerate(zip(np.asarray(got, dtype=np.float64).tolist(), exact, bound)):
        if isinstance(e, str):
            out[i] = 0. if g != g else np.inf
        elif mp.isinf(e) or abs(e) >= OVER + 4 * SP_TOP:
            out[i] = 0. if (math.isinf(g) and (g > 0) == (e > 0)) else np.inf
        elif g != g:
            out[i] = np.inf
        elif math.isinf(g):
            out[i] = 0. if (abs(e) >= OVER - 4 * SP_TOP and (g > 0) == (e > 0)) else np.inf
        else:
            err = abs(mpf(g) - e)
            out[i] = 0. if err == 0 else (float(err / b) if b > 0 else np.inf)
    return out


def _neighbours(c, width=2):
    """The doubles within +-width ulp of the real number c."""
    d = float(c)
    out, lo, hi = [d], d, d
    for _ in range(width):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [float(lo), float(hi)]
    return out


def _around(c):
    """The two doubles around the real number c."""
    d = float(c)
    return [float(np.nextafter(d, -np.inf)), d] if mpf(d) > c else [d, float(np.nextafter(d, np.inf))]


class Group(dict):
    """x: the inputs ([n] or [n_in][n]); exact, bound: lists; sets: name -> indices (the host test counts them)."""
    __getattr__ = dict.__getitem__


# ---- elementary functions
EXP_KS = range(-1076, 1026)


@functools.lru_cache(None)
def exp_cases():
    ln2 = mp.ln(2)
    xs, sets = [], {}

    def add(name, vals):
        sets[name] = list(range(len(xs), len(xs) + len(vals)))
        xs.extend(vals)
    add('half', [v for k in EXP_KS for v in _neighbours((k + mpf(0.5)) * ln2)])      # largest |r|
    add('flip', [v for k in EXP_KS for v in _neighbours(k * ln2)])                   # ... and where rint flips
    mag = 10. ** np.random.default_rng(101).uniform(-320., 0., 2000)
    add('small', np.concatenate([mag, -mag]).tolist())
    add('thresholds', [0., -0.] + _around(-1075 * ln2) + _around(-1022 * ln2) + _around(mp.log(DBL_MAX)) + [-745.5, 710.])
    add('specials', [1e308, -1e308, np.inf, -np.inf, np.nan])
    x = np.array(xs)
    exact = []
    for v in xs:
        exact.append(NAN if v != v else mp.inf if v > 1e4 else mpf(0) if v < -1e4 else mp.exp(mpf(v)))
    bound = [None if isinstance(e, str) or mp.isinf(e) else max(mpf(E_EXP) * e, TINY) for e in exact]
    return Group(x=x, exact=exact, bound=bound, sets=sets)


@functools.lru_cache(None)
def exp_sharp_bounds():
    """A second, sharper bound on fast_exp, from its own operations (first order, NOT doubled: it is there to see one missing
    Taylor term, 1 / 13! at |r| = ln 2 / 2 being 2.4e-16 of the result).  y is clamped, k = rint(y log2 e) in fp64 as on the device,
    r = y - k ln 2 exactly.  The first reduction fma is exact (the high word of ln 2 has 21 trailing zeros), the second rounds: u |r|.
    Horner with fma, p_13 = 1 / 13!, p_j = fl(p_{j+1} r + 1 / j!), result p_0: |d p_0| <= u sum_j |r|^j |p_j| with
    |p_j| <= e^|r| / j!, so sum_{j >= 1} <= e^|r| (e^|r| - 1), and the j = 0 term is the result itself.  Truncation |r|^14 / 14!.
    Relative: u (1 + e^|r| (e^|r| - 1) / e^r + |r|) + |r|^14 / (14! e^r); ldexp is exact on normal results and rounds by at
    most half a spacing on subnormal ones.  The sets 'half', 'flip' and 'small'; a result that overflows is left to `ratios`."""
    g, ln2 = exp_cases(), mp.ln(2)
    idx = g.sets['half'] + g.sets['flip'] + g.sets['small']
    bound = []
    for i in idx:
        yc = min(max(float(g.x[i]), -745.5), 710.)
        r = mpf(yc) - int(np.rint(yc * 1.4426950408889634)) * ln2
        a, e = abs(r), g.exact[i]
        rel = U * (1 + mp.exp(a) * (mp.exp(a) - 1) / mp.exp(r) + a) + a ** 14 / (mp.factorial(14) * mp.exp(r))
        bound.append(rel * e + (TINY / 2 if e < MIN_NORMAL else 0))
    return idx, bound


TANH_ES = range(-1074, 6)


@functools.lru_cache(None)
def tanh_cases():
    xs, sets = [], {}

    def add(name, vals):
        vals = [s * v for v in vals for s in (1., -1.)]      # pairs (x, -x): oddness is checked on neighbours
        sets[name] = list(range(len(xs), len(xs) + len(vals)))
        xs.extend(vals)
    add('binades', [float(np.ldexp(m, e)) for e in TANH_ES for m in (1., 1.75)])
    add('dense', (10. ** np.random.default_rng(102).uniform(-3., math.log10(20.), 1500)).tolist())
    add('clamp', _neighbours(mpf(20)))
    add('specials', [np.inf, 0.])
    sets['nan'] = [len(xs)]
    xs.append(np.nan)
    exact = [NAN if v != v else mpf(1) if v == np.inf else mpf(-1) if v == -np.inf else mp.tanh(mpf(v)) for v in xs]
    return Group(x=np.array(xs), exact=exact, bound=[mpf(E_TANH)] * len(xs), sets=sets)


LOG_ES = range(-1074, 1024)


@functools.lru_cache(None)
def log_cases():
    r2 = _around(mp.sqrt(2))
    seeded = np.random.default_rng(103).uniform(1., 2., (len(LOG_ES), 5))
    xs, sets = [], {}

    def add(name, vals):
        sets[name] = list(range(len(xs), len(xs) + len(vals)))
        xs.extend(vals)
    add('binades', [float(np.ldexp(m, e)) for i, e in enumerate(LOG_ES)
                    for m in [1., 1. + 2. ** -52, 2. - 2. ** -52] + r2 + seeded[i].tolist()])
    add('near_one', [1. + s * 2. ** (j - 53) for j in range(41) for s in (1., -1.)])
    add('one', [1., 1. + 2. ** -52])
    n_finite = len(xs)
    add('specials', [0., -0., np.inf, -1., -np.inf, np.nan])
    exact = [mp.log(mpf(v)) for v in xs[:n_finite]] + [-mp.inf, -mp.inf, mp.inf, None, None, NAN]
    bound = [None if (e is None or isinstance(e, str) or mp.isinf(e)) else mpf(E_LOG) * max(abs(e), 1) for e in exact]
    return Group(x=np.array(xs), exact=exact, bound=bound, sets=sets)


RCP_ES = range(-1074, 1024)


@functools.lru_cache(None)
def rcp_cases(which):
    """which: 'rcp' (both signs; 1 / v) or 'rsq' (v > 0; 1 / sqrt(v)).  exact is None where 1 / v overflows: non-finite."""
    seeded = np.random.default_rng(104).uniform(1., 2., (len(RCP_ES), 2))
    v = np.array([float(np.ldexp(m, e)) for i, e in enumerate(RCP_ES)
                  for m in [1., 1. + 2. ** -52, 1.5, 2. - 2. ** -52] + seeded[i].tolist()])
    if which == 'rcp':
        v = np.concatenate([v, -v])
    exact, bound = [], []
    for t in v.tolist():
        e = 1 / mpf(t) if which == 'rcp' else 1 / mp.sqrt(mpf(t))
        if abs(e) >= OVER:
            e = None                                   # overflow: asserted non-finite
        exact.append(e)
        bound.append(None if e is None else max(mpf(2) ** -52 * abs(e), TINY))
    sets = {'overflow': [i for i, e in enumerate(exact) if e is None],
            'subnormal': [i for i, e in enumerate(exact) if e is not None and abs(e) < MIN_NORMAL]}
    sets['normal'] = [i for i, e in enumerate(exact) if e is not None and abs(e) >= MIN_NORMAL]
    return Group(x=v, exact=exact, bound=bound, sets=sets)


LFAC_YS = [float(y) for y in range(201)] + [1e3, 1e6, 1e9, 2. ** 53]


def lfac_bound(y):
    """The bound on log_factorial(y) (module docstring), as an mpf."""
    y = mpf(y)
    if y <= LFAC_MAX:
        return mpf(U) * (y + 2) * mp.loggamma(y + 1)
    return 4 * mpf(2) ** -52 * (y + 1) * mp.log(y + 1)


@functools.lru_cache(None)
def lfac_cases():
    exact = [mp.loggamma(mpf(y) + 1) for y in LFAC_YS]
    return Group(x=np.array(LFAC_YS), exact=exact, bound=[lfac_bound(y) for y in LFAC_YS], sets={})


# ---- polynomials (exact rationals) and the 2 x 2 Cholesky factor
def _coefs(rng, n):
    """n seeded coefficients of mixed sign and magnitude, some zero."""
    c = rng.standard_normal(n) * 10. ** rng.integers(-3, 4, n)
    c[rng.random(n) < 0.1] = 0.
    return c


@functools.lru_cache(None)
def horner_cases():
    rng = np.random.default_rng(105)
    rows = []
    for degree in range(MAX_DEGREE + 1):
        for u in [0., 1., -1., 0.5, -3.] + rng.uniform(-2.5, 2.5, 5).tolist():
            row = np.zeros(MAX_DEGREE + 1)
            row[:degree + 1] = _coefs(rng, degree + 1)
            row[degree + 1:] = 1e300               # beyond the degree: must not be read into the sum
            rows.append(np.concatenate([[degree, u], row]))
    x = np.array(rows).T
    exact, bound = [], []
    for col in x.T:
        degree, u, row = int(col[0]), Fraction(col[1]), [Fraction(v) for v in col[2:]]
        exact.append(sum(row[j] * u ** j for j in range(degree + 1)))
        bound.append(2 * (2 * degree) * Fraction(U) * sum(abs(row[j]) * abs(u) ** j for j in range(degree + 1)))
    return Group(x=x, exact=exact, bound=bound, sets={})


@functools.lru_cache(None)
def poly2_cases():
    """exact / bound: [3][n] -- value, d / dx0, d / dx1.  ops = 2 D^2 for the value, 6 D^2 (every operation of the loop) for the
    gradient form's three outputs."""
    rng = np.random.default_rng(106)
    rows = []
    for D in range(1, EXTENT_HI + 1):
        for x0, x1 in [(0., 0.), (1., -1.), (-0.5, 2.)] + rng.uniform(-2., 2., (7, 2)).tolist():
            c = np.full(EXTENT_HI ** 2, 1e300)     # beyond D x D: must not be read
            c[:D * D] = _coefs(rng, D * D)
            rows.append(np.concatenate([[D, x0, x1], c]))
    x = np.array(rows).T
    exact, bound = [[], [], []], [[], [], []]
    for col in x.T:
        D, x0, x1 = int(col[0]), Fraction(col[1]), Fraction(col[2])
        c = [[Fraction(col[3 + a * D + b]) for b in range(D)] for a in range(D)]
        terms = [(c[a][b], a, b) for a in range(D) for b in range(D)]
        for k, (da, db) in enumerate([(0, 0), (1, 0), (0, 1)]):
            def mono(t, x0=x0, x1=x1, da=da, db=db):
                cab, a, b = t
                if a < da or b < db:
                    return Fraction(0)
                return cab * (a if da else 1) * (b if db else 1) * x0 ** (a - da) * x1 ** (b - db)
            exact[k].append(sum(mono(t) for t in terms))
            absx = sum(abs(mono((abs(cab), a, b), abs(x0), abs(x1))) for cab, a, b in terms)
            bound[k].append((2 * (2 * D * D) * Fraction(U) * absx, 2 * (6 * D * D) * Fraction(U) * absx))
    return Group(x=x, exact=exact, bound=bound, sets={})


def frac_ratios(got, exact, bound):
    out = np.empty(len(exact))
    for i, (g, e, b) in enumerate(zip(np.asarray(got).tolist(), exact, bound)):
        if not math.isfinite(g):
            out[i] = np.inf
            continue
        err = abs(Fraction(g) - e)
        out[i] = 0. if err == 0 else (float(err / b) if b > 0 else np.inf)
    return out


@functools.lru_cache(None)
def chol2_cases():
    """Accuracy cases (ok = 1): l00 2u; l10 4u; d1 = p11 - l10^2 carries 9u l10^2 + u d1, l11 = sqrt(d1) half of that relative
    plus 2u; all doubled.  The ill-conditioned ones keep d1 >= 1e3 times its own error, so that the flag is decided."""
    rng = np.random.default_rng(107)
    P = [(4., 2., 1. + 1.), (1., 0., 1.), (2.5, -1.5, 7.)]
    for _ in range(12):                                     # well conditioned
        a, b = rng.uniform(0.5, 2., 2) * 10. ** rng.integers(-3, 4, 2)
        P.append((a * a, a * b * rng.uniform(-0.9, 0.9), b * b))
    for eps in (1e-3, 1e-6, 1e-9, 1e-11):                   # correlation 1 - eps
        for _ in range(3):
            a, b = rng.uniform(0.5, 2., 2)
            P.append((a * a, a * b * (1. - eps) * rng.choice([-1., 1.]), b * b))
    x = np.array(P).T
    exact, bound = [[], [], []], [[], [], []]
    for p00, p01, p11 in x.T.tolist():
        l00 = mp.sqrt(mpf(p00))
        l10 = mpf(p01) / l00
        d1 = mpf(p11) - l10 * l10
        assert d1 > 0
        dd1 = 9 * U * l10 * l10 + U * d1
        assert d1 >= 1e3 * dd1
        l11 = mp.sqrt(d1)
        for k, (e, b) in enumerate([(l00, 2 * U * l00), (l10, 4 * U * abs(l10)), (l11, (dd1 / d1 / 2 + 2 * U) * l11)]):
            exact[k].append(e)
            bound[k].append(2 * b)
    return Group(x=x, exact=exact, bound=bound, sets={})


# (p00, p01, p11) -> ok: the documented pivot rules
CHOL2_RULES = [((4., 2., 1.), 1.),             # zero second pivot: legal (P = l l^T of rank one)
               ((1., 0., 0.), 1.),
               ((0., 0., 1.), 0.),             # zero first pivot: 0 / 0
               ((0., 1., 1.), 0.),             # ... 1 / 0
               ((-1., 0., 1.), 0.), ((1., 0., -1.), 0.), ((1., 2., 1.), 0.),      # negative pivots
               ((np.inf, 0., 1.), 0.), ((1., 0., np.inf), 0.), ((1., np.inf, 1.), 0.),
               ((np.nan, 0., 1.), 0.), ((1., np.nan, 1.), 0.), ((1., 0., np.nan), 0.)]


# ---- likelihood forms: exact values and bounds (module docstring)
def _subnormal_floor(e):
    return TINY if abs(e) < MIN_NORMAL else mpf(0)


def bernoulli_exact(lp, y, x, link_ops):
    """(exact, relative bound before doubling) of the Bernoulli-logistic pmf with the device's y > 0.5 rule."""
    lp, x = [mpf(v) for v in lp], mpf(x)
    z = lp[0] + x * (lp[1] + x * (lp[2] + x * lp[3]))
    dz = link_ops * U * sum(abs(lp[j]) * abs(x) ** j for j in range(4))
    e = mp.exp(-z)
    p = 1 / (1 + e)
    q = e / (1 + e)
    rp = q * (E_EXP + dz) + 3 * U
    return (p, rp) if y > 0.5 else (q, p * rp / q + U)


def poisson_exact(eta, y, link_ops):
    eta, y = mpf(eta), mpf(y)
    E = mp.exp(eta)
    rate = mp.log(1 + E)
    L = mp.log(rate)
    d_rate = E_LOG * max(rate, 1) + U + E / (1 + E) * (E_EXP + link_ops * U * abs(eta))
    d_L = E_LOG * max(abs(L), 1) + d_rate / rate
    lf = mp.loggamma(y + 1)
    t = y * L - rate - lf
    d_t = y * d_L + U * abs(y * L) + d_rate + U * abs(y * L - rate) + lfac_bound(y) + U * abs(t)
    return mp.exp(t), E_EXP + d_t


def gaussian_exact(m, d_m, var, y):
    """m: the exact mean, d_m: the absolute error granted to the device's."""
    var, r = mpf(var), mpf(y) - m
    a = -r * r / (2 * var)
    d_r = d_m + U * abs(r)
    d_a = abs(r) * d_r / var + 4 * U * abs(a)
    return mp.exp(a) / mp.sqrt(2 * mp.pi * var), E_EXP + d_a + 4 * U


def form_exact(kind, lp, y, x):
    """A form that takes (lp, y, x): the link is the device's to compute."""
    if kind == BERNOULLI:
        return bernoulli_exact(lp, y, x, 6)
    if kind == POISSON:
        return poisson_exact(mpf(lp[0]) * mpf(x), y, 1)
    m = mpf(lp[0]) * mpf(x) + mpf(lp[1])
    return gaussian_exact(m, U * abs(mpf(lp[0]) * mpf(x)) + U * abs(m), lp[2], y)


def density_exact(kind, eta, var, y):
    """lik_density: the link value is an input."""
    if kind == BERNOULLI:
        return bernoulli_exact([eta, 0., 0., 0.], y, 0., 0)
    if kind == POISSON:
        return poisson_exact(eta, y, 0)
    return gaussian_exact(mpf(eta), 0, var, y)


def link_fp64(kind, lp, x):
    """The link value in fp64, one legitimate evaluation of it: what the agreement test hands to lik_density."""
    lp = np.asarray(lp, dtype=np.float64)
    if kind == BERNOULLI:
        return lp[0] + x * (lp[1] + x * (lp[2] + x * lp[3]))
    return lp[0] * x if kind == POISSON else lp[0] * x + lp[1]


POISSON_YS = [float(y) for y in range(41)] + [75., 200.]
POISSON_CORNERS = [(-8., 0.), (-8., 1.), (-8., 2.), (700., 0.), (700., 32.), (700., 33.), (700., 200.), (0., 0.), (0., 1.)]
KIND_NAME = {BERNOULLI: 'bernoulli', POISSON: 'poisson', GAUSSIAN: 'gaussian'}


def _working_candidates(kind, regime, rng):
    """An endless seeded stream of (lp[4], y, x, var) candidates of one kind."""
    if kind == BERNOULLI:
        while True:
            lp = rng.uniform(0.1, 2., 4) * rng.choice([-1., 1.], 4)
            x = rng.uniform(-2.5, 2.5)
            z = link_fp64(kind, lp, x)
            if abs(z) <= 30.:
                yield lp, float(rng.integers(0, 2)), x
    elif kind == POISSON:
        for eta, y in POISSON_CORNERS:                # the ends of the working range, at the counts whose bound allows them
            yield np.array([1., 0., 0., 0.]), y, eta
        k = 0
        while True:
            y = POISSON_YS[k % len(POISSON_YS)]       # every count in turn; the stream retries a count until a link fits it
            for _ in range(10000):
                lp0 = rng.uniform(0.5, 2.) * rng.choice([-1., 1.])
                # links over [-8, 700], denser at the small rates where the softplus is ill-conditioned
                eta = rng.choice([rng.uniform(-8., 5.), rng.uniform(-8., 700.), 10. ** rng.uniform(0., math.log10(700.))])
                cand = np.array([lp0, 0., 0., 0.]), y, eta / lp0
                if -8. <= link_fp64(kind, cand[0], cand[2]) <= 700. and _meets_cap(kind, cand):
                    break
            else:
                raise AssertionError(f'no link in [-8, 700] meets the cap at y = {y}')
            yield cand
            k += 1
    else:
        while True:
            sd = 10. ** rng.uniform(-6., 6.)
            if regime == 'subnormal':
                sd = 10. ** rng.uniform(0., 3.)
            l0, l1, x = rng.uniform(-2., 2.), rng.uniform(-3., 3.), rng.uniform(-4., 4.)
            # (a small variance amplifies the rounding of the mean by |r| / var: such cases fit the cap only close to the mean)
            dev = rng.uniform(37.7, 38.55) if regime == 'subnormal' else rng.choice([rng.uniform(0., 37.), 10. ** rng.uniform(-3., 1.5)])
            y = (l0 * x + l1) + rng.choice([-1., 1.]) * dev * sd
            yield np.array([l0, l1, sd * sd, 0.]), y, x


def _meets_cap(kind, cand):
    lp, y, x = cand
    return 2 * form_exact(kind, lp, y, x)[1] <= CAP


N_WORKING = {BERNOULLI: 300, POISSON: len(POISSON_CORNERS) + 5 * len(POISSON_YS), GAUSSIAN: 300}


@functools.lru_cache(None)
def working_cases(kind, regime='working'):
    """The accuracy cases of one kind: inputs of the (lp, y, x) forms, their exact value and absolute bound, and the same for
    lik_density on the fp64 link.  Every case meets the cap; the first candidates of the stream that do are kept."""
    rng = np.random.default_rng(200 + 10 * kind + (regime == 'subnormal'))
    n = 60 if regime == 'subnormal' else N_WORKING[kind]
    lps, ys, xs = [], [], []
    for cand in _working_candidates(kind, regime, rng):
        if kind == POISSON or _meets_cap(kind, cand):
            lps.append(cand[0]); ys.append(cand[1]); xs.append(cand[2])
        if len(ys) == n:
            break
    lp, y, x = np.array(lps), np.array(ys), np.array(xs)
    eta = np.array([link_fp64(kind, lp[i], x[i]) for i in range(n)])
    var = lp[:, 2] if kind == GAUSSIAN else np.zeros(n)
    out = Group(kind=kind, lp=lp, y=y, x=x, eta=eta, var=var, sets={})
    for name, fn in (('form', lambda i: form_exact(kind, lp[i], y[i], x[i])),
                     ('density', lambda i: density_exact(kind, eta[i], var[i], y[i]))):
        ex = [fn(i) for i in range(n)]
        out[name + '_exact'] = [e for e, _ in ex]
        out[name + '_rel'] = [2 * float(r) for _, r in ex]
        out[name + '_bound'] = [2 * (mpf(r) * abs(e) + _subnormal_floor(e)) for e, r in ex]
    return out


def form_columns(g):
    """The input columns of a (kind, lp[4], y, x) form."""
    return [g.kind, *g.lp.T, g.y, g.x]


def density_columns(g):
    return [g.kind, g.eta, g.var, g.y]


@functools.lru_cache(None)
def bearing_cases():
    rng = np.random.default_rng(260)
    n = 120
    x0, x1 = rng.uniform(-3., 3., (2, n))
    x0[:4], x1[:4] = [1., -1., 0., -2.], [0., 1e-3, 2., -1e-3]       # the axes and both sides of the branch cut
    sd = 10. ** rng.uniform(-2., 1., n)
    y = np.arctan2(x1, x0) + rng.uniform(-30., 30., n) * sd
    exact, bound, rel = [], [], []
    for i in range(n):
        m = mp.atan2(mpf(x1[i]), mpf(x0[i]))
        e, r = gaussian_exact(m, E_LOG * max(abs(m), 1), sd[i] ** 2, y[i])
        exact.append(e); rel.append(2 * float(r)); bound.append(2 * (mpf(r) * e + _subnormal_floor(e)))
    return Group(cols=[BEARING, sd * sd, 0., 0., 0., y, x0, x1], exact=exact, bound=bound, rel=rel, sets={})


# ---- edges: outcomes of the reference formula's fp64 semantics (xlogy, 1 / (1 + inf) = 0)
BERN_Z = [37., 40., 700., 745., 800., 1e308]
BERN_Y = [0., 1., 0.5, 2., np.nan]


def bernoulli_edges():
    """Columns (lp[4], y, x) and the expected value: p if y > 0.5 else 1 - p (NaN reads as 0), with p of the reference formula
    in fp64.  The last four rows overflow x^3."""
    rows = [([s * z, 0., 0., 0.], y, 0.) for z in BERN_Z for s in (1., -1.) for y in BERN_Y]
    rows += [([0., 0., 0., 1.], y, x) for x in (1e103, -1e103) for y in (0., 1.)]
    lp, y, x = np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    with np.errstate(all='ignore'):
        z = lp[:, 0] + x * (lp[:, 1] + x * (lp[:, 2] + x * lp[:, 3]))
        p = 1. / (1. + np.exp(-z))
    return Group(lp=lp, y=y, x=x, z=z, p=p, expected=np.where(y > 0.5, p, 1. - p))


POIS_EDGE_ETA = [-30., -33., -36., -36.5, -36.7, -36.8, -37., -40., -100., -700., -745., 710., 800., np.inf]
POIS_EDGE_Y = [0., 1., 2., 5., 33.]


def poisson_edges():
    """Columns and, per row: rate (the reference's, fp64) and the asserted outcome -- 'unit' (finite, in [0, 1]), or the exact
    value 1., 0. or NaN once the rate is 0 or inf."""
    rows = [(eta, y) for eta in POIS_EDGE_ETA for y in POIS_EDGE_Y]
    eta, y = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    with np.errstate(all='ignore'):
        rate = np.log(1. + np.exp(eta))
    want = np.where(rate == 0., np.where(y == 0., 1., 0.), np.where(np.isinf(rate), np.where(y == 0., 0., np.nan), -1.))
    return Group(eta=eta, y=y, rate=rate, want=want)       # want = -1: only 'unit'
