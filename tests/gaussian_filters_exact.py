"""Arbiter of the Gaussian-filter envelope tests: the sigma-point filter and the EKF of include/mfs_hip.h (mfs_gaussian_filter_1d /
_nd) in 50-digit arithmetic (mpmath), a closed-form assumed-density filter that uses no quadrature rule at all, a matrix Kalman
filter, and the table of cases that tests/golden/make_gaussian_filters_exact.py freezes into tests/golden/
gaussian_filters_exact.npz and that tests/test_host_gaussian_filters.py and tests/test_gpu_gaussian_filters_envelope.py read.
A plain helper module, not a conftest.

Every function takes the arrays the device receives -- the coefficient table, the likelihood parameters, the rule, the initial
law, the measurements -- and takes every double as exact.  At 50 digits the order of a sum of <= 256 terms is invisible, so the
results owe nothing to the order in which fp64 code adds.

    sigma_point_mp / ekf_mp   the step of include/mfs_hip.h restated: the same operation as the device, in high precision,
                              with the NaN rule (a negative or non-finite Cholesky pivot, S not finite and > 0, a measurement
                              that is not finite)
    adf_closed_form           polynomial tables in x and the Gaussian kind: E[mu], E[mu mu^T + S] under N(m, P) from the moments
                              of the standard Normal (E z^k = (k - 1)!!), then the linear-Gaussian update.  Any rule that is exact
                              to degree max(2 deg mu, deg S) per standard variable must reproduce it -- deg the TOTAL degree at
                              d = 2, where x_1 = m_1 + l10 z_0 + l11 z_1 carries z_0 as well; it depends on nobody's reading
                              of the point layout or of the sigma-point equations
    kalman_mp                 the matrix Kalman filter of a linear model

Two statements about numbers outside the range of a double, so that "the same operation" stays well defined there:
  * the rule on S is applied to S as a double (float(S) > 0 and finite): a logistic factor a few thousand into its tail has
    p (1 - p) = 1e-2000, which is 0 in every fp64 output;
  * a zero first pivot with d = 2 makes l10 = P01 / 0, which is NaN or +-inf in IEEE arithmetic and fails the test on the second
    pivot: the arbiter poisons that step.
"""
import math
from typing import NamedTuple, Optional

import mpmath as mp
import numpy as np

DPS = 50
KINDS = ('bernoulli_logistic', 'poisson_softplus', 'gaussian')
SIGMA_POINT, EKF, ADF = 'sigma_point', 'ekf', 'adf'


class Model(NamedTuple):
    """What the device receives of a model.  d = 1: coef (2, J + 1) = mean, variance in ascending powers of u (or (R, 2, J + 1),
    one per replicate), mu(x) = cx x + P_m(u), u = x or tanh x.  d = 2: coef (5, D, D) = mu_0, mu_1, S_00, S_01, S_11,
    coef[r, a, b] multiplying x_0^a x_1^b.  lik (n_lik,) or (R, n_lik); component: the state component the measurement reads."""
    d: int
    coef: np.ndarray
    kind: str
    lik: np.ndarray
    umap: str = 'x'
    cx: float = 0.
    component: int = 0

    def replicate(self, r):
        coef = self.coef[r] if self.d == 1 and self.coef.ndim == 3 else self.coef
        lik = self.lik[r] if self.lik.ndim == 2 else self.lik
        return self._replace(coef=coef, lik=lik)


class Exact(NamedTuple):
    means: np.ndarray      # (T, d)
    covs: np.ndarray       # (T, d, d)
    nells: np.ndarray      # (T,) running sum
    first_nan: int
    trace: Optional[list] = None      # per step (m, P, nell) before rounding, None at a poisoned step


def _f(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def _finite(x):
    return bool(mp.isfinite(x))


def _pivot_ok(v):
    return _finite(v) and v >= 0


def _s_ok(S):
    if not _finite(S):
        return False
    s = float(S)
    return s > 0. and math.isfinite(s)


# ---- the model in mpmath
def measure_mp(kind, l, x):
    """(h, Xi, dh/dx) of the likelihood kinds of include/mfs_hip.h at x."""
    l = list(l) + [mp.mpf(0)] * (4 - len(l))
    if kind == 'bernoulli_logistic':
        z = l[0] + x * (l[1] + x * (l[2] + x * l[3]))
        p = 1 / (1 + mp.exp(-z))
        v = p * (1 - p)
        return p, v, v * (l[1] + x * (2 * l[2] + x * 3 * l[3]))
    if kind == 'poisson_softplus':
        z = l[0] * x
        rate = mp.log(1 + mp.exp(z))
        return rate, rate, l[0] / (1 + mp.exp(-z))
    if kind == 'gaussian':
        return l[0] * x + l[1], l[2], l[0]
    raise ValueError(kind)


def _horner(c, u):
    acc = mp.mpf(0)
    for v in reversed(c):
        acc = acc * u + v
    return acc


def trans1_mp(coef, umap, cx, x):
    """(mu, var, d mu / d x) at x for the d = 1 table."""
    u = mp.tanh(x) if umap == 'tanh' else x
    cm, cv = coef
    dm = _horner([k * cm[k] for k in range(1, len(cm))], u)
    return cx * x + _horner(cm, u), _horner(cv, u), cx + dm * ((1 - u * u) if umap == 'tanh' else 1)


def _poly2(c, x0, x1):
    return _horner([_horner(row, x1) for row in c], x0)


def trans2_mp(coef, x0, x1):
    """(mu (2,), S (00, 01, 11)) at x for the d = 2 table."""
    v = [_poly2(c, x0, x1) for c in coef]
    return v[:2], v[2:]


def jac2_mp(coef, x0, x1):
    """d mu_i / d x_j, i, j = 0, 1."""
    out = []
    for c in coef[:2]:
        D = len(c)
        d0 = [[a * c[a][b] for b in range(D)] for a in range(1, D)]
        d1 = [[b * c[a][b] for b in range(1, D)] for a in range(D)]
        out.append([_poly2(d0, x0, x1) if d0 else mp.mpf(0), _poly2(d1, x0, x1) if D > 1 else mp.mpf(0)])
    return out


def _chol2(p00, p01, p11):
    """-> (ok, l00, l10, l11) by the closed forms of the step."""
    if not _pivot_ok(p00) or p00 == 0 or not _finite(p01) or not _finite(p11):
        # a zero first pivot: l10 = p01 / 0 is NaN (p01 = 0) or +-inf, and p11 - l10^2 is then NaN or -inf
        return False, None, None, None
    l00 = mp.sqrt(p00)
    l10 = p01 / l00
    d1 = p11 - l10 * l10
    if not _pivot_ok(d1):
        return False, None, None, None
    return True, l00, l10, mp.sqrt(d1)


def _mp_table(model):
    if model.d == 1:
        assert model.coef.ndim == 2 and model.coef.shape[0] == 2, 'one replicate at a time: Model.replicate(r)'
        return [[_f(v) for v in row] for row in model.coef]
    assert model.coef.ndim == 3 and model.coef.shape[0] == 5
    return [[[_f(v) for v in row] for row in blk] for blk in model.coef]


class _Run:
    """The part of a run that both methods and both dimensions share: the update, the NaN rule and the outputs."""

    def __init__(self, model, m0, P0, ys):
        self.d = d = model.d
        self.kind, self.c = model.kind, int(model.component)
        assert np.ndim(model.lik) == 1, 'one replicate at a time: Model.replicate(r)'
        self.l = [_f(v) for v in model.lik]
        m0, P0 = np.asarray(m0, dtype=object).reshape(d), np.asarray(P0, dtype=object).reshape(d, d)
        self.m = [_f(v) for v in m0]
        self.P = [[_f(P0[max(i, j), min(i, j)]) for j in range(d)] for i in range(d)]      # the lower triangle counts
        self.ys = [_f(v) for v in np.asarray(ys, dtype=object).reshape(-1)]
        self.T = len(self.ys)
        self.nell = mp.mpf(0)
        self.first_nan = -1
        self.means, self.covs, self.nells = np.empty((self.T, d)), np.empty((self.T, d, d)), np.empty(self.T)
        self.trace = []

    def step(self, t, ok, mp_, Pp, pred, S, C):
        """Closes step t: the update if `ok` (and S and y are legal), NaN from here on otherwise."""
        d, y = self.d, self.ys[t]
        ok = ok and self.first_nan < 0 and _s_ok(S) and _finite(y)
        if ok:
            K = [C[k] / S for k in range(d)]
            r = y - pred
            self.m = [mp_[k] + K[k] * r for k in range(d)]
            self.P = [[Pp[i][j] - K[i] * K[j] * S for j in range(d)] for i in range(d)]
            self.nell += (r * r / S + mp.log(2 * mp.pi * S)) / 2
            self.means[t] = [float(v) for v in self.m]
            self.covs[t] = [[float(v) for v in row] for row in self.P]
            self.nells[t] = float(self.nell)
            self.trace.append((list(self.m), [list(row) for row in self.P], self.nell))
        else:
            self.trace.append(None)
            if self.first_nan < 0:
                self.first_nan = t
            self.means[t], self.covs[t], self.nells[t] = np.nan, np.nan, np.nan

    @property
    def dead(self):
        return self.first_nan >= 0

    def result(self):
        return Exact(self.means, self.covs, self.nells, self.first_nan, self.trace)


def _points(d, P):
    """-> (ok, map from a standard point (e_0[, e_1]) to its offset from the mean)."""
    if d == 1:
        if not _pivot_ok(P[0][0]):
            return False, None
        sd = mp.sqrt(P[0][0])
        return True, lambda e: [sd * e[0]]
    ok, l00, l10, l11 = _chol2(P[0][0], P[1][0], P[1][1])
    if not ok:
        return False, None
    return True, lambda e: [l00 * e[0], l10 * e[0] + l11 * e[1]]


def _transition(model, table, x):
    """(mu (d,), S (d, d)) at x."""
    if model.d == 1:
        mu, var, _ = trans1_mp(table, model.umap, _f(model.cx), x[0])
        return [mu], [[var]]
    mu, (s00, s01, s11) = trans2_mp(table, x[0], x[1])
    return mu, [[s00, s01], [s01, s11]]


def sigma_point_mp(model, xi, w, m0, P0, ys) -> Exact:
    """MFS_GF_SIGMA_POINT for one replicate.  xi (n, d), w (n,): doubles or mpf."""
    mp.mp.dps = DPS
    d = model.d
    table = _mp_table(model)
    xi = [[_f(v) for v in np.atleast_1d(row)] for row in np.asarray(xi, dtype=object).reshape(-1, d)]
    w = [_f(v) for v in np.asarray(w, dtype=object).reshape(-1)]
    run = _Run(model, m0, P0, ys)
    c = run.c
    for t in range(run.T):
        if run.dead:
            run.step(t, False, None, None, None, None, None)
            continue
        ok, off = _points(d, run.P)
        if not ok:
            run.step(t, False, None, None, None, None, None)
            continue
        mus, Ss = [], []
        for e in xi:
            o = off(e)
            mu, S = _transition(model, table, [run.m[k] + o[k] for k in range(d)])
            mus.append(mu)
            Ss.append(S)
        mp_ = [mp.fsum(wi * mu[k] for wi, mu in zip(w, mus)) for k in range(d)]
        Pp = [[mp.fsum(wi * (mu[i] * mu[j] + S[i][j]) for wi, mu, S in zip(w, mus, Ss)) - mp_[i] * mp_[j] for j in range(d)]
              for i in range(d)]
        ok, off = _points(d, Pp)
        if not ok:
            run.step(t, False, None, None, None, None, None)
            continue
        chis, hs, Xis = [], [], []
        for e in xi:
            o = off(e)
            chi = [mp_[k] + o[k] for k in range(d)]
            h, Xi, _ = measure_mp(run.kind, run.l, chi[c])
            chis.append(chi)
            hs.append(h)
            Xis.append(Xi)
        pred = mp.fsum(wi * h for wi, h in zip(w, hs))
        S = mp.fsum(wi * (h * h + Xi) for wi, h, Xi in zip(w, hs, Xis)) - pred * pred
        C = [mp.fsum(wi * chi[k] * h for wi, chi, h in zip(w, chis, hs)) - mp_[k] * pred for k in range(d)]
        run.step(t, True, mp_, Pp, pred, S, C)
    return run.result()


def ekf_mp(model, m0, P0, ys) -> Exact:
    """MFS_GF_EKF for one replicate."""
    mp.mp.dps = DPS
    d = model.d
    table = _mp_table(model)
    run = _Run(model, m0, P0, ys)
    c = run.c
    for t in range(run.T):
        if run.dead or not all(_finite(v) for v in run.m) or not all(_finite(v) for row in run.P for v in row):
            run.step(t, False, None, None, None, None, None)
            continue
        mp_, Sig = _transition(model, table, run.m)
        if d == 1:
            F = [[trans1_mp(table, model.umap, _f(model.cx), run.m[0])[2]]]
        else:
            F = jac2_mp(table, run.m[0], run.m[1])
        FP = [[mp.fsum(F[i][k] * run.P[k][j] for k in range(d)) for j in range(d)] for i in range(d)]
        Pp = [[mp.fsum(FP[i][k] * F[j][k] for k in range(d)) + Sig[i][j] for j in range(d)] for i in range(d)]
        h, Xi, dh = measure_mp(run.kind, run.l, mp_[c])
        run.step(t, True, mp_, Pp, h, dh * dh * Pp[c][c] + Xi, [Pp[k][c] * dh for k in range(d)])
    return run.result()


# ---- the closed-form assumed-density filter: polynomials in the standard Normal (z_0, z_1) as {(a, b): coefficient}
def _padd(p, q):
    out = dict(p)
    for k, v in q.items():
        out[k] = out.get(k, 0) + v
    return out


def _pmul(p, q):
    out = {}
    for (a, b), u in p.items():
        for (c, e), v in q.items():
            out[a + c, b + e] = out.get((a + c, b + e), 0) + u * v
    return out


def _psubst1(c, x):
    """sum_j c[j] x^j for a polynomial x."""
    acc = {}
    for v in reversed(c):
        acc = _padd(_pmul(acc, x), {(0, 0): v})
    return acc


def _psubst2(c, x0, x1):
    acc = {}
    for row in reversed(c):
        acc = _padd(_pmul(acc, x0), _psubst1(row, x1))
    return acc


def _normal_moment(k):
    return mp.mpf(0) if k % 2 else (mp.fac2(k - 1) if k else mp.mpf(1))


def _expect(p):
    return mp.fsum(v * _normal_moment(a) * _normal_moment(b) for (a, b), v in p.items())


def adf_closed_form(model, m0, P0, ys) -> Exact:
    """The moment-matching (assumed-density) filter in closed form: identity u-map and the Gaussian kind."""
    mp.mp.dps = DPS
    assert model.umap == 'x' and model.kind == 'gaussian', 'the closed form needs polynomials in x and a linear measurement'
    d = model.d
    table = _mp_table(model)
    if d == 1:
        table = [list(table[0]) + [mp.mpf(0)] * max(0, 2 - len(table[0])), table[1]]
        table[0][1] += _f(model.cx)
    run = _Run(model, m0, P0, ys)
    c = run.c
    l0, l1, l2 = run.l[:3]
    for t in range(run.T):
        if run.dead:
            run.step(t, False, None, None, None, None, None)
            continue
        ok, off = _points(d, run.P)
        if not ok:
            run.step(t, False, None, None, None, None, None)
            continue
        # x = m + L z as polynomials in z
        basis = [[mp.mpf(1), mp.mpf(0)], [mp.mpf(0), mp.mpf(1)]]
        cols = [off(e[:d]) for e in basis[:d]]
        x = [{(0, 0): run.m[k], **{((1, 0) if j == 0 else (0, 1)): cols[j][k] for j in range(d)}} for k in range(d)]
        if d == 1:
            mu, S = [_psubst1(table[0], x[0])], [[_psubst1(table[1], x[0])]]
        else:
            v = [_psubst2(blk, x[0], x[1]) for blk in table]
            mu, S = v[:2], [[v[2], v[3]], [v[3], v[4]]]
        mp_ = [_expect(p) for p in mu]
        Pp = [[_expect(_padd(_pmul(mu[i], mu[j]), S[i][j])) - mp_[i] * mp_[j] for j in range(d)] for i in range(d)]
        ok, _ = _points(d, Pp)
        run.step(t, ok, mp_, Pp, l0 * mp_[c] + l1, l0 * l0 * Pp[c][c] + l2, [Pp[k][c] * l0 for k in range(d)])
    return run.result()


def kalman_mp(F, c, Q, H, l1, R, m0, P0, ys) -> Exact:
    """The Kalman filter of x' = c + F x + N(0, Q), y = H x + l1 + N(0, R), in matrices; no NaN rule (the model is regular)."""
    mp.mp.dps = DPS
    d = len(c)
    toM = lambda a, r, k: mp.matrix([[_f(v) for v in row] for row in np.asarray(a, dtype=object).reshape(r, k)])   # noqa: E731
    F, Q, H, c = toM(F, d, d), toM(Q, d, d), toM(H, 1, d), toM(c, d, 1)
    m, P = toM(m0, d, 1), toM(P0, d, d)
    l1, R = _f(l1), _f(R)
    ys = [_f(v) for v in np.asarray(ys).reshape(-1)]
    T = len(ys)
    means, covs, nells, nell, trace = np.empty((T, d)), np.empty((T, d, d)), np.empty(T), mp.mpf(0), []
    for t, y in enumerate(ys):
        m, P = c + F * m, F * P * F.T + Q
        S = (H * P * H.T)[0, 0] + R
        K = P * H.T / S
        r = y - (H * m)[0, 0] - l1
        m, P = m + K * r, P - K * K.T * S
        nell += (r * r / S + mp.log(2 * mp.pi * S)) / 2
        means[t], covs[t], nells[t] = [float(v) for v in m], [[float(P[i, j]) for j in range(d)] for i in range(d)], float(nell)
        trace.append(([m[i] for i in range(d)], [[P[i, j] for j in range(d)] for i in range(d)], nell))
    return Exact(means, covs, nells, -1, trace)


def trace_distance(a: Exact, b: Exact):
    """The largest difference between two runs before rounding, over means, covariance entries and running nells."""
    worst = mp.mpf(0)
    for u, v in zip(a.trace, b.trace):
        assert (u is None) == (v is None)
        if u is None:
            continue
        diffs = [x - y for x, y in zip(u[0], v[0])] + [x - y for ru, rv in zip(u[1], v[1]) for x, y in zip(ru, rv)] + [u[2] - v[2]]
        worst = max(worst, max(abs(x) for x in diffs))
    return worst


def gauss_hermite_mp(d, order):
    """The Gauss--Hermite rule of N(0, I) in the working precision (Golub--Welsch on the Jacobi matrix), in the point order of
    SigmaPoints.gauss_hermite: the last dimension fastest.  -> (xi list of d-lists, w list)."""
    mp.mp.dps = DPS
    J = mp.zeros(order)
    for k in range(1, order):
        J[k - 1, k] = J[k, k - 1] = mp.sqrt(k)
    E, V = mp.eigsy(J)
    x1, w1 = [E[k] for k in range(order)], [V[0, k] ** 2 for k in range(order)]
    if d == 1:
        return [[x] for x in x1], w1
    return [[x1[i], x1[j]] for i in range(order) for j in range(order)], [w1[i] * w1[j] for i in range(order) for j in range(order)]


# =====================================================================================================================
# The cases.  Everything below builds plain arrays from fixed seeds; nothing calls the device.
# =====================================================================================================================
R_DEFAULT, T_DEFAULT = 3, 24


class Case(NamedTuple):
    name: str
    model: Model
    method: str                  # SIGMA_POINT or EKF: what the device runs
    xi: Optional[np.ndarray]     # (n, d) / None for the EKF
    w: Optional[np.ndarray]
    m0: np.ndarray               # (d,) shared (init_batched = 0) or (R, d)
    P0: np.ndarray               # (d, d) or (R, d, d); only the lower triangle counts
    ys: np.ndarray               # (R, T)
    arbiter: str = ''            # SIGMA_POINT, EKF or ADF; '' = the method
    guarded: bool = True         # held to assert_well_conditioned (saturation and point masses are not)

    @property
    def R(self):
        return self.ys.shape[0]

    @property
    def n_points(self):
        return 0 if self.xi is None else self.w.shape[0]

    def initial(self, r):
        return (self.m0[r] if self.m0.ndim == 2 else self.m0), (self.P0[r] if self.P0.ndim == 3 else self.P0)


def arbiter_of(case, r) -> Exact:
    model = case.model.replicate(r)
    m0, P0 = case.initial(r)
    which = case.arbiter or case.method
    if which == ADF:
        return adf_closed_form(model, m0, P0, case.ys[r])
    if which == EKF:
        return ekf_mp(model, m0, P0, case.ys[r])
    return sigma_point_mp(model, case.xi, case.w, m0, P0, case.ys[r])


# ---- rules
def _gh(d, order):
    from mfs_amd.classical_filters_smoothers import SigmaPoints
    s = SigmaPoints.gauss_hermite(d, order)
    return np.ascontiguousarray(s.xi), np.ascontiguousarray(s.w)


def _cub(d):
    from mfs_amd.classical_filters_smoothers import SigmaPoints
    s = SigmaPoints.cubature(d)
    return np.ascontiguousarray(s.xi), np.ascontiguousarray(s.w)


def _rolled(rule, k):
    """The same rule with its points in another order: point i becomes point i + k."""
    return np.ascontiguousarray(np.roll(rule[0], k, axis=0)), np.ascontiguousarray(np.roll(rule[1], k))


def ring_rule(n, w0=0.25):
    """A d = 2 rule of n >= 4 points that need not be good, only legal: a centre of weight w0 and n - 1 points of equal weight
    on a circle whose radius makes the second moment I (n - 1 >= 3 points at equal angles have sum x x^T = (n - 1) r^2 / 2 I)."""
    k = n - 1
    ang = 2. * math.pi * (np.arange(k) + 0.25) / k
    r = math.sqrt(2. / (1. - w0))
    xi = np.concatenate([np.zeros((1, 2)), r * np.stack([np.cos(ang), np.sin(ang)], axis=-1)])
    return np.ascontiguousarray(xi), np.concatenate([[w0], np.full(k, (1. - w0) / k)])


def pair_rule():
    """Two points of a d = 2 state: +-(1, 1).  Their second moment is singular; the transition covariance keeps Pp regular."""
    return np.array([[1., 1.], [-1., -1.]]), np.array([0.5, 0.5])


def cub_centre_rule(w0=1. / 3.):
    """Cubature plus a weighted centre: five points."""
    s = math.sqrt(2. / (1. - w0))
    xi = np.concatenate([np.zeros((1, 2)), s * np.eye(2), -s * np.eye(2)])
    return np.ascontiguousarray(xi), np.concatenate([[w0], np.full(4, (1. - w0) / 4.)])


# ---- likelihood parameters and measurements
_LIK = {
    ('bernoulli_logistic', 1): [0.3], ('bernoulli_logistic', 2): [0.2, 0.9], ('bernoulli_logistic', 3): [0.1, 0.8, -0.15],
    ('bernoulli_logistic', 4): [-0.2, 0.7, 0.1, 0.12], ('poisson_softplus', 1): [1.3], ('gaussian', 3): [0.9, 0.1, 0.4],
}


def _lik(kind, n_lik=None, R=None, rng=None):
    n_lik = n_lik or {'bernoulli_logistic': 4, 'poisson_softplus': 1, 'gaussian': 3}[kind]
    base = np.array(_LIK[kind, n_lik])
    if R is None:
        return base
    return np.ascontiguousarray(base * (1. + 0.2 * rng.uniform(-1., 1., (R, n_lik))))


def _ys(kind, R, T, rng, centre=0.):
    if kind == 'bernoulli_logistic':
        return (rng.random((R, T)) < 0.5).astype(np.float64)
    if kind == 'poisson_softplus':
        return rng.poisson(1., (R, T)).astype(np.float64)
    return centre + 0.6 * rng.standard_normal((R, T))


def _rng(name):
    return np.random.default_rng([20261021] + list(name.encode()))


# ---- d = 1 tables
def _table1(degree, rng, scale, top=0.15):
    """mean and variance of the given degree with every coefficient nonzero, in powers of u / scale so that the polynomial
    stays O(1) for |u| <= scale: mean = 0.1 + (small) ..., var = 0.3 + (small) ..."""
    J1 = degree + 1
    j = np.arange(J1)
    sign = np.where(rng.random((2, J1)) < 0.5, -1., 1.)
    amp = sign * rng.uniform(0.5, 1., (2, J1)) * top / np.maximum(j, 1)
    amp[0, 0], amp[1, 0] = 0.1, 0.3
    amp[1, 1:] *= 0.3
    if degree >= 1:
        amp[0, 1] = abs(amp[0, 1])
    return np.ascontiguousarray(amp / scale ** j)


def case_1d(name, degree, umap, kind, method, rule=None, n_lik=None, coef_batched=False, lik_batched=False, cx=0.55,
            T=T_DEFAULT, R=R_DEFAULT, arbiter='', scale=None, table=None, seed=None):
    rng = _rng(seed or name)      # cases that share a seed share everything but the rule
    scale = scale or (1. if umap == 'tanh' else 3.)
    if table is not None:
        coef = np.array(table, dtype=np.float64)
    elif coef_batched:
        coef = np.stack([_table1(degree, rng, scale) for _ in range(R)])
    else:
        coef = _table1(degree, rng, scale)
    lik = _lik(kind, n_lik, R if lik_batched else None, rng)
    model = Model(1, coef, kind, lik, umap, cx if degree > 0 or table is not None else 0., 0)
    xi, w = (None, None) if method == EKF else rule
    m0 = 0.1 * rng.standard_normal((R, 1))
    P0 = 0.4 * (1. + 0.25 * rng.random((R, 1, 1)))
    return Case(name, model, method, xi, w, m0, P0, _ys(kind, R, T, rng, 0.2), arbiter)


# the cubic mean / quadratic variance of the closed-form ADF cases, identity map
ADF1_TABLE = [[0.1, 0.75, 0.05, -0.04], [0.25, 0.03, 0.05, 0.]]


# ---- d = 2 tables
def _table2(extent, rng, scale=3.):
    """(5, D, D) with every entry nonzero: mu_k = a contraction plus small terms of every degree, S = a constant positive
    definite matrix plus small terms, in powers of x / scale."""
    D = extent
    a, b = np.meshgrid(np.arange(D), np.arange(D), indexing='ij')
    sign = np.where(rng.random((5, D, D)) < 0.5, -1., 1.)
    amp = sign * rng.uniform(0.5, 1., (5, D, D)) * 0.12 / np.maximum(a + b, 1)
    amp[2:] *= 0.25
    amp[:, 0, 0] = [0.15, -0.1, 0.2, 0.05, 0.25]
    if D > 1:
        amp[0, 1, 0], amp[0, 0, 1], amp[1, 1, 0], amp[1, 0, 1] = 0.8 * scale, 0.12 * scale, -0.1 * scale, 0.7 * scale
    return np.ascontiguousarray(amp / scale ** (a + b))


LINEAR_F = np.array([[0.9, 0.15], [-0.1, 0.8]])
LINEAR_C = np.array([0.05, -0.02])
LINEAR_Q = np.array([[0.2, 0.06], [0.06, 0.15]])
LINEAR_LIK = np.array([0.9, 0.1, 0.4])


def linear_table2():
    coef = np.zeros((5, 2, 2))
    for k in range(2):
        coef[k, 0, 0], coef[k, 1, 0], coef[k, 0, 1] = LINEAR_C[k], LINEAR_F[k, 0], LINEAR_F[k, 1]
    coef[2, 0, 0], coef[3, 0, 0], coef[4, 0, 0] = LINEAR_Q[0, 0], LINEAR_Q[0, 1], LINEAR_Q[1, 1]
    return coef


def case_2d(name, extent, kind, component, method, rule=None, lik_batched=False, T=T_DEFAULT, R=R_DEFAULT, arbiter='',
            table=None, init_batched=True, asymmetric=False, P0=None, guarded=True, seed=None):
    rng = _rng(seed or name)
    coef = np.array(table, dtype=np.float64) if table is not None else _table2(extent, rng)
    lik = _lik(kind, None, R if lik_batched else None, rng)
    model = Model(2, coef, kind, lik, 'x', 0., component)
    xi, w = (None, None) if method == EKF else rule
    lead = (R,) if init_batched else ()
    m0 = np.array([0.3, -0.2]) + 0.1 * rng.standard_normal(lead + (2,))
    if P0 is None:
        a, b = 0.4 * (1. + 0.25 * rng.random(lead)), 0.3 * (1. + 0.25 * rng.random(lead))
        c = 0.1 * rng.uniform(-1., 1., lead)
        P0 = np.stack([np.stack([a, np.full(lead, 99.) if asymmetric else c], -1), np.stack([c, b], -1)], -2)
    return Case(name, model, method, xi, w, m0, np.ascontiguousarray(P0), _ys(kind, R, T, rng, 0.2), arbiter, guarded)


def _cases():
    out = []
    add = out.append
    # -- C.2 closed-form ADF: every rule of sufficient order against the same closed form
    for n in (4, 5, 8, 12, 33, 65):
        add(case_1d(f'adf1/gh{n}', 3, 'x', 'gaussian', SIGMA_POINT, _gh(1, n), arbiter=ADF, table=ADF1_TABLE, cx=0., seed='adf1'))
    # the same 65 points with the centre node last: the one point of the second round then carries weight 0.1, not 1e-28
    add(case_1d('adf1/gh65-centre-last', 3, 'x', 'gaussian', SIGMA_POINT, _rolled(_gh(1, 65), 32), arbiter=ADF, table=ADF1_TABLE,
                cx=0., seed='adf1'))
    adf2 = _table2(4, _rng('adf2'))
    # x_1 = m_1 + l10 z_0 + l11 z_1 carries z_0 too, so what a rule has to integrate is the TOTAL degree: means of total degree
    # 3 and covariances of total degree 2 (S_01 not constant) make an integrand of degree 6 in z_0
    total = np.add.outer(np.arange(4), np.arange(4))
    adf2[:2, total > 3] = 0.
    adf2[2:, total > 2] = 0.
    for order in (4, 5, 8):
        add(case_2d(f'adf2/gh{order}', 4, 'gaussian', 1, SIGMA_POINT, _gh(2, order), arbiter=ADF, table=adf2, seed='adf2'))
    # 81 points, the second round of 17 holding the centre of the rule
    add(case_2d('adf2/gh9-centre-last', 4, 'gaussian', 1, SIGMA_POINT, _rolled(_gh(2, 9), 32), arbiter=ADF, table=adf2, seed='adf2'))
    # -- C.3 every lane group at both dimensions
    for n in (1, 2, 3, 5, 7, 11, 17, 25, 33, 64):
        add(case_1d(f'lanes1/n{n}', 3, 'tanh', 'bernoulli_logistic', SIGMA_POINT, _gh(1, n)))
    rules2 = {'n1': _gh(2, 1), 'n2': pair_rule(), 'n4': _cub(2), 'n5': cub_centre_rule(), 'n7': ring_rule(7), 'n9': _gh(2, 3),
              'n16': _gh(2, 4), 'n17': ring_rule(17), 'n25': _gh(2, 5), 'n64': _gh(2, 8)}
    for key, rule in rules2.items():
        add(case_2d(f'lanes2/{key}', 3, 'bernoulli_logistic', 0, SIGMA_POINT, rule))
    # -- C.4 the d = 2 model matrix: kind x component x method, over the extents
    extents = iter((2, 3, 5, 7, 3, 5, 7, 2, 5, 3, 2, 7))
    for kind in KINDS:
        for comp in (0, 1):
            for method in (SIGMA_POINT, EKF):
                D = next(extents)
                add(case_2d(f'matrix2/{kind}/c{comp}/{method}/D{D}', D, kind, comp, method, _gh(2, 3)))
    for method in (SIGMA_POINT, EKF):
        add(case_2d(f'matrix2/constant/{method}', 1, 'bernoulli_logistic', 1, method, _gh(2, 3)))
        add(case_2d(f'matrix2/likbatched/{method}', 3, 'bernoulli_logistic', 1, method, _gh(2, 3), lik_batched=True, R=5))
        add(case_2d(f'matrix2/sharedinit/{method}', 3, 'poisson_softplus', 0, method, _gh(2, 3), init_batched=False))
        add(case_2d(f'matrix2/asymmetric/{method}', 3, 'gaussian', 1, method, _gh(2, 3), asymmetric=True))
    # -- C.5 the d = 1 table edges
    for method, rule in ((SIGMA_POINT, _gh(1, 5)), (EKF, None)):
        add(case_1d(f'edges1/deg0/{method}', 0, 'x', 'bernoulli_logistic', method, rule))
        for umap in ('x', 'tanh'):
            add(case_1d(f'edges1/deg15/{umap}/{method}', 15, umap, 'poisson_softplus', method, rule))
        add(case_1d(f'edges1/gaussian-nonlinear/{method}', 5, 'tanh', 'gaussian', method, rule))
        for n_lik in (1, 2, 3, 4):
            add(case_1d(f'edges1/nlik{n_lik}/{method}', 3, 'tanh', 'bernoulli_logistic', method, rule, n_lik=n_lik, lik_batched=True))
    for key, (method, rule) in {'ekf': (EKF, None), 'n1': (SIGMA_POINT, _gh(1, 1)), 'n5': (SIGMA_POINT, _gh(1, 5))}.items():
        for cb, lb in ((True, False), (False, True), (True, True)):
            add(case_1d(f'edges1/batched/{key}/coef{int(cb)}lik{int(lb)}', 15 if cb and lb else 4, 'x' if cb else 'tanh',
                        'bernoulli_logistic', method, rule, n_lik=3, coef_batched=cb, lik_batched=lb))
    # -- C.7 saturation: the outer points of the 256-point rule reach |q| = |x|^3 / 5 of several thousand, |l0 x| of hundreds
    sat = [[0.05, 0.8, 0., -0.02], [0.5, 0., 0.02, 0.]]
    for method, rule in ((SIGMA_POINT, _gh(1, 256)), (EKF, None)):
        for kind, lik in (('bernoulli_logistic', [0., 0., 0., 0.2]), ('poisson_softplus', [10.])):
            c = case_1d(f'saturation/{kind}/{method}', 3, 'x', kind, method, rule, table=sat, cx=0., T=8, R=2)
            add(c._replace(model=c.model._replace(lik=np.array(lik)), guarded=False))
    # -- C.8 point masses at d = 2: diag(v, 0) is legal; diag(0, v) and 0 divide by the zero first pivot
    pm = np.array([[[0.3, 0.], [0., 0.]], [[0., 0.], [0., 0.3]], [[0., 0.], [0., 0.]]])
    for method in (SIGMA_POINT, EKF):
        add(case_2d(f'pointmass2/{method}', 3, 'bernoulli_logistic', 0, method, _gh(2, 3), P0=pm, T=12, guarded=False))
    return out


_CASES = None


def cases():
    """The one list of cases: the generator, the host test and the GPU test share it."""
    global _CASES
    if _CASES is None:
        _CASES = _cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def case(name):
    return next(c for c in cases() if c.name == name)


FRESHNESS_CASES = ('lanes2/n2', 'edges1/deg0/ekf')      # cheap, and their rules are not the output of an eigenvalue solver


# ---- the restatement (tests/gaussian_filters_ref.py) on a case: host tables from the arrays
def host_tables(model, R=None):
    """The host description the Python layer would hold: TransitionTables (d = 1) or GaussianTablesND (d = 2), and the
    likelihood factor.  A (R', ...) table or parameter array is tiled to R replicates (R' must divide into it cyclically)."""
    from mfs_amd import sym
    from mfs_amd.tme_poly import TransitionTables
    from mfs_amd.tme_poly_nd import GaussianTablesND, PolyND

    def tile(a, nd):
        if a.ndim == nd or R is None:
            return a
        return np.ascontiguousarray(a[np.arange(R) % a.shape[0]])
    coef, lik = tile(model.coef, 2 if model.d == 1 else 3), tile(model.lik, 1)
    factor = sym.LikelihoodSpec(model.kind, lik, model.component)
    if model.d == 1:
        umap = model.umap
        return TransitionTables('gaussian', umap, [], model.cx, sym.Poly(coef[..., 0, :], umap), sym.Poly(coef[..., 1, :], umap),
                                'envelope'), factor
    p = [PolyND(blk) for blk in coef]
    return GaussianTablesND(2, p[:2], [[p[2], p[3]], [p[3], p[4]]], 'envelope'), factor


def restatement_of(case, r):
    from mfs_amd.classical_filters_smoothers import SigmaPoints
    from tests import gaussian_filters_ref as G
    tables, factor = host_tables(case.model.replicate(r))
    sgps = None if case.method == EKF else SigmaPoints(case.model.d, case.n_points, case.w, None, case.xi)
    m0, P0 = case.initial(r)
    return G.gaussian_filter_ref(tables, factor, G.EKF if case.method == EKF else G.SIGMA_POINT, sgps, m0, P0, case.ys[r])


# ---- the fixture
FIXTURE = 'gaussian_filters_exact.npz'
_INPUTS = ('coef', 'lik', 'xi', 'w', 'm0', 'P0', 'ys')
_OUTPUTS = ('means', 'covs', 'nells', 'first_nan')


def freeze(case):
    """Everything the fixture holds of one case: {key: array}."""
    out = {f'{case.name}:coef': case.model.coef, f'{case.name}:lik': case.model.lik, f'{case.name}:m0': case.m0,
           f'{case.name}:P0': case.P0, f'{case.name}:ys': case.ys}
    if case.xi is not None:
        out[f'{case.name}:xi'], out[f'{case.name}:w'] = case.xi, case.w
    for tag, run in (('exact', arbiter_of), ('ref', restatement_of)):
        res = [run(case, r) for r in range(case.R)]
        for q in _OUTPUTS[:3]:
            out[f'{case.name}:{tag}_{q}'] = np.stack([getattr(x, q) for x in res])
        out[f'{case.name}:{tag}_first_nan'] = np.array([x.first_nan for x in res], dtype=np.int32)
    return out


def thaw(npz, case):
    """The case with the stored inputs in place of the rebuilt ones (the stored doubles are what the arbiter saw), and the
    stored arbiter and restatement outputs: (case, exact, ref), each of the last two a dict of (R, ...) arrays."""
    get = lambda k: npz[f'{case.name}:{k}']      # noqa: E731
    sp = case.xi is not None
    stored = case._replace(model=case.model._replace(coef=get('coef'), lik=get('lik')), xi=get('xi') if sp else None,
                           w=get('w') if sp else None, m0=get('m0'), P0=get('P0'), ys=get('ys'))
    return stored, {q: get(f'exact_{q}') for q in _OUTPUTS}, {q: get(f'ref_{q}') for q in _OUTPUTS}


# ---- the sharp bar.  REF_SPREAD: the largest error of the fp64 restatement against the arbiter over every case of the fixture,
# in units of the hard bound (1e-9 (|mean| + sd) on means and covariance entries, 1e-9 relative on the running nells), measured
# on the CPU by tests/test_host_gaussian_filters.py::test_restatement_against_the_arbiter -- never from the device.
# Measured on the stored restatement outputs of the 82 cases: means 1.899e-06 (adf2/gh8), covs 1.011e-06 (adf2/gh9-centre-last),
# nells 6.533e-07 (edges1/nlik1/sigma_point) -- that is, 2e-15 (|mean| + sd): a few ulp.
REF_SPREAD = {'means': 1.90e-6, 'covs': 1.02e-6, 'nells': 6.54e-7}
SHARP_FACTOR = 8.
