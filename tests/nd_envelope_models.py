"""Three d = 2 models for the envelope tests of filternd_kernel (tests/test_gpu_nd_envelope.py, tests/test_host_nd.py), each in
a host form traced by mfs_amd.multi_dims.moments and an oracle form for oracle/tme_sympy.py + oracle/multi_dims.py.

  lv2    two-species competitive Lotka--Volterra, dx_i = x_i (r_i - sum_j A_ij x_j) dt + sigma_i x_i dW_i with r = A 1, dt = 0.05:
         every order of the TME table weighs 10 .. 1000 times the parity bar (TME-1 vs TME-2: 1.5e-4 .. 4.5e-4 in NLL, TME-2 vs
         TME-3: 1.4e-5 .. 4.1e-5), where prey--predator at dt = 1e-3 hides the |kappa| = 5, 6 rows below 1e-9.
  lin2   linear drift, constant dispersion, two broad Gaussian factors: the model whose raw-moment Gram matrices stay
         well-conditioned up to N = 7.
  well2  coupled double well (cubic drift): blocks of unequal extent per variable; TME-1 has extent 4, TME-2 extent 7 and TME-3
         extent 10, which the device refuses; its Euler closure has a cubic mean.

A likelihood is a list of factors (kind, component, y-column, parameter): 'gaussian' N(y; x, p^2), 'poisson' with rate
softplus(p x), 'bernoulli' with probability logistic(p x - 1).  Measurements of a replicate come from its own seeded
Euler--Maruyama path, 10 sub-steps per dt."""
import functools
import math
from typing import Callable, NamedTuple

import numpy as np
import sympy as sp

from mfs_amd import stats, sym
from mfs_amd.multi_dims import moments
from mfs_amd.multi_dims.multi_indices import generate_graded_lexico_multi_indices, gram_and_hankel_indices_graded_lexico
from oracle import models as om, multi_dims as omd, tme_sympy

MODES = ('raw', 'central', 'scaled')
OPERATOR = ('tme_1', 'tme_2', 'tme_3')
NORMAL = ('tme_normal_2', 'tme_normal_3', 'euler')

LV_A = np.array([[0.8, 0.3], [0.2, 0.6]])
LV_SIG = np.array([0.1, 0.15])
LIN_A = np.array([[-1., 0.6], [-0.4, -0.7]])


class Model(NamedTuple):
    dt: float
    drift: Callable        # x: a sequence of the two state variables (polynomial variables, SymPy symbols or floats) -> [a_0, a_1]
    disp: Callable         # -> 2 x 2 nested lists
    mean0: np.ndarray
    cov0: np.ndarray
    spec: tuple            # the model's own likelihood factors


def lv2(A=LV_A, sig=LV_SIG, dt=0.05):
    A, sig = np.asarray(A, dtype=float), np.asarray(sig, dtype=float)
    r = A.sum(axis=1)

    def drift(x):
        return [x[i] * (float(r[i]) - float(A[i, 0]) * x[0] - float(A[i, 1]) * x[1]) for i in range(2)]

    def disp(x):
        return [[float(sig[0]) * x[0], 0.], [0., float(sig[1]) * x[1]]]
    return Model(dt, drift, disp, np.array([1.0, 0.9]), np.array([[0.02, 0.005], [0.005, 0.03]]),
                 (('gaussian', 0, 0, 0.2), ('poisson', 1, 1, 1.0)))


def reverse(m: Model) -> Model:
    """The same model with x_0 and x_1 exchanged throughout: drift, dispersion, initial law, factors and y columns."""
    def drift(x):
        a = m.drift([x[1], x[0]])
        return [a[1], a[0]]

    def disp(x):
        b = m.disp([x[1], x[0]])
        return [[b[1][1], b[1][0]], [b[0][1], b[0][0]]]
    return Model(m.dt, drift, disp, m.mean0[::-1].copy(), m.cov0[::-1, ::-1].copy(),
                 tuple((kind, 1 - j, 1 - c, p) for kind, j, c, p in m.spec))


def _lin_drift(x):
    return [float(LIN_A[i, 0]) * x[0] + float(LIN_A[i, 1]) * x[1] for i in range(2)]


def _well_drift(x):
    return [x[0] - x[0] ** 3 + 0.4 * x[1], -1.0 * x[1] + 0.4 * x[0]]


# batch_closures points of test group f: three (A, sigma)
LV_BATCH = [(LV_A, LV_SIG), (LV_A * 1.25, LV_SIG * 0.6), (LV_A[::-1, ::-1] * 0.9, LV_SIG * 1.5)]

MODELS = {
    'lv2': lv2(),
    'lv2_rev': reverse(lv2()),
    'lin2': Model(0.1, _lin_drift, lambda x: [[0.8, 0.], [0., 0.8]], np.array([0.3, -0.2]), np.array([[1., 0.2], [0.2, 0.8]]),
                  (('gaussian', 0, 0, 1.5), ('gaussian', 1, 1, 2.0))),
    'well2': Model(0.05, _well_drift, lambda x: [[0.5, 0.], [0., 0.5]], np.array([0.8, 0.3]),
                   np.array([[0.05, 0.01], [0.01, 0.08]]), (('gaussian', 0, 0, 0.5), ('poisson', 1, 1, 1.0))),
}
# the SDE of the bearing-only example (constant velocity, noise on the velocity); its tests bring their own initial law
MODELS['cv2'] = Model(0.01, lambda x: [1.0 * x[1], 0.0 * x[0]], lambda x: [[0., 0.], [0., 1.]], None, None, ())
MODELS.update({f'lv2_b{b}': lv2(A, s) for b, (A, s) in enumerate(LV_BATCH)})


def host_drift(m):
    return lambda x: np.array(m.drift(x), dtype=object)


def host_disp(m):
    return lambda x: np.array(m.disp(x), dtype=object)


@functools.lru_cache(maxsize=None)
def tables(N):
    return generate_graded_lexico_multi_indices(2, 2 * N - 1), gram_and_hankel_indices_graded_lexico(N, 2)


def initial(mi, mean, cov):
    """Raw, central and scaled moments of N(mean, cov) on the table, with the mean and the scales."""
    mean, cov = np.asarray(mean, dtype=float), np.asarray(cov, dtype=float)
    rms = np.array([omd.raw_moments_mvn_kan(mean, cov, n) for n in mi])
    cms = np.array([omd.raw_moments_mvn_kan(np.zeros(2), cov, n) for n in mi])
    scale = np.sqrt(np.diag(cov))
    return {'rms': rms, 'cms': cms, 'scms': cms / np.prod(scale ** mi, axis=-1), 'mean': mean, 'scale': scale}


@functools.lru_cache(maxsize=None)
def host_family(model, fam, N):
    """-> (the five device closures, their signature) of a transition family of MODELS[model]."""
    m = MODELS[model]
    mi, _ = tables(N)
    if fam in OPERATOR:
        return moments.sde_cond_moments_tme(host_drift(m), host_disp(m), m.dt, int(fam[-1])), 'multi-index'
    if fam == 'euler':
        return moments.sde_cond_moments_euler_maruyama(host_drift(m), host_disp(m), m.dt, mi), 'index'
    return moments.sde_cond_moments_tme_normal(host_drift(m), host_disp(m), m.dt, int(fam[-1]), mi), 'index'


@functools.lru_cache(maxsize=None)
def sympy_family(model, fam, N):
    """The oracle's closures (rms, cms, scms, mean, mean_var) of the same family by SymPy differentiation (oracle/tme_sympy.py);
    the mean-and-variance closure of a Normal family from tme_sympy.mean_and_cov_expr itself."""
    m = MODELS[model]
    mi, _ = tables(N)
    if fam in OPERATOR and N < 4 and model in ('lv2', 'lin2', 'well2'):
        return sympy_family(model, fam, 4)      # 'multi-index' closures look a moment up by its multi-index: one table serves
    if fam in OPERATOR:
        orms, ocms, omean, omean_var = tme_sympy.sde_cond_moments_tme_nd(m.drift, m.disp, 2, m.dt, int(fam[-1]), mi)
        sel = lambda idx: np.asarray(idx)                                   # noqa: E731
    else:
        order = 'euler' if fam == 'euler' else int(fam[-1])
        orms, ocms, omean = tme_sympy.sde_cond_moments_normal_nd(m.drift, m.disp, 2, m.dt, order, mi)
        xs = sp.symbols('x0:2', real=True)
        gam = sp.Matrix(m.disp(list(xs)))
        gam = gam * gam.T
        cov_e = gam * sp.Float(m.dt) if fam == 'euler' else \
            tme_sympy.mean_and_cov_expr(xs, [sp.sympify(e) for e in m.drift(list(xs))], gam, m.dt, order)[1]
        var_f = [tme_sympy._lambdify(tuple(xs), cov_e[i, i]) for i in range(2)]

        def omean_var(x):
            x = np.asarray(x, dtype=np.float64)
            return omean(x), np.stack([f(x[..., 0], x[..., 1]) for f in var_f], axis=-1)
        sel = lambda idx: mi[np.asarray(idx)]                               # noqa: E731

    def oscms(x, idx, mean, scale):
        return ocms(x, idx, mean) / np.prod(np.asarray(scale) ** sel(idx), axis=-1)
    return orms, ocms, oscms, omean, omean_var


def oracle_family(model, fam, N):
    """The closures the oracle filter runs: SymPy tables for N <= 4; for N = 5..7 the host's NumPy closures, which
    tests/test_host_nd.py pins to SymPy at the multi-indices of N = 3, 4 (SymPy costs 10 .. 40 s per table at those orders)."""
    return sympy_family(model, fam, N) if N <= 4 else host_family(model, fam, N)[0]


# ---- likelihoods ----
def _factor(kind, y, xk, p, dev):
    if kind == 'gaussian':
        return stats.norm_pdf(y, xk, p) if dev else om.norm_pdf(y, xk, p)
    if kind == 'poisson':
        return stats.poisson_pmf(y, sym.log(1. + sym.exp(xk * p))) if dev else om.poisson_pmf(y, np.log1p(np.exp(xk * p)))
    return (stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-(xk * p) + 1.))) if dev else
            om.bernoulli_pmf(y, 1. / (1. + np.exp(-(xk * p) + 1.))))


def factor_pdfs(spec):
    """-> (device pdf, oracle pdf): the product of the factors of `spec` in that order; y is indexed by column."""
    def pdf(y, x):
        return math.prod(_factor(kind, y[c], x[j], p, True) for kind, j, c, p in spec)

    def opdf(y, x):
        return float(math.prod(_factor(kind, y[c], x[j], p, False) for kind, j, c, p in spec))
    return pdf, opdf


def path(m, T, seed):
    """One Euler--Maruyama path of the model on 10 sub-steps per dt from a draw of the initial law -> ((T, 2), generator)."""
    rng = np.random.default_rng(seed)
    x = m.mean0 + np.linalg.cholesky(m.cov0) @ rng.standard_normal(2)
    h = m.dt / 10
    xs = np.empty((T, 2))
    for t in range(T):
        for _ in range(10):
            a = np.array([float(v) for v in m.drift(x)])
            b = np.array([[float(v) for v in row] for row in m.disp(x)])
            x = x + a * h + b @ rng.standard_normal(2) * math.sqrt(h)
        xs[t] = x
    return xs, rng


def measurements(model, B, T, seed, spec=None):
    """(B, T, ny): replicate b measures its own path, seeded (seed, b), through the factors of `spec` (the model's own by
    default).  Two factors that read one column share that column's draw: the first one's."""
    m = MODELS[model]
    spec = m.spec if spec is None else spec
    ys = np.zeros((B, T, max(c for _, _, c, _ in spec) + 1))
    for b in range(B):
        xs, rng = path(m, T, [seed, b])
        done = set()
        for kind, j, c, p in spec:
            x = xs[:, j]
            if kind == 'gaussian':
                y = x + p * rng.standard_normal(T)
            elif kind == 'poisson':
                y = rng.poisson(np.log1p(np.exp(x * p))).astype(float)
            else:
                y = (rng.random(T) < 1. / (1. + np.exp(-(x * p) + 1.))).astype(float)
            if c not in done:
                ys[b, :, c] = y
                done.add(c)
    return ys


# ---- the oracle filter ----
def run_oracle(mode, ofns, sig, opdf, ys, N, st, stable=False):
    """oracle/multi_dims.py on one replicate (T, ny) -> dict(m, mean, scale, nell); raw mode reports its means as the
    first-order raw moments."""
    mi, inds = tables(N)
    mp = (mi, inds)
    if mode == 'raw':
        m, nell = omd.moment_filter_nd_rms((ofns[0], sig), opdf, ys, mp, st['rms'], stable)
        return {'m': m, 'nell': nell}
    if mode == 'central':
        m, mean, nell = omd.moment_filter_nd_cms((ofns[1], sig), ofns[3], opdf, ys, mp, st['cms'], st['mean'], stable)
        return {'m': m, 'mean': mean, 'nell': nell}
    m, mean, scale, nell = omd.moment_filter_nd_scms((ofns[2], sig), ofns[4], opdf, ys, mp, st['scms'], st['mean'], st['scale'],
                                                     stable)
    return {'m': m, 'mean': mean, 'scale': scale, 'nell': nell}


def raw_means(rms):
    """E[x_0], E[x_1] of a raw-moment table (graded-lex: (0, 1) at 1, (1, 0) at 2)."""
    return np.stack([rms[..., 2], rms[..., 1]], axis=-1)


def all_finite(r):
    return bool(np.isfinite(r['nell']) and all(np.all(np.isfinite(r[k])) for k in ('m', 'mean', 'scale') if k in r))


@functools.lru_cache(maxsize=None)
def oracle_case(model, fam, N, mode, T, seed, b=0, spec=None, stable=False):
    """The oracle's run of replicate b of measurements(model, b + 1, T, seed, spec), from the model's initial law, cached."""
    m = MODELS[model]
    mi, _ = tables(N)
    spec = m.spec if spec is None else spec
    ys = measurements(model, b + 1, T, seed, spec)[b]
    sig = 'multi-index' if fam in OPERATOR else 'index'
    return run_oracle(mode, oracle_family(model, fam, N), sig, factor_pdfs(spec)[1], ys, N, initial(mi, m.mean0, m.cov0), stable)


def admissible(model, fam, N, mode, T, seed, b=0, spec=None):
    """The admission condition of a case, on the oracle alone: every output finite, and for a raw case the oracle's raw NLL
    and means within 1e-8 of its central ones -- 100 times inside the parity bar, so that two correct fp64 implementations
    cannot differ by 1e-6 through the conditioning of the raw Gram matrices alone.  -> (ok, what was measured)."""
    r = oracle_case(model, fam, N, mode, T, seed, b, spec)
    if not all_finite(r):
        return False, 'the oracle is not finite'
    if mode != 'raw':
        return True, 'finite'
    c = oracle_case(model, fam, N, 'central', T, seed, b, spec)
    if not all_finite(c):
        return False, 'the central oracle is not finite'
    gap = max(abs(r['nell'] - c['nell']) / abs(c['nell']), float(np.max(np.abs(raw_means(r['m']) - c['mean']) / np.abs(c['mean']))))
    return gap <= 1e-8, f'raw vs central oracle {gap:.1e}'
