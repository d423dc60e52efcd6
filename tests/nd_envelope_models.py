"""The d = 2 models of the envelope tests of filternd_kernel (tests/test_gpu_nd_envelope.py, tests/test_host_nd.py): drift and
dispersion as callables on a sequence of the two state variables, which oracle/tme_sympy.py takes as they are and the host
traces through nd_support.host_drift / host_disp.  What does not depend on the dimension is in tests/nd_support.py.

  lv2    two-species competitive Lotka--Volterra, dx_i = x_i (r_i - sum_j A_ij x_j) dt + sigma_i x_i dW_i with r = A 1, dt = 0.05:
         every order of the TME table weighs 10 .. 1000 times the parity bar (TME-1 vs TME-2: 1.5e-4 .. 4.5e-4 in NLL, TME-2 vs
         TME-3: 1.4e-5 .. 4.1e-5), where prey--predator at dt = 1e-3 hides the |kappa| = 5, 6 rows below 1e-9.
  lin2   linear drift, constant dispersion, two broad Gaussian factors: the model whose raw-moment Gram matrices stay
         well-conditioned up to N = 7.
  well2  coupled double well (cubic drift): blocks of unequal extent per variable; TME-1 has extent 4, TME-2 extent 7 and TME-3
         extent 10, which the device refuses; its Euler closure has a cubic mean.

  cv2    the SDE of the bearing-only example; bearing_only_model() is the example itself, discretised exactly.

A likelihood is a factor spec (nd_support.factor_pdfs).  Measurements of a replicate come from its own seeded
Euler--Maruyama path, 10 sub-steps per dt."""
import functools
import math
from typing import Callable, NamedTuple

import numpy as np
import scipy.linalg
import sympy as sp

from mfs_amd.multi_dims import moments, ss_models
from oracle import multi_dims as omd, tme_sympy
from tests.nd_support import all_finite, factor_pdfs, host_disp, host_drift, initial, run_oracle, tables

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


@functools.lru_cache(maxsize=None)
def host_family(model, fam, N):
    """-> (the five device closures, their signature) of a transition family of MODELS[model]."""
    m = MODELS[model]
    mi, _ = tables(2, N)
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
    mi, _ = tables(2, N)
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


# ---- prey--predator (BASELINE config 5), for the N-D tests that live among the 1-D files -----------------------------------------
class PreyPredator(NamedTuple):
    mi: np.ndarray
    inds: tuple
    dt: float
    gs: object             # the device's initial law (.cms, .mean); ogs: the oracle's
    fns: tuple             # the five device closures of the family, of signature sig
    sig: str
    pmf: Callable
    ogs: object
    opmf: Callable


@functools.lru_cache(maxsize=None)
def prey_predator(N, family='tme_2'):
    """The device's prey--predator model on tables(2, N) with the closures of 'tme_2' or 'tme_normal_2', and the oracle's
    initial law and likelihood; shared, not to be written to."""
    mi, inds = tables(2, N)
    dt, _, _, gs, drift, disp, _, pmf, _ = ss_models.prey_predator(mi)
    _, _, ogs, _, _, _, opmf = omd.prey_predator(mi)
    if family == 'tme_2':
        fns, sig = moments.sde_cond_moments_tme(drift, disp, dt, 2), 'multi-index'
    else:
        fns, sig = moments.sde_cond_moments_tme_normal(drift, disp, dt, 2, mi), 'index'
    return PreyPredator(mi, inds, dt, gs, fns, sig, pmf, ogs, opmf)


@functools.lru_cache(maxsize=None)
def prey_predator_oracle(N, family='tme_2'):
    """-> (cms, mean): the oracle's closures of the same family by SymPy differentiation (seconds for 'tme_2')."""
    mi, _ = tables(2, N)
    dt, _, _, odrift, odisp, _, _ = omd.prey_predator(mi)
    derive = tme_sympy.sde_cond_moments_tme_nd if family == 'tme_2' else tme_sympy.sde_cond_moments_normal_nd
    return derive(odrift, odisp, 2, dt, 2, mi)[1:3]


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


def bearing_only_model():
    """The reference's examples/2d_bearing_only.ipynb, cells 3-7: constant-velocity LTI model discretised exactly, Gaussian-sum
    start, y_k = atan2(x_1, x_0) + sqrt(0.1) noise."""
    dt, T, xi = 0.01, 100, 0.1
    A = np.array([[0., 1.], [0., 0.]])
    Bm = np.array([[0., 0.], [0., 1.]])
    # discretise_lti_sde (mfs/utils.py, Van Loan / Axelsson & Gustafsson 2015): F = expm(A dt), Q = int_0^dt e^{As} B B^T e^{A^T s} ds
    blk = scipy.linalg.expm(np.block([[A, Bm @ Bm.T], [np.zeros((2, 2)), -A.T]]) * dt)
    F = blk[:2, :2]
    Q = blk[:2, 2:] @ F.T
    means0 = np.array([[1., 0.], [1., 1.]])
    covs0 = np.array([np.eye(2), np.eye(2)]) * 0.01
    weights0 = np.array([0.7, 0.3])
    rng = np.random.default_rng(999)
    comp = rng.choice(2, p=weights0)
    x = means0[comp] + 0.1 * rng.standard_normal(2)
    cq = np.linalg.cholesky(Q)
    ys = np.empty(T)
    for k in range(T):
        x = F @ x + cq @ rng.standard_normal(2)
        ys[k] = np.arctan2(x[1], x[0]) + math.sqrt(xi) * rng.standard_normal()
    return dt, T, xi, F, Q, means0, covs0, weights0, ys


def raw_means(rms):
    """E[x_0], E[x_1] of a raw-moment table (graded-lex: (0, 1) at 1, (1, 0) at 2)."""
    return np.stack([rms[..., 2], rms[..., 1]], axis=-1)


@functools.lru_cache(maxsize=None)
def oracle_case(model, fam, N, mode, T, seed, b=0, spec=None, stable=False):
    """The oracle's run of replicate b of measurements(model, b + 1, T, seed, spec), from the model's initial law, cached."""
    m = MODELS[model]
    mi, inds = tables(2, N)
    spec = m.spec if spec is None else spec
    ys = measurements(model, b + 1, T, seed, spec)[b]
    sig = 'multi-index' if fam in OPERATOR else 'index'
    return run_oracle(mode, oracle_family(model, fam, N), sig, factor_pdfs(spec)[1], ys, mi, inds,
                      initial(mi, m.mean0, m.cov0), stable)


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
