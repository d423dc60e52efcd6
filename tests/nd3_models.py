"""The d = 3 models of the N-D tests (tests/test_gpu_nd3*.py, tests/test_gpu_fuzz_nd3.py, tests/test_host_nd3.py) and of the
long-horizon fixture (tests/golden/make_nd3_golden.py), with their constants, path generators and measurement generators.

  lorenz  Lorenz-63 in units of 10 (x = X / 10), dispersion 0.1 I, y = x_0 + N(0, SD^2), a scalar
  lv      3-species competitive Lotka--Volterra, dx_i = x_i (r_i - sum_j A_ij x_j) dt + sigma_i x_i dW_i with r = A 1 (so that
          (1, 1, 1) is the equilibrium): a Gaussian factor on x_0 (column 0) and a Poisson-softplus factor on x_2 (column 1)
  ou      3-D Ornstein--Uhlenbeck with a Poisson-softplus factor on x_1

Drift and dispersion are callables on a sequence of the three state variables (polynomial variables, SymPy symbols or floats):
the oracle takes them as they are, the host traces them through nd_support.host_drift / host_disp."""
import functools
import math
from typing import Callable, NamedTuple

import numpy as np

from mfs_amd import stats, sym
from mfs_amd.multi_dims import moments
from oracle import models as om, tme_sympy
from tests.nd_support import host_disp, host_drift, tables

# ---- Lorenz-63 ----
DT = 0.01
SIG, RHO, BETA = 10., 28., 8. / 3.
M0 = np.array([0.1, 0.1, 2.4])
C0 = np.diag([0.01, 0.01, 0.01])
SD = 0.5


def lorenz_drift(x):
    return [SIG * (x[1] - x[0]), x[0] * (RHO - 10. * x[2]) - x[1], 10. * x[0] * x[1] - BETA * x[2]]


def lorenz_disp(x):
    return [[0.1, 0., 0.], [0., 0.1, 0.], [0., 0., 0.1]]


def lorenz_pdf(y, x):
    return stats.norm_pdf(y, x[0], SD)


def lorenz_opdf(y, x):
    return float(om.norm_pdf(y, x[0], SD))


def _lorenz_substeps(x, h, rng):
    """Ten Euler--Maruyama steps of length h on the states x (B, 3)."""
    for _ in range(10):
        a = np.stack(lorenz_drift(x.T), axis=-1)
        x = x + a * h + 0.1 * math.sqrt(h) * rng.standard_normal(x.shape)
    return x


def lorenz_ys(B, T, seed, sd=SD):
    """(B, T): x_0 + N(0, sd^2) along Euler--Maruyama paths on 10 sub-steps per DT, the noise drawn step by step."""
    rng = np.random.default_rng(seed)
    x = M0 + 0.1 * rng.standard_normal((B, 3))
    ys = np.empty((B, T))
    for t in range(T):
        x = _lorenz_substeps(x, DT / 10, rng)
        ys[:, t] = x[:, 0] + sd * rng.standard_normal(B)
    return ys


def lorenz_path(B, T, seed):
    """Euler--Maruyama states on 10 sub-steps per DT, (B, T, 3), and the generator for the measurement noise."""
    rng = np.random.default_rng(seed)
    x = M0 + 0.1 * rng.standard_normal((B, 3))
    xs = np.empty((B, T, 3))
    for t in range(T):
        x = xs[:, t] = _lorenz_substeps(x, DT / 10, rng)
    return xs, rng


# ---- 3-species Lotka--Volterra ----
LV_A = np.array([[0.8, 0.3, 0.1], [0.2, 0.6, 0.1], [0.4, 0.2, 0.9]])
LV_SIG = np.array([0.1, 0.15, 0.2])
LV_DT = 0.05
LV_M0 = np.array([1.0, 0.9, 1.1])
LV_C0 = np.array([[0.02, 0.005, 0.], [0.005, 0.03, -0.004], [0., -0.004, 0.025]])
LV_SD = 0.2


def lv_drift(x, A=LV_A):
    r = A.sum(axis=1)
    return [x[i] * (float(r[i]) - sum(float(A[i, j]) * x[j] for j in range(3))) for i in range(3)]


def lv_disp(x, sig=LV_SIG):
    return [[float(sig[i]) * x[i] if i == j else 0. for j in range(3)] for i in range(3)]


def lv_path(B, T, seed, A=LV_A, sig=LV_SIG):
    """Euler--Maruyama states on 10 sub-steps per dt, (B, T, 3), and the generator for the measurement noise."""
    rng = np.random.default_rng(seed)
    r = A.sum(axis=1)
    x = LV_M0 + 0.1 * rng.standard_normal((B, 3))
    h = LV_DT / 10
    xs = np.empty((B, T, 3))
    for t in range(T):
        for _ in range(10):
            x = np.abs(x + x * (r - x @ A.T) * h + sig * x * math.sqrt(h) * rng.standard_normal((B, 3)))
        xs[:, t] = x
    return xs, rng


def lv_pdf(y, x):
    return stats.norm_pdf(y[0], x[0], LV_SD) * stats.poisson_pmf(y[1], sym.log(1. + sym.exp(x[2])))


def lv_opdf(y, x):
    return float(om.norm_pdf(y[0], x[0], LV_SD) * om.poisson_pmf(y[1], np.log1p(np.exp(x[2]))))


def lv_ys(B, T, seed, A=LV_A, sig=LV_SIG):
    """(B, T, 2): x_0 + N(0, LV_SD^2) and Poisson(softplus(x_2)) counts."""
    xs, rng = lv_path(B, T, seed, A, sig)
    return np.stack([xs[..., 0] + LV_SD * rng.standard_normal((B, T)),
                     rng.poisson(np.log1p(np.exp(xs[..., 2]))).astype(np.float64)], axis=-1)


# ---- 3-D OU ----
OU_A = np.array([[-1., 0.3, 0.], [0., -0.8, 0.4], [0.2, 0., -0.6]])


def ou_drift(x):
    return [sum(float(OU_A[i, j]) * x[j] for j in range(3)) for i in range(3)]


def ou_disp(x):
    return [[0.3, 0., 0.], [0., 0.3, 0.], [0., 0., 0.3]]


class Model(NamedTuple):
    dt: float
    drift: Callable      # x: a sequence of the three state variables -> [a_0, a_1, a_2]
    disp: Callable       # -> 3 x 3 nested lists
    mean0: np.ndarray
    cov0: np.ndarray
    pdf: Callable        # the device's likelihood, traced
    opdf: Callable       # the oracle's, on numbers
    ys: Callable         # (B, T, seed) -> measurements


def lv_model(A=LV_A, sig=LV_SIG):
    return Model(LV_DT, lambda x: lv_drift(x, A), lambda x: lv_disp(x, sig), LV_M0, LV_C0, lv_pdf, lv_opdf,
                 lambda B, T, seed: lv_ys(B, T, seed, A, sig))


MODELS = {
    'lorenz': Model(DT, lorenz_drift, lorenz_disp, M0, C0, lorenz_pdf, lorenz_opdf, lorenz_ys),
    'lv': lv_model(),
    'ou': Model(0.1, ou_drift, ou_disp, np.array([1., 1.5, 0.5]), np.diag([0.1, 0.1, 0.1]),
                lambda y, x: stats.poisson_pmf(y, sym.log(1. + sym.exp(x[1]))),
                lambda y, x: float(om.poisson_pmf(y, np.log1p(np.exp(x[1])))),
                lambda B, T, seed: np.random.default_rng(seed).poisson(1.5, size=(B, T)).astype(np.float64)),
}


@functools.lru_cache(maxsize=None)
def family(model, fam, N):
    """-> (device closures, signature, oracle closures (rms, cms, scms, mean, mean_var)) of a transition family: SymPy tables
    for the operator families; for the Normal closures the host's vectorised Stein closure, which tests/test_host_nd3.py
    pins to the oracle's per-node Kan moments."""
    m = MODELS[model]
    mi, _ = tables(3, N)
    drift, disp = host_drift(m), host_disp(m)
    if fam in ('tme_1', 'tme_2'):
        order = int(fam[-1])
        fns = moments.sde_cond_moments_tme(drift, disp, m.dt, order, d=3)
        orms, ocms, omean, omean_var = tme_sympy.sde_cond_moments_tme_nd(m.drift, m.disp, 3, m.dt, order, mi)

        def oscms(x, idx, mean, scale):
            return ocms(x, idx, mean) / np.prod(np.asarray(scale) ** np.asarray(idx), axis=-1)
        return fns, 'multi-index', (orms, ocms, oscms, omean, omean_var)
    if fam == 'euler':
        fns = moments.sde_cond_moments_euler_maruyama(drift, disp, m.dt, mi)
    else:
        fns = moments.sde_cond_moments_tme_normal(drift, disp, m.dt, int(fam[-1]), mi)
    return fns, 'index', fns
