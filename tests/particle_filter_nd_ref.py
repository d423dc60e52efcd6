"""Yardstick of the d = 2 particle-filter tests: a NumPy restatement of the reference's bootstrap_filter
(mfs/classical_filters_smoothers/smc.py:62-84) as dardel/prey_predator/pf.py runs it -- the proposal m(x) + chol(S(x)) z per
particle, stratified / systematic resampling -- on the random stream that include/mfs_hip.h states for mfs_particle_filter_nd.
A plain helper module, not a conftest.  tests/test_host_particle_filter_nd.py pins it against the exact Kalman filter below.

The stream, the margin bound and the comparison are those of tests/particle_filter_ref.py.  The transition is evaluated through
the traced tables (`GaussianTablesND.mean`, `.cov`), the Cholesky factor by the closed form l00 = sqrt(s00), l10 = s01 / l00,
l11 = sqrt(s11 - l10^2) (a negative or non-finite pivot makes the particle NaN, as jnp.linalg.cholesky does), the likelihood
numerically from the Python callable, called as pdf(y, x) with x of shape (2, n) so that x[k] is component k of every particle,
and y the step's measurement (a scalar for one column, (ny,) otherwise).
"""
import math

import numpy as np

from mfs_amd import stats
from mfs_amd.utils import GaussianSumND
from tests.particle_filter_ref import draws, margin_bound, assert_close, philox4x32_10   # noqa: F401  (re-exported)


def chol2(s00, s01, s11):
    """-> (l00, l10, l11, ok): the closed-form lower factor; ok where both pivots are >= 0 and finite."""
    with np.errstate(all='ignore'):
        l00 = np.sqrt(s00)
        l10 = s01 / l00
        d1 = s11 - l10 * l10
        l11 = np.sqrt(d1)
        ok = (s00 >= 0.) & np.isfinite(s00) & (d1 >= 0.) & np.isfinite(d1)
    return l00, l10, l11, ok


def initial_particles(init, seed, n):
    """(n, 2): tag 0, draws 0 and 1 the normals, draw 2 the component uniform."""
    idx = np.arange(n)
    if isinstance(init, GaussianSumND):
        _, z0 = draws(seed, idx, 0, 0, 0)
        _, z1 = draws(seed, idx, 0, 0, 1)
        uc, _ = draws(seed, idx, 0, 0, 2)
        cumw = np.cumsum(init.weights)
        c = np.minimum((cumw[None, :] <= uc[:, None]).sum(axis=1), cumw.shape[0] - 1)
        l00, l10, l11, _ = chol2(init.covs[:, 0, 0], init.covs[:, 1, 0], init.covs[:, 1, 1])
        return np.stack([init.means[c, 0] + l00[c] * z0, init.means[c, 1] + l10[c] * z0 + l11[c] * z1], axis=-1)
    return np.array(init, dtype=np.float64).reshape(n, 2)


def particle_filter_nd_ref(trans_of, pdf_of, ys, init_of, seeds, n, resampling='stratified'):
    """trans_of(b) -> the GaussianTransitionND of replicate b, pdf_of(b) -> its callable (y, x) -> p(y | x), init_of(b) -> a
    GaussianSumND or (n, 2) particles.  ys (B, T) or (B, T, ny), seeds (B,).
    Returns samples (B, T, n, 2), means (B, T, 2), covs (B, T, 2, 2), nell (B,), first_nan (B,), margin (float)."""
    ys = np.asarray(ys, dtype=np.float64)
    B, T = ys.shape[:2]
    idx_all = np.arange(n)
    samples = np.empty((B, T, n, 2))
    means, covs = np.empty((B, T, 2)), np.empty((B, T, 2, 2))
    nell, first_nan = np.zeros(B), np.full(B, -1, dtype=np.int32)
    margin = math.inf
    with np.errstate(all='ignore'):
        for b in range(B):
            tables, pdf, seed = trans_of(b).tables, pdf_of(b), int(seeds[b])
            x = initial_particles(init_of(b), seed, n)
            for t in range(T):
                _, z0 = draws(seed, idx_all, t, 1, 0)
                _, z1 = draws(seed, idx_all, t, 1, 1)
                shape = (n,)
                mu0, mu1 = (np.broadcast_to(tables.mean[k](x), shape) for k in range(2))
                s00, s01, s11 = (np.broadcast_to(tables.cov[i][j](x), shape) for i, j in ((0, 0), (0, 1), (1, 1)))
                l00, l10, l11, ok = chol2(s00, s01, s11)
                x = np.stack([np.where(ok, mu0 + l00 * z0, np.nan), np.where(ok, mu1 + l10 * z0 + l11 * z1, np.nan)], axis=-1)
                w = np.broadcast_to(np.asarray(pdf(ys[b, t], x.T), dtype=np.float64), shape)
                s = w.sum()
                if not (np.isfinite(s) and s > 0.):
                    x = np.full((n, 2), np.nan)
                    nell[b] = np.nan
                    if first_nan[b] < 0:
                        first_nan[b] = t
                else:
                    nell[b] -= math.log(np.mean(w))
                    cs = np.cumsum(w / s)
                    u, _ = draws(seed, idx_all if resampling == 'stratified' else 0, t, 2, 0)
                    v = (np.arange(n, dtype=np.float64) + u) / n
                    j = np.searchsorted(cs, v)
                    right = np.abs(cs[np.minimum(j, n - 1)] - v)
                    left = np.where(j > 0, np.abs(v - cs[np.maximum(j - 1, 0)]), np.inf)
                    margin = min(margin, float(np.min(np.minimum(left, right))))
                    x = x[np.clip(j, 0, n - 1)]
                samples[b, t] = x
                means[b, t] = np.mean(x, axis=0)
                d = x - means[b, t]
                covs[b, t] = d.T @ d / n
    return samples, means, covs, nell, first_nan, margin


def kalman_2d(F, Q, H, R, m0, P0, ys):
    """The exact filter of x' = F x + N(0, Q), y = H x + N(0, R), started from N(m0, P0) BEFORE the first transition (the
    particle filter propagates, then weighs).  ys (T, ny).  Returns means (T, 2), covs (T, 2, 2), nell."""
    F, Q, H, R = (np.asarray(a, dtype=np.float64) for a in (F, Q, H, R))
    m, P = np.asarray(m0, dtype=np.float64), np.asarray(P0, dtype=np.float64)
    ms, Ps, nell = [], [], 0.
    for y in np.asarray(ys, dtype=np.float64):
        m, P = F @ m, F @ P @ F.T + Q
        S = H @ P @ H.T + R
        r = y - H @ m
        K = np.linalg.solve(S, H @ P).T
        nell += 0.5 * (r @ np.linalg.solve(S, r) + math.log(np.linalg.det(2. * math.pi * S)))
        m, P = m + K @ r, P - K @ S @ K.T
        ms.append(m)
        Ps.append(P)
    return np.array(ms), np.array(Ps), nell


# ---- the linear-Gaussian model both test files pin against: dx = A x dt + G dW, y_k ~ N(x_k, 0.5^2), x_0 ~ N(0, 0.25 I)
LIN_A = np.array([[-0.5, 0.3], [-0.2, -0.8]])
LIN_G = np.array([[0.5, 0.], [0.1, 0.4]])
LIN_DT, LIN_SD, LIN_P0 = 0.1, 0.5, 0.25
# what tests/test_host_particle_filter_nd.py::test_restatement_against_the_kalman_filter measured with n = 10 000 particles and
# eight seeds (its docstring): the worst |mean error| / sqrt(P_kk / n) and the worst |nell error|.  The tests assert twice these.
LIN_R, LIN_NELL_ERR = 5.81, 0.138


def lin_drift(x):
    return np.array([LIN_A[0, 0] * x[0] + LIN_A[0, 1] * x[1], LIN_A[1, 0] * x[0] + LIN_A[1, 1] * x[1]])


def lin_dispersion(x):
    return LIN_G


def lin_pdf(y, x):
    return stats.norm_pdf(y[0], x[0], LIN_SD) * stats.norm_pdf(y[1], x[1], LIN_SD)


def lin_init():
    return GaussianSumND.new([[0., 0.]], [LIN_P0 * np.eye(2)], [1.], ((0, 0), (0, 1), (1, 0)))


def lin_kalman_matrices(tables):
    """F, Q of the (linear, constant) tables, read off by evaluation."""
    o, e0, e1 = np.zeros(2), np.array([1., 0.]), np.array([0., 1.])
    mean = lambda p: np.array([float(tables.mean[k](p)) for k in range(2)])   # noqa: E731
    F = np.stack([mean(e0) - mean(o), mean(e1) - mean(o)], axis=1)
    Q = np.array([[float(tables.cov[i][j](o)) for j in range(2)] for i in range(2)])
    return F, Q


def lin_data(T, rng, F, Q):
    """A path of the model and its measurements (T, 2)."""
    x = math.sqrt(LIN_P0) * rng.standard_normal(2)
    Lq = np.linalg.cholesky(Q)
    ys = np.empty((T, 2))
    for t in range(T):
        x = F @ x + Lq @ rng.standard_normal(2)
        ys[t] = x + LIN_SD * rng.standard_normal(2)
    return ys
