"""Yardstick of the Gaussian-filter tests: a NumPy restatement of the sigma-point filter and of the extended Kalman filter for
d = 1, 2 and a scalar measurement, written from the equations of include/mfs_hip.h (mfs_gaussian_filter_1d), on the host tables
of the transition (`cond_mean`, the variance / covariance polynomials, `Poly.dx`, `PolyND.diff`).  One replicate per call.  A
plain helper module, not a conftest.

Beside the filter outputs it reports what decides how far two correct implementations in fp64 can differ: the largest
eigenvalue ratio of the predicted to the filtered covariance (the cancellation of P = Pp - K K^T S), the smallest innovation
variance S, and whether anything was NaN.  tests/test_host_gaussian_filters.py pins it against the exact Kalman filter.
"""
import math
from typing import NamedTuple

import numpy as np

from mfs_amd.classical_filters_smoothers.gfs import MeasurementMoments

SIGMA_POINT, EKF = 'sigma_point', 'ekf'


class GaussianFilterRef(NamedTuple):
    means: np.ndarray      # (T, d)
    covs: np.ndarray       # (T, d, d)
    nells: np.ndarray      # (T,) running sum
    first_nan: int         # -1 if none
    ratio: float           # max over the steps of the largest eigenvalue of Pf^-1 Pp
    s_min: float           # min over the steps of S
    any_nan: bool


# ---- measurement moments of the likelihood kinds
def measurement(lik, x):
    """(h, Xi, dh/dx) at the scalar or array x of the state component the factor reads."""
    x = np.asarray(x, dtype=np.float64)
    p = np.asarray(lik.params, dtype=np.float64)
    with np.errstate(over='ignore'):
        if lik.kind == 'bernoulli_logistic':
            l = np.concatenate([p, np.zeros(4 - p.shape[0])])
            z = l[0] + x * (l[1] + x * (l[2] + x * l[3]))
            pr = 1. / (1. + np.exp(-z))
            var = pr * (1. - pr)
            return pr, var, var * (l[1] + x * (2. * l[2] + x * 3. * l[3]))
        if lik.kind == 'poisson_softplus':
            z = p[0] * x
            rate = np.maximum(z, 0.) + np.log1p(np.exp(-np.abs(z)))
            return rate, rate, p[0] / (1. + np.exp(-z))
        if lik.kind == 'gaussian':
            return p[0] * x + p[1], np.full(x.shape, p[2]), np.full(x.shape, p[0])
    raise ValueError(lik.kind)


# ---- transition mean, covariance and Jacobian on the host tables
def transition(tables, x):
    """x (..., d) -> (mu (..., d), Sigma (..., d, d))."""
    x = np.asarray(x, dtype=np.float64)
    if not hasattr(tables, 'cov'):     # 1-D TransitionTables
        return tables.cond_mean(x), tables.cond_var(x)[..., None]
    d = tables.d
    mu = np.stack([tables.mean[k](x) for k in range(d)], axis=-1)
    cov = np.stack([np.stack([tables.cov[i][j](x) for j in range(d)], axis=-1) for i in range(d)], axis=-2)
    return mu, cov


def transition_jacobian(tables, x):
    """d mu / d x at one point x (d,) -> (d, d)."""
    x = np.asarray(x, dtype=np.float64)
    if not hasattr(tables, 'cov'):
        return np.reshape(tables.mean_x_coef + tables.mean_poly.dx()(x[0]), (1, 1))
    d = tables.d
    return np.array([[float(tables.mean[i].diff(j)(x)) for j in range(d)] for i in range(d)])


def chol(P):
    """Lower Cholesky factor by the closed forms the step is stated with, and whether every pivot was legal (>= 0 and finite)."""
    d = P.shape[0]
    with np.errstate(all='ignore'):
        if d == 1:
            return np.sqrt(P), bool(P[0, 0] >= 0. and np.isfinite(P[0, 0]))
        l00 = np.sqrt(P[0, 0])
        l10 = P[1, 0] / l00
        d1 = P[1, 1] - l10 * l10
        ok = bool(P[0, 0] >= 0. and np.isfinite(P[0, 0]) and d1 >= 0. and np.isfinite(d1))
        return np.array([[l00, 0.], [l10, np.sqrt(d1)]]), ok


def gaussian_filter_ref(tables, lik, method, sgps, m0, v0, ys) -> GaussianFilterRef:
    """tables: TransitionTables (kind 'gaussian') or GaussianTablesND (d = 2); lik: the traced likelihood factor (or a
    MeasurementMoments); sgps: a SigmaPoints (ignored by the EKF); m0 (d,), v0 (d, d); ys (T,)."""
    d = tables.d if hasattr(tables, 'cov') else 1
    if isinstance(lik, MeasurementMoments):
        lik = lik.spec(d)
    c = int(lik.component)
    ys = np.asarray(ys, dtype=np.float64).reshape(-1)
    T = ys.shape[0]
    m, P = np.asarray(m0, dtype=np.float64).reshape(d).copy(), np.asarray(v0, dtype=np.float64).reshape(d, d).copy()
    P[np.triu_indices(d, 1)] = P.T[np.triu_indices(d, 1)]      # the lower triangle is what counts
    means, covs, nells = np.empty((T, d)), np.empty((T, d, d)), np.empty(T)
    nell, first_nan, ratio, s_min = 0., -1, 0., math.inf
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for t in range(T):
            ok = True
            if method == EKF:
                mu, Sig = transition(tables, m)
                F = transition_jacobian(tables, m)
                mp, Pp = mu, F @ P @ F.T + Sig
                h, Xi, dh = (float(v) for v in measurement(lik, mp[c]))
                pred = h
                S = dh * dh * Pp[c, c] + Xi
                C = Pp[:, c] * dh
            else:
                L, ok = chol(P)
                chi = m + sgps.xi @ L.T
                mu, Sig = transition(tables, chi)
                mp = sgps.w @ mu
                Pp = np.einsum('i,ij,ik->jk', sgps.w, mu, mu) + np.einsum('i,ijk->jk', sgps.w, Sig) - np.outer(mp, mp)
                Lp, okp = chol(Pp)
                ok = ok and okp
                chi = mp + sgps.xi @ Lp.T
                h, Xi, _ = measurement(lik, chi[:, c])
                pred = float(sgps.w @ h)
                S = float(sgps.w @ (h * h + Xi)) - pred * pred
                C = sgps.w @ (chi * h[:, None]) - mp * pred
            ok = ok and bool(np.isfinite(S) and S > 0.) and bool(np.isfinite(ys[t]))      # a measurement that is not finite poisons
            if ok:
                K = C / S
                m = mp + K * (ys[t] - pred)
                P = Pp - np.outer(K, K) * S
                nell += 0.5 * ((ys[t] - pred) ** 2 / S + math.log(2. * math.pi * S))
                s_min = min(s_min, S)
                if np.all(np.isfinite(P)) and np.all(np.isfinite(Pp)):
                    try:
                        ratio = max(ratio, float(np.max(np.real(np.linalg.eigvals(np.linalg.solve(P, Pp))))))
                    except np.linalg.LinAlgError:
                        ratio = math.inf
            else:
                m, P, nell = np.full(d, np.nan), np.full((d, d), np.nan), math.nan
                if first_nan < 0:
                    first_nan = t
            means[t], covs[t], nells[t] = m, P, nell
    any_nan = bool(np.isnan(means).any() or np.isnan(covs).any() or np.isnan(nells).any())
    return GaussianFilterRef(means, covs, nells, first_nan, ratio, s_min, any_nan)


# ---- the conditions every parity case asserts on the restatement alone, and the comparison
RATIO_MAX, S_MIN = 16., 1e-3


def assert_well_conditioned(ref: GaussianFilterRef, what):
    assert not ref.any_nan, f'{what}: the restatement is NaN (first_nan {ref.first_nan}): choose another seed'
    assert ref.ratio <= RATIO_MAX, f'{what}: eigenvalue ratio Pp / Pf {ref.ratio:.3g} > {RATIO_MAX}: choose another seed'
    assert ref.s_min >= S_MIN, f'{what}: smallest S {ref.s_min:.3g} < {S_MIN}: choose another seed'


def assert_close(dev, ref, scale, what, rtol=1e-9):
    """|dev - ref| <= rtol * scale elementwise; both NaN agrees.  Returns the worst error / bound."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape, f'{what}: shapes {dev.shape} and {ref.shape}'
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), f'{what}: NaN patterns differ'
    with np.errstate(invalid='ignore'):
        err = np.where(np.isnan(ref), 0., np.abs(dev - ref))
        bound = np.where(np.isnan(ref), 1., rtol * np.broadcast_to(scale, ref.shape))
    worst = float(np.max(err / bound)) if err.size else 0.
    assert worst <= 1., f'{what}: worst error is {worst:.3g} x the bound'
    return worst


def assert_filter_close(dev_means, dev_covs, dev_nells, ref_means, ref_covs, ref_nells, what):
    """The tolerance of the particle-filter suite: |delta| <= 1e-9 (|mean| + sd) on means and covariance entries, with
    (mean, sd) the restatement's, componentwise for the means and the largest over the components for covariance entries;
    rtol 1e-9 on nells."""
    ref_means, ref_covs = np.asarray(ref_means), np.asarray(ref_covs)
    with np.errstate(invalid='ignore'):
        sd = np.sqrt(np.diagonal(ref_covs, axis1=-2, axis2=-1))
    scale = np.abs(ref_means) + sd
    worst = {'means': assert_close(dev_means, ref_means, scale, f'{what} means'),
             'covs': assert_close(dev_covs, ref_covs, np.max(scale, axis=-1)[..., None, None], f'{what} covs'),
             'nells': assert_close(dev_nells, ref_nells, np.abs(ref_nells), f'{what} nells')}
    print(f'{what}: worst error / bound ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    return worst
