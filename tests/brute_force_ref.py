"""Yardstick of the grid-filter tests: a NumPy restatement of the Chapman branch of the reference's brute_force_filter
(mfs/classical_filters_smoothers/brute_force.py:66-136), batched over replicates, and the exact Kalman filter of the
reference's own analytic pin (tests/test_classical_filters_smoothers.py:128-191).  A plain helper module, not a conftest.

The restatement is stepwise, as the reference is: `integration_steps` products with the one-sub-step matrix per
measurement, then the update with the weights of np.trapz.  tests/test_host_brute_force.py pins it against the Kalman filter.
"""
import math

import numpy as np

from mfs_amd.one_dim.moments import _trace_sde
from mfs_amd.tme_poly import euler_tables, tme_tables


trapz = getattr(np, 'trapezoid', None) or np.trapz   # NumPy 2 renamed it


def trapz_weights(xs):
    """w with np.trapz(f, xs) == w @ f: half the distance between a point's neighbours."""
    w = np.empty_like(xs)
    w[0], w[-1] = 0.5 * (xs[1] - xs[0]), 0.5 * (xs[-1] - xs[-2])
    w[1:-1] = 0.5 * (xs[2:] - xs[:-2])
    return w


def transition_mean_sd(drift, dispersion, xs, ddt, pred_method):
    a, b = _trace_sde(drift, dispersion)
    tables = euler_tables(a, b, ddt) if pred_method == 'chapman-euler' \
        else tme_tables(a, b, ddt, int(pred_method.split('-')[-1]), gaussian=True)
    return np.broadcast_to(tables.cond_mean(xs), xs.shape), np.sqrt(np.broadcast_to(tables.cond_var(xs), xs.shape))


def brute_force_ref(drift, dispersion, pdf_of, init_ps, xs, ys, dt, integration_steps=1, pred_method='chapman-tme-2'):
    """pdf_of(b) -> the callable (y, x) -> p(y | x) of replicate b, evaluated numerically on the grid.
    init_ps (n,) or (B, n), ys (B, T).  Returns pdfs (B, T, n), means, variances (B, T), nell (B,), first_nan (B,).
    A replicate whose normaliser is zero or not finite is NaN from that step on."""
    xs = np.asarray(xs, dtype=np.float64)
    ys = np.asarray(ys, dtype=np.float64)
    B, T = ys.shape
    n = xs.shape[0]
    m, s = transition_mean_sd(drift, dispersion, xs, dt / integration_steps, pred_method)
    w = trapz_weights(xs)
    # K[i][j] = norm.pdf(x_i; m_j, s_j) w_j  (brute_force.py:86: trapz(norm.pdf(x, m, scale) * ps, xs))
    K = np.exp(-0.5 * ((xs[:, None] - m[None, :]) / s[None, :]) ** 2) / (math.sqrt(2 * math.pi) * s[None, :]) * w[None, :]
    ps = np.broadcast_to(np.asarray(init_ps, dtype=np.float64), (B, n)).copy()
    pdfs = np.empty((B, T, n))
    means, variances = np.empty((B, T)), np.empty((B, T))
    nell, first_nan = np.zeros(B), np.full(B, -1, dtype=np.int32)
    pdf_fns = [pdf_of(b) for b in range(B)]
    with np.errstate(all='ignore'):
        for t in range(T):
            for _ in range(integration_steps):
                ps = ps @ K.T
            for b in range(B):
                l = np.asarray(pdf_fns[b](ys[b, t], xs), dtype=np.float64) * ps[b]
                z = w @ l
                if not (np.isfinite(z) and z > 0.):
                    ps[b] = np.nan
                    nell[b] = np.nan
                    if first_nan[b] < 0:
                        first_nan[b] = t
                else:
                    ps[b] = l / z
                    nell[b] -= math.log(z)
                means[b, t] = w @ (xs * ps[b])
                variances[b, t] = w @ ((xs - means[b, t]) ** 2 * ps[b])
            pdfs[:, t] = ps
    return pdfs, means, variances, nell, first_nan


# ---- the Ornstein--Uhlenbeck / Gaussian setting of the reference's TestBruteForce, and its exact Kalman filter -------------
OU_ELL, OU_SIGMA, OU_DT, OU_R = 1., 0.5, 1e-2, 0.1


def ou_drift(x):
    return -1 / OU_ELL * x


def ou_dispersion(_):
    return math.sqrt(2) * OU_SIGMA / math.sqrt(OU_ELL)


def ou_data(T, rng, dt=OU_DT):
    """Measurements along an exact OU path started in the stationary law."""
    F, Sigma = math.exp(-dt / OU_ELL), OU_SIGMA ** 2 * (1 - math.exp(-2 * dt / OU_ELL))
    x = OU_SIGMA * rng.standard_normal()
    traj = np.empty(T)
    for k in range(T):
        x = F * x + math.sqrt(Sigma) * rng.standard_normal()
        traj[k] = x
    return traj + math.sqrt(OU_R) * rng.standard_normal(T)


def kalman(ys, dt=OU_DT, mean0=0., var0=OU_SIGMA ** 2):
    """Exact filtering means, variances and negative log-likelihood (test_classical_filters_smoothers.py:163-179)."""
    F, Sigma = math.exp(-dt / OU_ELL), OU_SIGMA ** 2 * (1 - math.exp(-2 * dt / OU_ELL))
    mf, vf, nell = mean0, var0, 0.
    mfs, vfs = [], []
    for y in ys:
        mp, vp = F * mf, F * vf * F + Sigma
        s = vp + OU_R
        k = vp / s
        mf, vf = mp + k * (y - mp), vp - vp * k
        nell += 0.5 * math.log(2 * math.pi * s) + 0.5 * (y - mp) ** 2 / s
        mfs.append(mf)
        vfs.append(vf)
    return np.array(mfs), np.array(vfs), nell


def kalman_setting():
    """xs = linspace(-5, 5, 1000), T = 100, integration_steps = 20, ys from default_rng(0)."""
    xs = np.linspace(-5., 5., 1000)
    init_ps = np.exp(-0.5 * xs ** 2 / OU_SIGMA ** 2) / math.sqrt(2 * math.pi * OU_SIGMA ** 2)
    ys = ou_data(100, np.random.default_rng(0))
    return xs, init_ps, ys, 20


def assert_pdfs_close(dev, ref, rtol=1e-9, floor=1e-12):
    """rtol on every entry above floor x its row's maximum, atol = floor x the row maximum below that; both NaN agrees."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape
    nan_d, nan_r = np.isnan(dev), np.isnan(ref)
    assert np.array_equal(nan_d, nan_r), 'NaN patterns differ'
    rmax = np.max(np.where(nan_r, 0., ref), axis=-1, keepdims=True)
    with np.errstate(invalid='ignore'):
        err = np.abs(dev - ref)
        ok = np.where(ref > floor * rmax, err <= rtol * np.abs(ref), err <= floor * rmax) | nan_r
        rel = np.where((ref > floor * rmax) & ~nan_r, err / np.where(ref > 0, ref, 1.), 0.)
    assert ok.all(), f'{(~ok).sum()} of {ok.size} pdf entries differ; worst relative error {rel.max():.3e}'
    return float(rel.max())
