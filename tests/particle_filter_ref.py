"""Yardstick of the particle-filter tests: a NumPy restatement of the reference's bootstrap_filter
(mfs/classical_filters_smoothers/smc.py:62-84) with its stratified / systematic resamplers (resampling.py:43-59: cumsum,
searchsorted, clip), on the random stream that include/mfs_hip.h states (Philox4x32-10, counter = (particle, step, tag, draw)).
A plain helper module, not a conftest.  tests/test_host_particle_filter.py pins it against the exact Kalman filter.

The transition is evaluated through the traced tables (`cond_mean`, `cond_var`), the likelihood numerically from the Python
callable.  Besides the outputs the restatement returns the run's resampling margin: the smallest distance of any target
(i + u_i) / n to its two neighbouring entries of the cumulative weights.  Resampling is discrete, so two implementations agree
only while that margin exceeds the rounding of their prefix sums; the parity tests assert it.
"""
import functools
import math

import numpy as np

from mfs_amd import stats
from mfs_amd.classical_filters_smoothers import gaussian_transition
from mfs_amd.utils import GaussianSum1D
from tests import brute_force_ref as R

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


# ---- the linear model of the shape sweeps: the OU model of tests/brute_force_ref.py through TME-2, a Gaussian measurement
SWEEP_DT = 0.2


def gauss_pdf(y, x):
    return stats.norm_pdf(y, x, math.sqrt(R.OU_R))


@functools.lru_cache(maxsize=None)
def sweep_model():
    """-> (the transition, the initial law)."""
    return (gaussian_transition(R.ou_drift, R.ou_dispersion, SWEEP_DT, 'tme-2'),
            GaussianSum1D.new([0.], [R.OU_SIGMA ** 2], [1.]))


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays of 32-bit words held in uint64; the key is bumped after every round.  Returns r0..r3."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(a, b):
    """U(a, b) = ((a >> 6) 2^26 + (b >> 6) + 1/2) 2^-52: exact in fp64, strictly inside (0, 1)."""
    six = np.uint64(6)
    return (((a >> six) * np.uint64(1 << 26) + (b >> six)).astype(np.float64) + 0.5) * 2. ** -52


def draws(seed, i, t, tag, draw):
    """(uniform, normal) of the draws (seed, i, t, tag, draw); i may be an array."""
    seed = int(seed)
    r0, r1, r2, r3 = philox4x32_10(i, t, tag, draw, seed & 0xFFFFFFFF, seed >> 32)
    u = uniform(r0, r1)
    return u, np.sqrt(-2. * np.log(u)) * np.cos(6.283185307179586476925 * uniform(r2, r3))


def initial_particles(init, seed, n):
    idx = np.arange(n)
    if isinstance(init, GaussianSum1D):
        _, z = draws(seed, idx, 0, 0, 0)
        uc, _ = draws(seed, idx, 0, 0, 1)
        cumw = np.cumsum(init.weights)
        c = np.minimum((cumw[None, :] <= uc[:, None]).sum(axis=1), cumw.shape[0] - 1)
        return init.means[c] + np.sqrt(init.variances[c]) * z
    return np.array(init, dtype=np.float64)


def particle_filter_ref(trans_of, pdf_of, ys, init_of, seeds, n, resampling='stratified', zs=None):
    """trans_of(b) -> the GaussianTransition of replicate b, pdf_of(b) -> its callable (y, x) -> p(y | x), init_of(b) -> a
    GaussianSum1D or (n,) particles.  ys (B, T), seeds (B,).
    Returns samples (B, T, n), means, variances (B, T), cfs (B, T, nz) or None, nell (B,), first_nan (B,), margin (float)."""
    ys = np.asarray(ys, dtype=np.float64)
    B, T = ys.shape
    idx_all = np.arange(n)
    samples = np.empty((B, T, n))
    means, variances = np.empty((B, T)), np.empty((B, T))
    cfs = None if zs is None else np.empty((B, T, len(zs)), dtype=np.complex128)
    nell, first_nan = np.zeros(B), np.full(B, -1, dtype=np.int32)
    margin = math.inf
    with np.errstate(all='ignore'):
        for b in range(B):
            tables, pdf, seed = trans_of(b).tables, pdf_of(b), int(seeds[b])
            x = initial_particles(init_of(b), seed, n)
            for t in range(T):
                _, z = draws(seed, idx_all, t, 1, 0)
                mu = np.broadcast_to(tables.cond_mean(x), x.shape)
                var = np.broadcast_to(tables.cond_var(x), x.shape)
                x = np.where((var > 0.) & np.isfinite(var), mu + np.sqrt(var) * z, np.nan)
                w = np.asarray(pdf(ys[b, t], x), dtype=np.float64)
                s = w.sum()
                if not (np.isfinite(s) and s > 0.):
                    x = np.full(n, np.nan)
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
                means[b, t] = np.mean(x)
                variances[b, t] = np.mean((x - means[b, t]) ** 2)
                if zs is not None:
                    cfs[b, t] = np.mean(np.exp(1j * np.asarray(zs)[:, None] * x[None, :]), axis=1)
    return samples, means, variances, cfs, nell, first_nan, margin


def margin_bound(n):
    """16 n u: both sides' prefix sums are within n u of exact, so this is eight times the worst-case gap."""
    return 16 * n * 2. ** -53


def assert_close(dev, ref, scale, what, rtol=1e-9):
    """|dev - ref| <= rtol * scale elementwise; both NaN agrees."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape, f'{what}: shapes {dev.shape} and {ref.shape}'
    assert np.array_equal(np.isnan(dev), np.isnan(ref)), f'{what}: NaN patterns differ'
    with np.errstate(invalid='ignore'):
        err = np.where(np.isnan(ref), 0., np.abs(dev - ref))
        bound = np.where(np.isnan(ref), 1., rtol * np.broadcast_to(scale, ref.shape))
    worst = float(np.max(err / bound)) if err.size else 0.
    assert worst <= 1., f'{what}: worst error is {worst:.3g} x the bound'
    return worst
