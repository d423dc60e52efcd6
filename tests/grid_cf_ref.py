"""Yardstick of the grid-filter characteristic-function tests: an exactly summed restatement of characteristic_from_pdf
(mfs/one_dim/moments.py:340-343) and the derived parity bound.  A plain helper module, not a conftest.

For a density row p on xs and a frequency z the terms are w_i cos(z x_i) p_i and w_i sin(z x_i) p_i, each formed in float64
(fl(z x_i), libm's cos / sin, two multiplications), with w the weights of np.trapezoid(., xs); the terms are then summed
exactly (math.fsum), so the restatement carries no accumulation error of its own.

Bound on |device - restatement| per real and imaginary part:

    2 (n + 2 max|z_k x_i| + 8) 2^-53 sum_i w_i |p_i|

n roundings of the k-ascending accumulation, each at most u times the sum of the absolute terms; one argument rounding
u |z x| on each side (the sine and cosine have slope <= 1); three roundings per table entry and term on each side, inside the 8;
a factor 2 of room.
"""
import math

import numpy as np

from tests.brute_force_ref import trapz_weights

U = 2.0 ** -53


def cf_ref(ps, xs, zs):
    """ps (..., n), xs (n,), zs (m,) -> complex128 (..., m).  A row with a non-finite entry is NaN in both parts."""
    ps, xs, zs = np.asarray(ps, dtype=np.float64), np.asarray(xs, dtype=np.float64), np.atleast_1d(np.asarray(zs, dtype=np.float64))
    w = trapz_weights(xs)
    rows = ps.reshape(-1, xs.shape[0])
    out = np.empty((rows.shape[0], zs.shape[0]), dtype=np.complex128)
    arg = zs[:, None] * xs[None, :]
    wc, ws = w[None, :] * np.cos(arg), w[None, :] * np.sin(arg)
    for r, p in enumerate(rows):
        if not np.isfinite(p).all():
            out[r] = complex(np.nan, np.nan)
            continue
        tc, ts = wc * p[None, :], ws * p[None, :]
        for k in range(zs.shape[0]):
            out[r, k] = complex(math.fsum(tc[k]), math.fsum(ts[k]))
    return out.reshape(ps.shape[:-1] + zs.shape)


def cf_bound(ps, xs, zs):
    """The parity bound per part, shape ps.shape[:-1] + (1,): it does not depend on the frequency beyond max |z x|."""
    ps, xs, zs = np.asarray(ps, dtype=np.float64), np.asarray(xs, dtype=np.float64), np.atleast_1d(np.asarray(zs, dtype=np.float64))
    n = xs.shape[0]
    zx = np.abs(zs).max() * np.abs(xs).max()
    mass = np.abs(ps) @ trapz_weights(xs)
    return (2. * (n + 2. * zx + 8.) * U * mass)[..., None]


def worst_ratio(dev, ref, bound):
    """max over both parts of |dev - ref| / bound, NaN entries of the reference (which the device must share) left out."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape and dev.dtype == np.complex128
    nan_r = np.isnan(ref.real) | np.isnan(ref.imag)
    nan_d = np.isnan(dev.real) & np.isnan(dev.imag)
    assert np.array_equal(nan_d, nan_r) and not (np.isnan(dev.real) ^ np.isnan(dev.imag)).any(), 'NaN patterns differ'
    bound = np.broadcast_to(bound, ref.shape)
    ok = ~nan_r
    if not ok.any():
        return 0.
    d = dev[ok] - ref[ok]
    return float(max(np.abs(d.real / bound[ok]).max(), np.abs(d.imag / bound[ok]).max()))


# ---- the two analytic pins, shared by the host test of the restatement alone and the GPU tests
def normal_pin_case():
    """N(mu, sigma^2) on linspace(mu - 8 sigma, mu + 8 sigma, 257) and frequencies with |z| sigma <= 4, uneven."""
    mu, sigma = 0.7, 0.45
    xs = np.linspace(mu - 8 * sigma, mu + 8 * sigma, 257)
    ps = np.exp(-0.5 * ((xs - mu) / sigma) ** 2) / (math.sqrt(2 * math.pi) * sigma)
    zs = np.concatenate([np.linspace(-4., 4., 23) ** 3 / 16., [0., 4., -4.]]) / sigma
    return mu, sigma, xs, ps, zs


KALMAN_ZS = np.concatenate([np.linspace(-2., 2., 9), [0.37, -1.9]])


def kalman_cf_tolerance(zs, true_m, true_v):
    """|z| dm + z^2 dv / 2 + 1e-12 with dm, dv the absolute deviations test_kalman_pin_on_the_device_power_route allows:
    atol 1e-11 plus rtol 1e-10 of the value (of m_t and of v_t, the smaller of the readings for the variance)."""
    dm = 1e-11 + 1e-10 * np.abs(true_m)
    dv = 1e-11 + 1e-10 * np.abs(true_v)
    return np.abs(zs)[None, :] * dm[:, None] + 0.5 * zs[None, :] ** 2 * dv[:, None] + 1e-12
