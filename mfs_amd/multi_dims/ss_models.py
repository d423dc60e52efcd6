"""N-D test models, mirroring `mfs.multi_dims.ss_models` (same factory name and return tuple)."""
import numpy as np

from mfs_amd import sym, stats
from mfs_amd.utils import GaussianSumND


def prey_predator(multi_indices):
    """The prey--predator model (mfs/multi_dims/ss_models.py:40-95)."""
    dt = 1e-3
    T = 2000
    ts = np.linspace(dt, dt * T, T)
    alp, beta, delta, gamma, sigma = 4., 4., 4., 4., 0.1
    means = np.array([[1., 1.], [1., 1.]])
    covs = np.array([[[1., 0.], [0., 1.]], [[2., 0.], [0., 2.]]]) * 0.001
    weights = np.array([0.5, 0.5])
    gs = GaussianSumND.new(means, covs, weights, multi_indices)

    def drift(x):
        return x * (x[::-1] * np.array([-beta, delta]) + np.array([alp, -gamma]))

    def dispersion(x):
        return np.diag(sigma * x)

    def emission(x):
        return 1 / (1 + sym.exp(-x ** 3 + 1))

    def measurement_cond_pmf(y, x):
        return stats.bernoulli_pmf(y, emission(x[0]))

    def simulate(rng: np.random.Generator, integration_steps: int = 100):
        """Milstein path + Bernoulli measurements (:69-93); NumPy Generator instead of a JAX key."""
        ddt = dt / integration_steps
        x = gs.sampler(rng, 1)[0]
        x0 = x.copy()
        xs = np.empty((T, 2))
        for k in range(T):
            ddws = np.sqrt(ddt) * rng.standard_normal((integration_steps, 2))
            for ddw in ddws:
                x = x + drift(x) * ddt + sigma * x * ddw + 0.5 * sigma ** 2 * x * (ddw ** 2 - ddt)
            xs[k] = x
        p = 1 / (1 + np.exp(-xs[:, 0] ** 3 + 1))
        ys = (rng.random(T) < p).astype(np.float64)
        return x0, xs, ys

    return dt, T, ts, gs, drift, dispersion, emission, measurement_cond_pmf, simulate


def lorenz_tracking(multi_indices, sensor=(-5., -5., -2.), range_sd=0.5, angle_sd=0.1):
    """Lorenz-63 in units of 10 (d = 3) tracked by a sensor at `sensor` that measures range, azimuth and elevation of the
    state -- the 3-D form of the bearing-only measurement of the reference's examples/2d_bearing_only.ipynb.  The
    likelihood is three joint factors on the three measurement columns (no angle wrapping, as there).  Same return tuple as
    `prey_predator`; `emission(x)` is the noise-free (range, azimuth, elevation)."""
    dt = 0.01
    T = 200
    ts = np.linspace(dt, dt * T, T)
    sig, rho, beta, q = 10., 28., 8. / 3., 0.1
    sensor = np.asarray(sensor, dtype=np.float64)
    gs = GaussianSumND.new(np.array([[0.1, 0.1, 2.4]]), 0.01 * np.eye(3)[None], np.array([1.]), multi_indices)

    def drift(x):
        return np.array([sig * (x[1] - x[0]), x[0] * (rho - 10. * x[2]) - x[1], 10. * x[0] * x[1] - beta * x[2]],
                        dtype=object)

    def dispersion(x):
        return np.diag([q, q, q]).astype(object)

    def emission(x):
        dx, dy, dz = x[0] - sensor[0], x[1] - sensor[1], x[2] - sensor[2]
        ground = dx * dx + dy * dy
        return sym.sqrt(ground + dz * dz), sym.arctan2(dy, dx), sym.arctan2(dz, sym.sqrt(ground))

    def measurement_cond_pdf(y, x):
        rng_, az, el = emission(x)
        return stats.norm_pdf(y[0], rng_, range_sd) * stats.norm_pdf(y[1], az, angle_sd) * stats.norm_pdf(y[2], el, angle_sd)

    def simulate(rng: np.random.Generator, integration_steps: int = 10):
        """Euler--Maruyama path on `integration_steps` sub-steps per dt + the three noisy measurements, (T, 3)."""
        ddt = dt / integration_steps
        x = gs.sampler(rng, 1)[0]
        x0 = x.copy()
        xs = np.empty((T, 3))
        for k in range(T):
            for _ in range(integration_steps):
                x = x + drift(x).astype(np.float64) * ddt + q * np.sqrt(ddt) * rng.standard_normal(3)
            xs[k] = x
        clean = np.stack([np.asarray(v, dtype=np.float64) for v in emission(xs.T)], axis=-1)
        ys = clean + np.array([range_sd, angle_sd, angle_sd]) * rng.standard_normal((T, 3))
        return x0, xs, ys

    return dt, T, ts, gs, drift, dispersion, emission, measurement_cond_pdf, simulate
