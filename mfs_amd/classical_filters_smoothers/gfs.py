"""The Gaussian filters on MI355X, mirroring `mfs.classical_filters_smoothers.gfs`: the sigma-point filter `sgp_filter`
(:503-551; with `SigmaPoints.gauss_hermite` it is the Gauss--Hermite filter of the paper's tables) and the extended Kalman
filter `ekf` (:317-362), for states of dimension 1 and 2 and a scalar measurement.

Same names and positional order as the reference.  Its two callables return JAX arrays and are differentiated by JAX, so
descriptors stand in their slots, as in `smc.py`:

    state_cond_m_cov         `gaussian_transition(drift, dispersion, dt, method)` (1-D) or
                             `gaussian_transition_nd(drift, dispersion, d, dt, method)` (d = 2): the Normal closure of the SDE
                             step, tme.mean_and_cov ('tme-k') or Euler--Maruyama ('euler'), as polynomial tables
    measurement_cond_m_cov   `measurement_moments(measurement_cond_pdf)`: the pdf is traced as the moment filters trace it, and
                             the conditional mean and variance follow from its kind -- Bernoulli-logistic (p, p (1 - p)),
                             Poisson-softplus (rate, rate), Gaussian (l0 x + l1, l2)

The time loop runs in hand-written HIP (mfs_amd/csrc/gaussfilter_kernel.hpp) through `mfs_gaussian_filter_1d` / `_nd` of
include/mfs_hip.h, which states the step and the NaN rule.  The EKF's Jacobians are analytic, on the device.  Extension over
the reference: a leading replicate axis B on `ys` (and then optionally on `m0` / `v0` and, as (B,) arrays, on the model
parameters): Monte-Carlo runs, or a parameter grid whose negative log-likelihoods give finite-difference gradients.

Out of scope: the smoothers (`rts`, `eks`, `sgp_smoother`), the continuous-discrete `cd_*` filters and smoothers, the linear
`kf`, vector measurements (dy > 1), d = 3, and gradients of the negative log-likelihood (a parameter batch covers finite
differences).  There is no CPU fallback: arguments are validated before the library is loaded, and a missing library raises.
"""
import ctypes as C
from typing import Callable, NamedTuple, Optional

import numpy as np

from mfs_amd import _lib
from mfs_amd.classical_filters_smoothers.quadratures import SigmaPoints
from mfs_amd.classical_filters_smoothers.smc import GaussianTransition
from mfs_amd.multi_dims import filtering as _fnd
from mfs_amd.one_dim.filtering import _trace_likelihood, build_model_struct
from mfs_amd.tme_poly_nd import GaussianTablesND, normal_tables_nd

__all__ = ['sgp_filter', 'ekf', 'gaussian_transition_nd', 'measurement_moments', 'GaussianTransitionND', 'MeasurementMoments']

GF_SIGMA_POINT, GF_EKF = _lib.GF_METHOD['sigma_point'], _lib.GF_METHOD['ekf']
GF_MAX_POINTS = _lib.GF_MAX_POINTS
_LIK_KINDS = ('bernoulli_logistic', 'poisson_softplus', 'gaussian')


class GaussianTransitionND(NamedTuple):
    """X' | x ~ N(mu(x), S(x)) of a d-dimensional SDE step as device tables, and the step `dt` they were built for."""
    tables: GaussianTablesND
    dt: Optional[float] = None


class MeasurementMoments(NamedTuple):
    """Stands in the reference's `measurement_cond_m_cov` slot: the measurement pdf, traced when the filter knows the state
    dimension."""
    pdf: Callable

    def spec(self, d: int):
        """The single likelihood factor of the traced pdf for a d-dimensional state (.kind, .params, .component)."""
        if d == 1:
            lik = _trace_likelihood(self.pdf)
            factors = lik.factors
        else:
            factors = _fnd._trace_likelihood(self.pdf, d)
        if len(factors) != 1:
            raise NotImplementedError(f'the Gaussian filters take a scalar measurement (dy = 1): one likelihood factor, got '
                                      f'{len(factors)}')
        f = factors[0]
        if f.kind not in _LIK_KINDS or int(f.component) not in range(d):
            raise NotImplementedError(f'the Gaussian filters support the likelihood kinds {_LIK_KINDS} of one state component, '
                                      f'got {f!r}')
        return f


def measurement_moments(measurement_cond_pdf: Callable) -> MeasurementMoments:
    """The conditional mean and variance of the measurement, from its pdf (y, x) -> p(y | x) written with mfs_amd.stats /
    mfs_amd.sym as for the moment filters.  For d = 2 the pdf must be one factor of one state component (the prey--predator
    model); two factors or a bearing measurement raise NotImplementedError when the filter is called."""
    if not callable(measurement_cond_pdf):
        raise ValueError(f'measurement_cond_pdf must be a callable (y, x) -> pdf, got {type(measurement_cond_pdf).__name__}')
    return MeasurementMoments(measurement_cond_pdf)


def gaussian_transition_nd(drift: Callable, dispersion: Callable, d: int, dt: float, method: str = 'tme-2'):
    """The Normal transition of a d-dimensional SDE step over `normal_tables_nd`: method 'euler' or 'tme-k'.  d = 1 gives the
    1-D descriptor (`GaussianTransition`)."""
    if method == 'euler':
        order = 'euler'
    else:
        try:
            if not method.startswith('tme-'):
                raise ValueError
            order = int(method.split('-')[-1])
        except (ValueError, AttributeError):
            raise ValueError(f"method must be 'tme-k' or 'euler', got {method!r}") from None
    tables = normal_tables_nd(drift, dispersion, int(d), float(dt), order)
    if int(d) == 1:
        return GaussianTransition(tables.as_one_dim(), float(dt))
    return GaussianTransitionND(tables, float(dt))


def _split_ys(ys):
    """-> (ys (B, T) contiguous float64, squeeze): (T,), (T, 1), (B, T) or (B, T, 1)."""
    ys = np.asarray(ys)
    shape = ys.shape
    if ys.ndim == 3 and shape[-1] == 1:
        ys, squeeze = ys[..., 0], False
    elif ys.ndim == 2 and shape[-1] == 1:
        ys, squeeze = ys[None, :, 0], True
    elif ys.ndim == 2:
        squeeze = False
    elif ys.ndim == 1:
        ys, squeeze = ys[None, :], True
    else:
        raise ValueError(f'ys must have shape (T,), (T, 1), (B, T) or (B, T, 1), got {shape}')
    if ys.shape[0] < 1 or ys.shape[1] < 1:
        raise ValueError(f'ys must hold at least one replicate and one measurement, got shape {shape}')
    return np.ascontiguousarray(ys, dtype=np.float64), squeeze


def _initial(m0, v0, d, B, squeeze):
    """-> (m0 (d,) or (B, d), v0 (d, d) or (B, d, d), batched)."""
    m0, v0 = np.asarray(m0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    if m0.shape == (d,) or (d == 1 and m0.shape == ()):
        bm = False
    elif m0.shape == (B, d) or (d == 1 and m0.shape == (B,)):
        bm = True
    else:
        raise ValueError(f'm0 must have shape ({d},) or ({B}, {d}), got {m0.shape}')
    if v0.shape == (d, d) or (d == 1 and v0.shape in ((), (1,))):
        bv = False
    elif v0.shape == (B, d, d) or (d == 1 and v0.shape in ((B,), (B, 1))):
        bv = True
    else:
        raise ValueError(f'v0 must have shape ({d}, {d}) or ({B}, {d}, {d}), got {v0.shape}')
    batched = bm or bv
    if batched and squeeze:
        raise ValueError('m0 / v0 with a leading replicate axis need ys with one too')
    lead = (B,) if batched else ()
    m0 = np.ascontiguousarray(np.broadcast_to(m0.reshape(((B,) if bm else ()) + (d,)), lead + (d,)))
    v0 = np.ascontiguousarray(np.broadcast_to(v0.reshape(((B,) if bv else ()) + (d, d)), lead + (d, d)))
    return m0, v0, batched


def _run(method, state_cond_m_cov, measurement_cond_m_cov, sgps, m0, v0, dt, ys, return_first_nan, device):
    if not isinstance(state_cond_m_cov, (GaussianTransition, GaussianTransitionND)):
        raise ValueError('state_cond_m_cov must be built by gaussian_transition(drift, dispersion, dt, method) or '
                         'gaussian_transition_nd(drift, dispersion, d, dt, method): a callable cannot be traced; got '
                         f'{type(state_cond_m_cov).__name__}')
    if not isinstance(measurement_cond_m_cov, MeasurementMoments):
        raise ValueError('measurement_cond_m_cov must be built by measurement_moments(measurement_cond_pdf); got '
                         f'{type(measurement_cond_m_cov).__name__}')
    tables = state_cond_m_cov.tables
    nd = isinstance(state_cond_m_cov, GaussianTransitionND)
    d = tables.d if nd else 1
    if nd and d != 2:
        raise NotImplementedError(f'the Gaussian filters run d = 1 and d = 2 on the device, got d = {d}')
    if not nd and tables.kind != 'gaussian':
        raise ValueError(f'state_cond_m_cov needs the Normal closure of the transition, got {tables.kind!r} tables ({tables.label})')
    if state_cond_m_cov.dt is not None and not np.isclose(float(dt), state_cond_m_cov.dt, rtol=1e-12, atol=0.):
        raise ValueError(f'dt = {dt} differs from the step the transition was built for, {state_cond_m_cov.dt}')
    xi = w = None
    n_points = 0
    if method == GF_SIGMA_POINT:
        if not isinstance(sgps, SigmaPoints):
            raise ValueError(f'sgps must be a SigmaPoints of mfs_amd.classical_filters_smoothers.quadratures, got '
                             f'{type(sgps).__name__}')
        if sgps.d != d:
            raise ValueError(f'the sigma points are {sgps.d}-dimensional, the state is {d}-dimensional')
        xi, w = np.ascontiguousarray(sgps.xi, dtype=np.float64), np.ascontiguousarray(sgps.w, dtype=np.float64)
        n_points = w.shape[0]
        if xi.shape != (n_points, d) or n_points != sgps.n_points:
            raise ValueError(f'sigma points of shape {xi.shape} and weights of shape {w.shape} do not make a rule of '
                             f'{sgps.n_points} points in {d} dimensions')
        if not 1 <= n_points <= GF_MAX_POINTS:
            raise ValueError(f'the device takes rules of 1 .. {GF_MAX_POINTS} points, got {n_points}')
    lik = measurement_cond_m_cov.spec(d)
    ys2, squeeze = _split_ys(ys)
    B, T = ys2.shape
    m0, v0, batched = _initial(m0, v0, d, B, squeeze)
    if squeeze and (np.ndim(lik.params) != 1 or (not nd and tables.batch_shape() != ())):
        raise ValueError('per-replicate model parameters need ys with a leading replicate axis')
    if nd:
        model, keep = _fnd._model_struct(tables, [lik], B)
    else:
        model, keep = build_model_struct(tables, lik, B)

    means = _lib.pinned_empty((B, T, d), device=device)
    covs = _lib.pinned_empty((B, T, d, d), device=device)
    nells = _lib.pinned_empty((B, T), device=device)
    first_nan = np.empty((B,), dtype=np.int32)
    entry = _lib.lib().mfs_gaussian_filter_nd if nd else _lib.lib().mfs_gaussian_filter_1d
    _lib.check(entry(C.byref(model), method, n_points, _lib.ptr(xi), _lib.ptr(w), T, B, _lib.ptr(m0), _lib.ptr(v0),
                     int(batched), _lib.ptr(ys2), _lib.ptr(means), _lib.ptr(covs), _lib.ptr(nells), _lib.ptr(first_nan),
                     device, None))
    del keep
    return _lib.shape_outputs((means, covs, nells, first_nan), squeeze, return_first_nan)


def sgp_filter(state_cond_m_cov, measurement_cond_m_cov, sgps: SigmaPoints, m0, v0, dt: float, ys,
               const_measurement_cov: bool = False, *, return_first_nan: bool = False, device: int = 0):
    """Sigma-point filter (mfs/classical_filters_smoothers/gfs.py:503-551).

    state_cond_m_cov        `gaussian_transition(...)` / `gaussian_transition_nd(...)`
    measurement_cond_m_cov  `measurement_moments(measurement_cond_pdf)`
    sgps                    a `SigmaPoints` rule of the state's dimension, 1 .. 256 points
    m0, v0                  (dx,), (dx, dx), or with a leading B
    dt                      must equal the step the transition was built for (ValueError otherwise)
    ys                      (T,), (T, 1) as the reference's `_ys[:, None]`, (B, T) or (B, T, 1)
    const_measurement_cov   accepted and ignored: in the reference it only saves evaluating a constant measurement variance at
                            every sigma point, and changes no number

    Returns (mfs (T, dx), vfs (T, dx, dx), nells (T,)) with `nells` the running sum, as the reference's scan returns it; with a
    replicate axis on `ys` each has a leading B.  return_first_nan=True appends (B,) int32: the first step at which a Cholesky
    pivot was negative, the innovation variance not positive or the measurement not finite, from which on that replicate is
    NaN, or -1.
    """
    return _run(GF_SIGMA_POINT, state_cond_m_cov, measurement_cond_m_cov, sgps, m0, v0, dt, ys, return_first_nan, device)


def ekf(state_cond_m_cov, measurement_cond_m_cov, m0, v0, dt: float, ys, fwd_jacobian: bool = False, *,
        return_first_nan: bool = False, device: int = 0):
    """Extended Kalman filter (mfs/classical_filters_smoothers/gfs.py:317-362); arguments and returns as `sgp_filter`.
    fwd_jacobian is accepted and ignored: it chooses between JAX's forward and reverse autodiff in the reference, and the
    device evaluates the Jacobians of the polynomial tables and of the measurement mean analytically."""
    return _run(GF_EKF, state_cond_m_cov, measurement_cond_m_cov, None, m0, v0, dt, ys, return_first_nan, device)
