"""The brute-force grid filter on MI355X, mirroring `mfs.classical_filters_smoothers.brute_force`.

Same name, positional order and defaults as the reference (mfs/classical_filters_smoothers/brute_force.py:26-29); the
Chapman--Kolmogorov time loop runs in hand-written HIP (mfs_amd/csrc/gridfilter_kernel.hpp: an fp64 matrix-core GEMM and a
per-replicate measurement update) through `mfs_grid_filter_1d` of include/mfs_hip.h.  Extension over the reference: `ys` may
be (B, T) and `init_ps` (B, n) for B replicates on the one grid, likelihood parameters may be per-replicate, and the
posterior means, variances and the true negative log marginal likelihood come back on request.

There is no CPU fallback: callables that cannot be reduced to a device description raise `NotDeviceDescribable`.
"""
from typing import Callable, NamedTuple, Optional

import numpy as np

from mfs_amd import _lib
from mfs_amd.one_dim.filtering import _trace_likelihood
from mfs_amd.one_dim.moments import _trace_sde
from mfs_amd.tme_poly import TransitionTables, euler_tables, tme_tables

__all__ = ['brute_force_filter', 'GridFilterResult', 'GridFilterCFResult', 'transition_on_grid']

_LIK_KINDS = ('bernoulli_logistic', 'poisson_softplus', 'gaussian')


class GridFilterResult(NamedTuple):
    """pdfs (B, T, n) or None; means, variances (B, T): trapezoid integrals of each posterior; nell (B,): minus the sum of
    log int p(y_t | x) p_pred(x) dx; first_nan (B,): the first step whose normaliser was zero or not finite, -1 if none.
    Without a replicate axis on `ys` the leading B is dropped."""
    pdfs: Optional[np.ndarray]
    means: np.ndarray
    variances: np.ndarray
    nell: np.ndarray
    first_nan: np.ndarray


class GridFilterCFResult(NamedTuple):
    """The five fields of `GridFilterResult`, then cfs (B, T, m) complex128: the characteristic function of each posterior at
    the frequencies `zs`, trapezoid rule on the grid; NaN in both parts for a replicate from its `first_nan` on."""
    pdfs: Optional[np.ndarray]
    means: np.ndarray
    variances: np.ndarray
    nell: np.ndarray
    first_nan: np.ndarray
    cfs: np.ndarray


def _check_zs(zs) -> np.ndarray:
    """The frequencies of a characteristic function on the grid as a contiguous (m,) float64 array."""
    zs = np.asarray(zs, dtype=np.float64)
    if zs.ndim != 1 or zs.shape[0] < 1:
        raise ValueError(f'zs must have shape (m,) with m >= 1, got {zs.shape}')
    zs = np.ascontiguousarray(zs)
    if zs.shape[0] > _lib.GRID_MAX_NZ:
        raise ValueError(f'm = {zs.shape[0]} frequencies exceed the supported {_lib.GRID_MAX_NZ}')
    if not np.all(np.isfinite(zs)):
        raise ValueError('zs must be finite')
    return zs


def _transition_tables(drift: Callable, dispersion: Callable, ddt: float, pred_method: str) -> TransitionTables:
    if pred_method == 'kolmogorov':
        raise NotImplementedError("pred_method 'kolmogorov' (finite-difference Kolmogorov forward equation) is not "
                                  "implemented: no driver uses it and the reference warns about its stability; use "
                                  "'chapman-euler' or 'chapman-tme-k'")
    a, b = _trace_sde(drift, dispersion)
    if pred_method == 'chapman-euler':
        tables = euler_tables(a, b, ddt)
    elif pred_method.startswith('chapman-tme-'):
        try:
            order = int(pred_method.split('-')[-1])
        except ValueError:
            raise NotImplementedError(f'Prediction method {pred_method} not implemented.') from None
        tables = tme_tables(a, b, ddt, order, gaussian=True)
    else:
        raise NotImplementedError(f'Prediction method {pred_method} not implemented.')
    if tables.batch_shape() != ():
        raise ValueError('per-replicate drift / dispersion parameters are not supported by the grid filter: one transition '
                         'matrix serves the whole batch (call once per parameter value)')
    return tables


def transition_on_grid(drift: Callable, dispersion: Callable, xs, dt: float, integration_steps: int = 1,
                       pred_method: str = 'chapman-tme-2'):
    """(mean, sd) of the Normal transition density over one sub-step dt / integration_steps, at every grid point: the
    `m, scale` of brute_force.py:69-78 (Euler, or tme.mean_and_cov)."""
    xs = np.asarray(xs, dtype=np.float64)
    tables = _transition_tables(drift, dispersion, float(dt) / int(integration_steps), pred_method)
    mean = np.broadcast_to(tables.cond_mean(xs), xs.shape)
    var = np.broadcast_to(tables.cond_var(xs), xs.shape)
    return np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(np.sqrt(var), dtype=np.float64)


def brute_force_filter(drift: Callable, dispersion: Callable, measurement_cond_pdf: Callable, init_ps, xs, ys, dt,
                       integration_steps: int = 1, pred_method: str = 'chapman-tme-2', *,
                       return_pdfs: bool = True, return_summaries: bool = False, route: str = 'auto', device: int = 0,
                       zs=None):
    """Brute-force computing the true filtering solution of a 1-D state on a grid
    (mfs/classical_filters_smoothers/brute_force.py:26-136, the 'chapman-euler' and 'chapman-tme-k' predictors).

    drift, dispersion      the SDE coefficients, traced like `sde_cond_moments_*` trace them
    measurement_cond_pdf   (y, x) -> pdf, traced like the moment filters trace it (Bernoulli-logistic, Poisson-softplus,
                           Gaussian; parameters may be (B,) arrays)
    init_ps                (n,) or (B, n) initial density on the grid
    xs                     (n,) strictly increasing grid, shared by the batch (uneven spacing allowed: trapezoid weights)
    ys                     (T,) or (B, T) measurements
    dt, integration_steps  measurement interval and the sub-steps per interval
    route                  'power': form the matrix of one whole interval once (K^S by repeated squaring), one product per
                           measurement; 'stepwise': apply K S times per measurement, as the reference does; 'auto': power
                           when S > 1
    return_pdfs            False: nothing of size B * T * n is allocated, on the host or the device
    return_summaries       True: return a `GridFilterResult`
    zs                     (m,) frequencies: also compute the characteristic function of every posterior on the device,
                           trapz(exp(i z x) p, x) -- the `true_filtering_cfs` of
                           dardel/benes_bernoulli/post_processing_brute_force.py:27-50 -- and return a `GridFilterCFResult`
                           (implies return_summaries; with return_pdfs=False the pdfs never leave the device)

    Returns the (T, n) or (B, T, n) filtering pdfs, as the reference does, or a `GridFilterResult` / `GridFilterCFResult`.
    A replicate whose normaliser is zero or not finite is NaN from that step on (see `first_nan`); the others are unaffected.
    """
    if route not in ('auto', 'power', 'stepwise'):
        raise ValueError(f"route must be 'auto', 'power' or 'stepwise', got {route!r}")
    if zs is not None:
        zs = _check_zs(zs)
        return_summaries = True
    if not (return_pdfs or return_summaries):
        raise ValueError('nothing to return: return_pdfs and return_summaries are both False')
    S = int(integration_steps)
    if S < 1:
        raise ValueError(f'integration_steps must be >= 1, got {integration_steps}')
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    if xs.ndim != 1 or xs.shape[0] < 2:
        raise ValueError(f'xs must have shape (n,) with n >= 2, got {xs.shape}')
    if not np.all(np.isfinite(xs)) or not np.all(np.diff(xs) > 0.):
        raise ValueError('xs must be finite and strictly increasing')
    n = xs.shape[0]
    if n > _lib.GRID_MAX_N:
        raise ValueError(f'n = {n} grid points exceed the supported {_lib.GRID_MAX_N}')
    trans_mean, trans_sd = transition_on_grid(drift, dispersion, xs, dt, S, pred_method)
    if not np.all(np.isfinite(trans_sd)) or not np.all(trans_sd > 0.):
        raise ValueError('the transition variance is not finite and positive on the whole grid')
    lik = _trace_likelihood(measurement_cond_pdf)
    if lik.kind not in _LIK_KINDS or len(lik.factors) != 1:
        raise ValueError(f'the grid filter supports the 1-D likelihoods {_LIK_KINDS}, got {lik!r}')

    ys = np.asarray(ys)
    squeeze = ys.ndim == 1
    ys2 = np.ascontiguousarray(ys[None, :] if squeeze else ys, dtype=np.float64)
    if ys2.ndim != 2 or ys2.shape[1] < 1:
        raise ValueError(f'ys must have shape (T,) or (B, T) with T >= 1, got {ys.shape}')
    B, T = ys2.shape
    init_ps = np.ascontiguousarray(init_ps, dtype=np.float64)
    if init_ps.shape not in ((n,), (B, n)) or (squeeze and init_ps.ndim == 2):
        raise ValueError(f'init_ps must have shape ({n},) or, with ys of shape ({B}, T), ({B}, {n}); got {init_ps.shape}')
    lp = np.ascontiguousarray(lik.params, dtype=np.float64)
    if lp.ndim != 1 and (squeeze or lp.shape[:-1] != (B,)):
        raise ValueError(f'likelihood parameters are batched with shape {lp.shape[:-1]}, but ys has '
                         f'{"no replicate axis" if squeeze else f"{B} replicates"}')

    pdfs = _lib.pinned_empty((B, T, n), device=device) if return_pdfs else None
    means, variances = np.empty((B, T)), np.empty((B, T))
    nell, first_nan = np.empty((B,)), np.empty((B,), dtype=np.int32)
    use_power = int(route == 'power' or (route == 'auto' and S > 1))
    nz = 0 if zs is None else zs.shape[0]
    cfs = _lib.pinned_empty((B, T, nz), dtype=np.complex128, device=device) if nz else None
    _lib.check(_lib.lib().mfs_grid_filter_1d_cf(
        n, T, B, S, use_power, _lib.ptr(xs), _lib.ptr(trans_mean), _lib.ptr(trans_sd),
        _lib.LIK[lik.kind], lp.shape[-1], _lib.ptr(lp), int(lp.ndim != 1), _lib.ptr(init_ps), int(init_ps.ndim == 2),
        _lib.ptr(ys2), nz, _lib.ptr(zs), _lib.ptr(pdfs), _lib.ptr(means), _lib.ptr(variances), _lib.ptr(cfs), _lib.ptr(nell),
        _lib.ptr(first_nan), device, None))
    if not return_summaries:
        return pdfs[0] if squeeze else pdfs
    outs = [pdfs, means, variances, nell, first_nan] + ([cfs] if nz else [])
    if squeeze:
        outs = [None if o is None else o[0] for o in outs]
    return (GridFilterCFResult if nz else GridFilterResult)(*outs)
