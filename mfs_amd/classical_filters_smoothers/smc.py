"""The bootstrap particle filter on MI355X, mirroring `mfs.classical_filters_smoothers.smc`.

Same name and positional order as the reference's `bootstrap_filter` (mfs/classical_filters_smoothers/smc.py:26-33).  Its two
sampler callables draw from JAX keys and cannot be traced, so descriptors stand in their slots: `gaussian_transition(...)` for
`transition_sampler` (the Normal proposal of the drivers, tme.mean_and_cov or Euler--Maruyama) and a `GaussianSum1D` or an
array of initial particles for `init_sampler`.  The time loop -- propagation, weights, prefix sums, resampling, the per-step
mean, variance and empirical characteristic function -- runs in hand-written HIP (mfs_amd/csrc/particle_kernel.hpp) through
`mfs_particle_filter_1d` of include/mfs_hip.h, on the counter-based random stream that header states.  Extension over the
reference: `ys` may be (B, T) for B replicates (Monte-Carlo keys, or a parameter grid through (B,)-array model parameters).

A two-dimensional state (dardel/prey_predator/pf.py) takes the same call: `gaussian_transition_nd(drift, dispersion, 2, dt,
method)` in the transition slot and a `GaussianSumND` or (n, 2) particles in the initial slot run `mfs_particle_filter_nd`
(mfs_amd/csrc/particle_nd_kernel.hpp), whose per-step summaries are the mean vector and the covariance matrix.

There is no CPU fallback: callables that cannot be reduced to a device description raise `NotDeviceDescribable`.
"""
import ctypes as C
from typing import Callable, NamedTuple, Optional

import numpy as np

from mfs_amd import _lib
from mfs_amd.classical_filters_smoothers.resampling import Resampling, stratified
from mfs_amd.one_dim.filtering import _trace_likelihood, build_model_struct
from mfs_amd.one_dim.moments import _trace_sde
from mfs_amd.tme_poly import TransitionTables, euler_tables, tme_tables
from mfs_amd.utils import GaussianSum1D, GaussianSumND

__all__ = ['bootstrap_filter', 'gaussian_transition', 'GaussianTransition', 'ParticleFilterResult', 'ParticleFilterResultND']

_LIK_KINDS = ('bernoulli_logistic', 'poisson_softplus', 'gaussian')


class GaussianTransition(NamedTuple):
    """The proposal X' | x ~ N(mu(x), var(x)) as device tables (`tables.cond_mean`, `tables.cond_var` evaluate them); `dt` is
    the step the tables were built for (None if they were not built by `gaussian_transition`), which the Gaussian filters check
    against their own `dt` argument."""
    tables: TransitionTables
    dt: Optional[float] = None


class ParticleFilterResult(NamedTuple):
    """samples (B, T, n) or None: the resampled particles of every step; means, variances (B, T): their unweighted mean and
    population variance; cfs (B, T, nz) complex or None: mean_i exp(i z_k x_i); nell (B,): minus the sum of log mean_i w_i;
    first_nan (B,): the first step whose weights summed to zero or to a non-finite value, -1 if none.  Without a replicate
    axis on `ys` the leading B is dropped."""
    samples: Optional[np.ndarray]
    means: np.ndarray
    variances: np.ndarray
    cfs: Optional[np.ndarray]
    nell: np.ndarray
    first_nan: np.ndarray


class ParticleFilterResultND(NamedTuple):
    """The d = 2 filter's result: samples (B, T, n, 2) or None; means (B, T, 2) and covs (B, T, 2, 2): the unweighted mean and
    population covariance of every step's resampled particles; nell (B,); first_nan (B,) as in `ParticleFilterResult`.  Without
    a replicate axis on `ys` the leading B is dropped."""
    samples: Optional[np.ndarray]
    means: np.ndarray
    covs: np.ndarray
    nell: np.ndarray
    first_nan: np.ndarray


def gaussian_transition(drift: Callable, dispersion: Callable, dt: float, method: str = 'tme-3') -> GaussianTransition:
    """The Normal transition proposal of the reference's drivers (dardel/benes_bernoulli/pf.py: `tme.mean_and_cov`), traced
    like `brute_force_filter` traces its SDE.  method: 'tme-k' (TME of order k, Normal closure) or 'euler'.  Drift / dispersion
    parameters may be (B,) arrays: one table per replicate."""
    a, b = _trace_sde(drift, dispersion)
    if method == 'euler':
        return GaussianTransition(euler_tables(a, b, float(dt)), float(dt))
    if method.startswith('tme-'):
        try:
            order = int(method.split('-')[-1])
        except ValueError:
            raise ValueError(f"method must be 'tme-k' or 'euler', got {method!r}") from None
        return GaussianTransition(tme_tables(a, b, float(dt), order, gaussian=True), float(dt))
    raise ValueError(f"method must be 'tme-k' or 'euler', got {method!r}")


def _seeds(key, B, squeeze):
    if isinstance(key, (int, np.integer)):
        if key < 0:
            raise ValueError(f'key must be a non-negative integer, got {key}')
        return (np.uint64(int(key)) + np.arange(B, dtype=np.uint64)).astype(np.uint64)
    key = np.asarray(key)
    if key.dtype.kind not in 'ui' or (key.dtype.kind == 'i' and np.any(key < 0)):
        raise ValueError(f'key must be an int or an array of non-negative integers (uint64 seeds), got dtype {key.dtype}')
    if key.shape != (B,) or squeeze:
        raise ValueError(f'key must be an int or, with ys of shape ({B}, T), an array of shape ({B},); got shape {key.shape}')
    return np.ascontiguousarray(key, dtype=np.uint64)


def bootstrap_filter(transition, measurement_cond_pdf: Callable, ys, init, key, nsamples: int,
                     resampling: Resampling = stratified, conti_resampling: bool = False, *, zs=None,
                     return_samples: bool = True, return_summaries: bool = False, device: int = 0):
    """Bootstrap particle filter of a 1-D or 2-D state (mfs/classical_filters_smoothers/smc.py:26-84).

    transition             `gaussian_transition(drift, dispersion, dt, method)`; for a 2-D state
                           `gaussian_transition_nd(drift, dispersion, 2, dt, method)`: then measurement_cond_pdf is (y, x) with
                           x the two components (one or two factors, each of one component), ys (T,), (T, ny), (B, T) or
                           (B, T, ny), init a `GaussianSumND` or particles (n, 2) / (B, n, 2), zs is not available, and the
                           result is (samples (T, n, 2), nell) or a `ParticleFilterResultND`
    measurement_cond_pdf   (y, x) -> pdf, traced like the moment filters trace it (Bernoulli-logistic, Poisson-softplus,
                           Gaussian; parameters may be (B,) arrays)
    ys                     (T,) or (B, T) measurements
    init                   a `GaussianSum1D` (drawn on the device) or an array (n,) / (B, n) of initial particles
    key                    an int k: replicate b uses seed k + b; or a (B,) array of uint64 seeds
    nsamples               particles per replicate, 1 .. 2^20
    resampling             `stratified` or `systematic` of mfs_amd.classical_filters_smoothers.resampling
    zs                     (nz,) frequencies: also return the empirical characteristic function of every step
    return_samples         False: nothing of size B * T * n is allocated, on the host or the device
    return_summaries       True: return a `ParticleFilterResult`

    Returns (samples (T, n) or (B, T, n), nell), as the reference does, or a `ParticleFilterResult`.  Replicate b depends on
    its seed alone: it returns the same bits alone and in a batch.  A replicate whose weights sum to zero or to a non-finite
    value is NaN from that step on (see `first_nan`); the others are unaffected.
    """
    if conti_resampling:
        raise NotImplementedError('conti_resampling=True (continuous resampling, resampling.py:76-110) is not implemented: it '
                                  'needs a sort of the particles at every step, which the device filter does not have')
    if not isinstance(resampling, Resampling):
        raise ValueError('resampling must be `stratified` or `systematic` of mfs_amd.classical_filters_smoothers.resampling '
                         f'(the device draws from its own stream, not from a callable); got {resampling!r}')
    if resampling.code is None:
        raise NotImplementedError(f'{resampling.name} resampling is not implemented on the device (it needs n + 1 sorted '
                                  'uniforms, a prefix sum over the random stream); use stratified or systematic')
    from mfs_amd.classical_filters_smoothers.gfs import GaussianTransitionND     # (gfs imports this module)
    if isinstance(transition, GaussianTransitionND):
        return _bootstrap_filter_nd(transition, measurement_cond_pdf, ys, init, key, nsamples, resampling, zs, return_samples,
                                    return_summaries, device)
    if not isinstance(transition, GaussianTransition):
        raise ValueError('transition must be built by gaussian_transition(drift, dispersion, dt, method): a sampler callable '
                         f'cannot be traced; got {type(transition).__name__}')
    if not (return_samples or return_summaries):
        raise ValueError('nothing to return: return_samples and return_summaries are both False')
    if zs is not None and not return_summaries:
        raise ValueError('zs asks for characteristic functions, which only a ParticleFilterResult carries: pass '
                         'return_summaries=True')
    n = int(nsamples)
    if n != nsamples or not 1 <= n <= _lib.PF_MAX_PARTICLES:
        raise ValueError(f'nsamples must be an integer in [1, {_lib.PF_MAX_PARTICLES}], got {nsamples}')
    tables = transition.tables
    lik = _trace_likelihood(measurement_cond_pdf)
    if lik.kind not in _LIK_KINDS or len(lik.factors) != 1:
        raise ValueError(f'the particle filter supports the 1-D likelihoods {_LIK_KINDS}, got {lik!r}')

    ys = np.asarray(ys)
    squeeze = ys.ndim == 1
    ys2 = np.ascontiguousarray(ys[None, :] if squeeze else ys, dtype=np.float64)
    if ys2.ndim != 2 or ys2.shape[1] < 1 or ys2.shape[0] < 1:
        raise ValueError(f'ys must have shape (T,) or (B, T) with T >= 1, got {ys.shape}')
    B, T = ys2.shape
    if squeeze and (tables.batch_shape() != () or np.ndim(lik.params) != 1):
        raise ValueError('per-replicate model parameters need ys of shape (B, T)')
    seeds = _seeds(key, B, squeeze)

    mix = [None, None, None]
    init_samples = None
    if isinstance(init, GaussianSum1D):
        K = init.means.shape[0]
        if not 1 <= K <= _lib.PF_MAX_MIX:
            raise ValueError(f'the initial mixture has {K} components; the device draws from 1 .. {_lib.PF_MAX_MIX}')
        if not (np.all(np.isfinite(init.variances)) and np.all(init.variances > 0.) and np.all(np.isfinite(init.means))):
            raise ValueError('the initial mixture needs finite means and finite variances > 0')
        mix = [np.ascontiguousarray(np.cumsum(init.weights), dtype=np.float64),
               np.ascontiguousarray(init.means, dtype=np.float64), np.ascontiguousarray(init.variances, dtype=np.float64)]
    else:
        init_samples = np.ascontiguousarray(init, dtype=np.float64)
        if init_samples.shape not in ((n,), (B, n)) or (squeeze and init_samples.ndim == 2):
            raise ValueError(f'init must be a GaussianSum1D or particles of shape ({n},) or, with ys of shape ({B}, T), '
                             f'({B}, {n}); got {init_samples.shape}')
    nz = 0
    if zs is not None:
        zs = np.ascontiguousarray(zs, dtype=np.float64)
        if zs.ndim != 1 or zs.shape[0] < 1 or not np.all(np.isfinite(zs)):
            raise ValueError(f'zs must be a finite array of shape (nz,) with nz >= 1, got shape {zs.shape}')
        nz = zs.shape[0]
    model, keep = build_model_struct(tables, lik, B)

    samples = _lib.pinned_empty((B, T, n), device=device) if return_samples else None
    means, variances = np.empty((B, T)), np.empty((B, T))
    cfs = _lib.pinned_empty((B, T, nz), dtype=np.complex128, device=device) if nz else None
    nell, first_nan = np.empty((B,)), np.empty((B,), dtype=np.int32)
    _lib.check(_lib.lib().mfs_particle_filter_1d(
        C.byref(model), n, T, B, resampling.code, _lib.ptr(seeds), 0 if mix[0] is None else mix[0].shape[0],
        _lib.ptr(mix[0]), _lib.ptr(mix[1]), _lib.ptr(mix[2]), _lib.ptr(init_samples),
        int(init_samples is not None and init_samples.ndim == 2), _lib.ptr(ys2), nz, _lib.ptr(zs), _lib.ptr(samples),
        _lib.ptr(means), _lib.ptr(variances), _lib.ptr(cfs), _lib.ptr(nell), _lib.ptr(first_nan), device, None))
    del keep
    if not return_summaries:
        return (samples[0], nell[0]) if squeeze else (samples, nell)
    outs = [samples, means, variances, cfs, nell, first_nan]
    if squeeze:
        outs = [None if o is None else o[0] for o in outs]
    return ParticleFilterResult(*outs)


def _chol2(covs):
    """Lower Cholesky factors of (K, 2, 2) covariance matrices by the closed form the device uses per particle:
    l00 = sqrt(c00), l10 = c01 / l00, l11 = sqrt(c11 - l10^2)."""
    covs = np.asarray(covs, dtype=np.float64)
    L = np.zeros(covs.shape)
    with np.errstate(all='ignore'):
        L[:, 0, 0] = np.sqrt(covs[:, 0, 0])
        L[:, 1, 0] = covs[:, 1, 0] / L[:, 0, 0]
        L[:, 1, 1] = np.sqrt(covs[:, 1, 1] - L[:, 1, 0] ** 2)
    return L


def _bootstrap_filter_nd(transition, measurement_cond_pdf, ys, init, key, nsamples, resampling, zs, return_samples,
                         return_summaries, device):
    """The d = 2 path of `bootstrap_filter` (its resampler checks are done).  Every argument error comes before the library is
    loaded."""
    from mfs_amd.multi_dims import filtering as fnd
    tables = transition.tables
    if zs is not None:
        raise NotImplementedError('zs asks for characteristic functions, which exist for 1-D states only: there is no N-D '
                                  'characteristic function on the device')
    if tables.d != 2:
        raise NotImplementedError(f'the particle filter runs 1-D and 2-D states on the device, got d = {tables.d}')
    if not tables.is_gaussian:
        raise ValueError('transition needs the Normal closure built by gaussian_transition_nd(drift, dispersion, 2, dt, method)')
    if not (return_samples or return_summaries):
        raise ValueError('nothing to return: return_samples and return_summaries are both False')
    n = int(nsamples)
    if n != nsamples or not 1 <= n <= _lib.PF_MAX_PARTICLES:
        raise ValueError(f'nsamples must be an integer in [1, {_lib.PF_MAX_PARTICLES}], got {nsamples}')
    factors = fnd._trace_likelihood(measurement_cond_pdf, 2)    # NotDeviceDescribable beyond MFS_ND_MAX_FACTORS factors
    for f in factors:
        if f.kind not in _LIK_KINDS or int(f.component) not in (0, 1):
            raise ValueError(f'the 2-D particle filter supports the likelihood kinds {_LIK_KINDS}, each of one state component; '
                             f'got {f!r}')
    ny = max(f.ycol for f in factors) + 1
    ys3, squeeze = fnd._split_ys(ys, ny)
    if ys3.shape[0] < 1 or ys3.shape[1] < 1:
        raise ValueError(f'ys must hold at least one replicate and one measurement, got shape {np.shape(ys)}')
    B, T = ys3.shape[:2]
    seeds = _seeds(key, B, squeeze)

    mix = [None, None, None]
    init_samples = None
    if isinstance(init, GaussianSumND):
        K = init.means.shape[0]
        if init.d != 2:
            raise ValueError(f'the initial mixture is {init.d}-dimensional, the state 2-dimensional')
        if not 1 <= K <= _lib.PF_MAX_MIX:
            raise ValueError(f'the initial mixture has {K} components; the device draws from 1 .. {_lib.PF_MAX_MIX}')
        chol = _chol2(init.covs)
        if not (np.all(np.isfinite(chol)) and np.all(chol[:, 0, 0] > 0.) and np.all(chol[:, 1, 1] > 0.)
                and np.all(np.isfinite(init.means))):
            raise ValueError('the initial mixture needs finite means and positive definite covariances')
        mix = [np.ascontiguousarray(np.cumsum(init.weights), dtype=np.float64),
               np.ascontiguousarray(init.means, dtype=np.float64), np.ascontiguousarray(chol)]
    elif isinstance(init, GaussianSum1D):
        raise ValueError('init is a GaussianSum1D, the state is 2-dimensional: pass a GaussianSumND')
    else:
        init_samples = np.ascontiguousarray(init, dtype=np.float64)
        if init_samples.shape not in ((n, 2), (B, n, 2)) or (squeeze and init_samples.ndim == 3):
            raise ValueError(f'init must be a GaussianSumND or particles of shape ({n}, 2) or, with a replicate axis on ys, '
                             f'({B}, {n}, 2); got {init_samples.shape}')
    if squeeze and (hasattr(tables, 'members') or any(np.ndim(f.params) != 1 for f in factors)):
        raise ValueError('per-replicate model parameters need ys with a leading replicate axis')
    model, keep = fnd._model_struct(tables, factors, B)

    samples = _lib.pinned_empty((B, T, n, 2), device=device) if return_samples else None
    means, covs = np.empty((B, T, 2)), np.empty((B, T, 2, 2))
    nell, first_nan = np.empty((B,)), np.empty((B,), dtype=np.int32)
    _lib.check(_lib.lib().mfs_particle_filter_nd(
        C.byref(model), n, T, B, resampling.code, _lib.ptr(seeds), 0 if mix[0] is None else mix[0].shape[0],
        _lib.ptr(mix[0]), _lib.ptr(mix[1]), _lib.ptr(mix[2]), _lib.ptr(init_samples),
        int(init_samples is not None and init_samples.ndim == 3), _lib.ptr(ys3), _lib.ptr(samples), _lib.ptr(means),
        _lib.ptr(covs), _lib.ptr(nell), _lib.ptr(first_nan), device, None))
    del keep
    if not return_summaries:
        return (samples[0], nell[0]) if squeeze else (samples, nell)
    outs = [samples, means, covs, nell, first_nan]
    if squeeze:
        outs = [None if o is None else o[0] for o in outs]
    return ParticleFilterResultND(*outs)
