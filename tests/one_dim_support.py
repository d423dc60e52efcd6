"""Support for the tests of the 1-D public API (mfs_amd.one_dim.filtering.moment_filter_rms / _cms / _scms), each piece defined
once: the device models paired with their oracle twins, one runner for the device filters and one for oracle/one_dim.py, the
moment comparison of tests/test_gpu_parity_1d.py, the fixture loader and the two checks of the NaN-poisoning structure.  The
prey--predator pair of the N-D tests that live in the 1-D files is in tests/nd_envelope_models.py.  A plain module: no
fixtures, nothing runs on import; tests/test_host_one_dim_support.py checks what the helpers here return, accept and refuse,
tests/test_host_test_layers.py that no support module imports a test module."""
import collections
import functools
import math
import os

import numpy as np
import pytest

from mfs_amd import stats
from mfs_amd.one_dim import filtering, moments, ss_models
from oracle import models as om, one_dim as o, tme_sympy

MODES = ('raw', 'central', 'scaled')
# A model's closures come as (rms, cms, scms, mean, mean_var), on the device and in the oracle alike.
MOMENTS_OF = {'raw': 0, 'central': 1, 'scaled': 2}        # mode -> the closure of its transition moments
MEAN_OF = {'raw': None, 'central': 3, 'scaled': 4}        # mode -> its mean (central) or mean-and-variance (scaled) closure
FILTER_OF = {'raw': 'moment_filter_rms', 'central': 'moment_filter_cms', 'scaled': 'moment_filter_scms'}
START_OF = {'raw': ('rms',), 'central': ('cms', 'mean'), 'scaled': ('scms', 'mean', 'scale')}   # mode -> its start arguments

Start = collections.namedtuple('Start', 'rms cms scms mean scale')
# what a run returns, with the replicate axis; None stands for an output the mode (or the side) does not have
Run = collections.namedtuple('Run', 'moments means scales nell first_nan')


def start_of(ic, variance=None):
    """The start of every mode from an initial law (a GaussianSum1D of either side); the scale is sqrt(variance)."""
    return Start(ic.rms, ic.cms, ic.scms, ic.mean, math.sqrt(ic.variance if variance is None else variance))


# ---- paired models ------------------------------------------------------------------------------------------------------
class Pair:
    """A device model and its oracle twin.  Device: dt, ic, fns (the five closures), pmf, start.  Oracle: oic, ofns, opmf,
    ostart, and osde = (drift, dispersion, dt) for a SymPy derivation of its own.  `ofns` is derived by SymPy (seconds at
    TME order 3) when it is first read: a test that runs the device alone does not pay for it.  Shared: not to be written to."""

    def __init__(self, make_ofns, **fields):
        self._make_ofns = make_ofns
        self.__dict__.update(fields)

    @functools.cached_property
    def ofns(self):
        return self._make_ofns()


def _sde_pair(N, family, order, sde, osde, **fields):
    """The closures of one transition family ('tme', 'tme_normal' of `order`, or 'euler') on both sides."""
    if family == 'euler':
        fns, make = moments.sde_cond_moments_euler(*sde, N), lambda: tme_sympy.sde_cond_moments_euler_1d(*osde, N)
    elif family == 'tme_normal':
        fns = moments.sde_cond_moments_tme_normal(*sde, order, N)
        make = lambda: tme_sympy.sde_cond_moments_tme_normal_1d(*osde, order, N)      # noqa: E731
    else:
        assert family == 'tme', family
        fns, make = moments.sde_cond_moments_tme(*sde, order), lambda: tme_sympy.sde_cond_moments_tme_1d(*osde, order, 2 * N)
    ic, oic = fields['ic'], fields['oic']
    # the scaled filters of both sides start from the device law's scale
    return Pair(make, N=N, dt=sde[2], fns=fns, osde=osde, start=start_of(ic), ostart=start_of(oic, ic.variance), **fields)


@functools.lru_cache(maxsize=None)
def benes(N, family='tme', order=3):
    """Benes--Bernoulli (BASELINE configs 1 and 2)."""
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli(N)
    odt, _, oic, odrift, odisp, _, opmf = om.benes_bernoulli(N)
    return _sde_pair(N, family, order, (drift, dispersion, dt), (odrift, odisp, odt), ic=ic, pmf=pmf, oic=oic, opmf=opmf)


@functools.lru_cache(maxsize=None)
def benes_operator_tables(N):
    """The TME-3 operator tables of the Benes pair for the C port (oracle/c): SymPy's derivation, independent of the product's."""
    return tme_sympy.operator_tables_1d(*benes(N).osde, 3, 'tanh')


@functools.lru_cache(maxsize=None)
def well(N, p1, family='tme_normal', order=2, p2=3.):
    """Well--Poisson (BASELINE config 4) with the drift bound to p1 and the emission to p2.  A tuple stands for per-replicate
    parameters, which only the device takes: the oracle twin of replicate b is well(N, p1[b], family, order, p2[b])."""
    p1, p2 = (np.asarray(p) if isinstance(p, tuple) else p for p in (p1, p2))
    dt, _, _, ic, drift0, dispersion, _, pmf0, _ = ss_models.well_poisson(3., N)
    odt, _, oic, odrift0, odisp, _, opmf0 = om.well_poisson(N)
    return _sde_pair(N, family, order, (lambda x: drift0(x, p1), dispersion, dt), (lambda x: odrift0(x, p1), odisp, odt),
                     ic=ic, pmf=lambda y, x: pmf0(y, x, p2), oic=oic, opmf=lambda y, x: opmf0(y, x, p2))


@functools.lru_cache(maxsize=None)
def ou_gaussian(N):
    """OU / Gaussian (BASELINE config 3): the exact discretisation X' | x ~ N(F x, Sigma), y | x ~ N(x, 1).  Both sides start
    from the oracle's moments of N(0, var0); `kf` is the exact Kalman filter of one replicate."""
    m = om.ou_gaussian(N)
    F, Sigma = m['F'], m['Sigma']
    start = Start(m['rms0'], m['cms0'], None, m['mean0'], None)
    ofns = (m['cond_rms'], m['cond_cms'], m['cond_scms'], m['cond_mean'], m['cond_mean_var'])
    return Pair(lambda: ofns, N=N, dt=0.1, F=F, Sigma=Sigma, var0=m['var0'], kf=m['kf'], start=start, ostart=start,
                fns=moments.sde_cond_moments_normal(lambda x: F * x, lambda x: Sigma),
                pmf=lambda y, x: stats.norm_pdf(y, x, 1.), opmf=m['pdf'])


# ---- the runners --------------------------------------------------------------------------------------------------------
def _filter(side, mode, fns, pmf, st, ys, **kw):
    closures = [fns[MOMENTS_OF[mode]]] + ([] if mode == 'raw' else [fns[MEAN_OF[mode]]])
    return getattr(side, FILTER_OF[mode])(*closures, pmf, *[getattr(st, k) for k in START_OF[mode]], ys, **kw)


def _run(mode, out):
    """A filter's (moments[, means[, scales]], nell, first_nan) as a Run."""
    aux = list(out[1:-2])
    return Run(out[0], *(aux + [None, None])[:2], out[-2], out[-1])


def run_device(mode, model, ys, *, start=None, stable=False, return_first_nan=False):
    """The public device filter of one mode on `ys`, (B, T) or (T,), from the model's start or `start` -> Run."""
    out = _filter(filtering, mode, model.fns, model.pmf, start or model.start, ys, stable=stable,
                  return_first_nan=return_first_nan)
    return _run(mode, tuple(out) + (() if return_first_nan else (None,)))


def run_oracle(mode, model, ys, *, start=None, stable=False):
    """oracle/one_dim.py on each replicate of `ys` (B, T) in turn, from the model's oracle start or `start`, stacked -> Run."""
    refs = [_filter(o, mode, model.ofns, model.opmf, start or model.ostart, y, stable=stable) for y in ys]
    return _run(mode, tuple(np.stack([r[k] for r in refs]) for k in range(len(refs[0]))) + (None,))


# ---- assertions ---------------------------------------------------------------------------------------------------------
RTOL = 1e-6


def assert_moments(got, ref, rtol=RTOL):
    """Relative error per moment order, with the denominator max(|ref|, typical magnitude of that order)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), 'NaN pattern differs'
    ok = ~nan_r
    # per-order magnitude: the largest |moment| of that order over the run, floored by the neighbouring even order
    # (odd central moments of near-symmetric laws and cms[1] are rounding noise around zero)
    colmax = np.nanmax(np.abs(ref), axis=0)
    even_neighbour = np.maximum(colmax, np.concatenate([colmax[1:], colmax[-1:]]))
    scale = np.maximum(np.abs(ref), even_neighbour[None, :] * 1e-3 + 1e-300)
    err = np.abs(got - ref)[ok] / scale[ok]
    assert err.size == 0 or err.max() <= rtol, f'max scaled error {err.max():.3e} > {rtol}'


def assert_poisoned_from(moments, means, nell, first_nan):
    """The strict rule: nothing before first_nan is NaN, everything from first_nan on is -- moments (if given) and means; the
    NLL is NaN exactly for a poisoned replicate."""
    nt = means.shape[1]
    for b in range(means.shape[0]):
        f = first_nan[b] if first_nan[b] >= 0 else nt
        assert np.isfinite(means[b, :f]).all() and np.isnan(means[b, f:]).all(), (b, f)
        if moments is not None:
            assert np.isfinite(moments[b, :f]).all() and np.isnan(moments[b, f:]).all(), (b, f)
        assert np.isnan(nell[b]) == (f < nt), (b, f)


def assert_poisoned_after(moments, means, nell, first_nan):
    """The lenient rule: first_nan >= 0  <=>  nell is NaN; before first_nan everything is finite, after it everything is NaN."""
    dead = first_nan >= 0
    assert np.array_equal(np.isnan(nell), dead)
    fin = np.isfinite(means)
    t = np.arange(means.shape[1])[None, :]
    expect_fin = np.where(dead[:, None], t < first_nan[:, None], True)
    # the poisoned step itself may hold a mixture; everything strictly before is finite, strictly after is NaN
    assert np.all(fin[expect_fin])
    after = np.where(dead[:, None], t > first_nan[:, None], False)
    assert not np.any(fin[after])
    assert np.all(np.isnan(moments[after]))


def load_golden(golden_dir, name, hint):
    """The fixture tests/golden/`name`; a missing one fails the test and says how to make it (`hint`)."""
    path = os.path.join(golden_dir, name)
    if not os.path.exists(path):
        pytest.fail(f'{name} is missing: {hint}')
    return np.load(path)
