"""Freeze what the Python host layer hands the C ABI as tests/golden/host_calls.npz.

libmfs_hip.so is a function of its arguments, so the behaviour of every public filter is fixed by the arguments that reach
`mfs_filter_1d`, `mfs_filter_1d_grad`, `mfs_filter_nd`, `mfs_filter_nd3` and `mfs_filter_nd3_joint`.  This module runs the
public entry points of mfs_amd.one_dim.filtering, mfs_amd.multi_dims.filtering and mfs_amd.estimation over small cases that
take every branch of the host layer, with the library replaced by a recorder (no GPU, no libmfs_hip.so), and stores per case
the C call (entry point, scalars, arrays, descriptor structs with their pointer fields zeroed, the tables those pointers
address) and what the public function returned or raised.  tests/test_host_calls.py replays the cases and compares without
a tolerance.  Arrays of more than 4096 elements are stored as shape and SHA-256.  The file is written with fixed zip
timestamps: the same code gives the same bytes.  Run from the repository root:

    python tests/golden/make_host_calls.py
"""
import ctypes as C
import hashlib
import io
import json
import math
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mfs_amd import _lib, estimation, stats, sym  # noqa: E402
from mfs_amd.multi_dims import filtering as fnd, moments as mnd, ss_models as snd  # noqa: E402
from mfs_amd.multi_dims.multi_indices import (generate_graded_lexico_multi_indices as gen_mi,  # noqa: E402
                                              gram_and_hankel_indices_graded_lexico as gen_inds)
from mfs_amd.one_dim import filtering as f1, moments as m1, ss_models as s1  # noqa: E402

PATH = os.path.join(HERE, 'host_calls.npz')
BIG = 4096
T, B = 5, 3
ENTRY_POINTS = ('mfs_filter_1d', 'mfs_filter_1d_grad', 'mfs_filter_nd', 'mfs_filter_nd3', 'mfs_filter_nd3_joint')
# positions of the output arrays in each entry point's argument list (include/mfs_hip.h)
OUTPUTS = {'mfs_filter_1d': range(11, 16), 'mfs_filter_1d_grad': range(13, 16), 'mfs_filter_nd': range(14, 19),
           'mfs_filter_nd3': range(14, 19), 'mfs_filter_nd3_joint': range(15, 20)}


# ---------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------
def _addressed(p, n):
    """The n doubles a descriptor's pointer field addresses (copied)."""
    return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0)


def _tables_of(name, structs, args):
    """The arrays the descriptors point to, with the element counts the host units (mfs_amd/csrc/capi_*.hip) compute for their uploads."""
    m = structs[0]
    nb = args[7 if name == 'mfs_filter_1d_grad' else 3 + len(structs)]
    if isinstance(m, _lib.MfsModel1d):
        ncoef, nlik = m.n_rows * (m.degree + 1), m.n_lik
    elif isinstance(m, _lib.MfsModelNd):
        ncoef, nlik = _lib.nd_table_rows(m.n_terms) * m.extent ** 2, m.n_factors * _lib.MAX_LIK
    else:
        ncoef, nlik = _lib.ND3_ROWS * m.extent ** 3, m.n_factors * _lib.MAX_LIK
    out = [_addressed(m.coef, (nb if m.coef_batched else 1) * ncoef), _addressed(m.lik, (nb if m.lik_batched else 1) * nlik)]
    if len(structs) == 2:
        j = structs[1]
        njb = nb if j.batched else 1
        out += [_addressed(j.coef, njb * j.n_joint * 2 * j.extent ** 3), _addressed(j.par, njb * j.n_joint)]
    return out


def _struct_bytes(s):
    raw = bytearray(C.string_at(C.addressof(s), C.sizeof(s)))
    for field, ctype in s._fields_:
        if ctype is _lib.c_double_p:
            off = getattr(type(s), field).offset
            raw[off:off + 8] = bytes(8)
    return np.frombuffer(bytes(raw), dtype=np.uint8)


class Recorder:
    """Stands in for the loaded library: every attribute is a function that logs its call, fills the output arrays with
    arange + their argument position, and returns MFS_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            meta, arrays, structs = [], {}, []
            for pos, a in enumerate(args):
                if hasattr(a, '_obj'):                       # C.byref(descriptor)
                    structs.append(a._obj)
                    meta.append('struct')
                    arrays[f'arg{pos}'] = _struct_bytes(a._obj)
                elif isinstance(a, np.ndarray) and pos in OUTPUTS.get(name, ()):
                    assert a.flags['C_CONTIGUOUS']
                    meta.append(['out', a.dtype.str, list(a.shape)])
                    a[...] = (np.arange(a.size) + pos).astype(a.dtype).reshape(a.shape)
                elif isinstance(a, np.ndarray):
                    assert a.flags['C_CONTIGUOUS']           # what _lib.ptr insists on
                    meta.append('array')
                    arrays[f'arg{pos}'] = a.copy()
                else:
                    assert a is None or isinstance(a, (int, np.integer)), (name, pos, a)
                    meta.append(None if a is None else int(a))
            if structs:
                for k, t in enumerate(_tables_of(name, structs, args)):
                    arrays[f'table{k}'] = t
            self.calls.append((name, meta, arrays))
            return _lib.MFS_OK
        return entry


def install(monkeypatch):
    """Replace the library, the pointer conversion and the pinned allocator (the filtering modules look all three up as
    `_lib.<name>` at call time); returns the recorder."""
    rec = Recorder()
    monkeypatch.setattr(_lib, 'lib', lambda: rec)
    monkeypatch.setattr(_lib, 'ptr', lambda a: a)
    monkeypatch.setattr(_lib, 'pinned_empty', lambda shape, dtype=np.float64, device=0: np.empty(shape, dtype=dtype))
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# the cases: name -> function performing one public call
# ---------------------------------------------------------------------------------------------------------------------
def _grid(shape, mod=5, div=4.):
    """Deterministic measurements without a random generator or libm: ((7 k) mod `mod`) / div."""
    n = int(np.prod(shape))
    return ((np.arange(n) * 7) % mod / div).reshape(shape)


def _bits(shape):
    return _grid(shape, 2, 1.)


CASES = {}


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return deco


# ---- 1-D, N = 3 ----
def _benes(N=3, order=2):
    dt, _, _, ic, drift, disp, _, pmf, _ = s1.benes_bernoulli(N)
    return ic, pmf, m1.sde_cond_moments_tme(drift, disp, dt, order)


def _call_1d(mode, ys, batched_ms0, **kw):
    ic, pmf, fns = _benes()
    rep = (lambda v: np.tile(v, (B, 1)) * (1. + 0.01 * np.arange(B))[:, None]) if batched_ms0 else (lambda v: v)
    mean0 = ic.mean + 0.1 * np.arange(B) if batched_ms0 else ic.mean
    if mode == 'raw':
        return f1.moment_filter_rms(fns[0], pmf, rep(ic.rms), ys, **kw)
    if mode == 'central':
        return f1.moment_filter_cms(fns[1], fns[3], pmf, rep(ic.cms), mean0, ys, **kw)
    return f1.moment_filter_scms(fns[2], fns[4], pmf, rep(ic.scms), mean0, math.sqrt(ic.variance), ys, **kw)


for _mode in ('raw', 'central', 'scaled'):
    CASES[f'1d_benes_{_mode}_T'] = lambda m=_mode: _call_1d(m, _bits((T,)), False)
    CASES[f'1d_benes_{_mode}_BT'] = lambda m=_mode: _call_1d(m, _bits((B, T)), False)
    CASES[f'1d_benes_{_mode}_BT_ms0B'] = lambda m=_mode: _call_1d(m, _bits((B, T)), True)
    CASES[f'1d_benes_{_mode}_first_nan'] = lambda m=_mode: _call_1d(m, _bits((T,)), False, return_first_nan=True)
CASES['1d_benes_central_stable'] = lambda: _call_1d('central', _bits((B, T)), False, stable=True)
CASES['1d_benes_int_ys'] = lambda: _call_1d('central', _bits((B, T)).astype(np.int64), False)


@case('1d_benes_raw_odd_moment_count')
def _():
    ic, pmf, fns = _benes()
    return f1.moment_filter_rms(fns[0], pmf, ic.rms[:5], _bits((B, T)))


def _well(p1, p2, N=3):
    dt, _, _, ic, drift, disp, _, pmf, _ = s1.well_poisson(3., N)
    _, c, _, mu, _ = m1.sde_cond_moments_tme_normal(lambda x: drift(x, p1), disp, dt, 2, N)
    return ic, c, mu, (lambda y, x: pmf(y, x, p2))


@case('1d_well_poisson_normal_per_replicate')
def _():
    ic, c, mu, pdf = _well(np.array([0.5, 2., 4.5]), np.array([1., 3., 2.5]))
    return f1.moment_filter_cms(c, mu, pdf, ic.cms, ic.mean, _grid((B, T), 5, 1.), return_first_nan=True)


@case('1d_hand_written_mean')
def _():
    F, Sigma = 0.9, 0.2
    _, c, _, _, _ = m1.sde_cond_moments_normal(lambda x: F * x, lambda x: Sigma)
    ic = s1.benes_bernoulli(3)[3]
    return f1.moment_filter_cms(c, lambda x: F * x, lambda y, x: stats.norm_pdf(y, x, 1.), ic.cms, ic.mean, _grid((T,)))


def _linear_scaled(var_of):
    """Scaled filter of x' = F x + N(0, Sigma) with a hand-written (mean, variance) closure."""
    F, Sigma = 0.9, 0.2
    _, _, s, _, _ = m1.sde_cond_moments_normal(lambda x: F * x, lambda x: Sigma)
    ic = s1.benes_bernoulli(3)[3]
    return f1.moment_filter_scms(s, lambda x: (F * x, var_of(x, Sigma)), lambda y, x: stats.norm_pdf(y, x, 1.), ic.scms,
                                 ic.mean, math.sqrt(ic.variance), _grid((T,)))


CASES['1d_hand_written_mean_var'] = lambda: _linear_scaled(lambda x, Sigma: 0. * x + Sigma)
CASES['1d_refuse_hand_written_variance_disagrees'] = lambda: _linear_scaled(lambda x, Sigma: 0. * x + 2. * Sigma)


# refusals of one_dim.filtering
@case('1d_refuse_untraceable_transition')
def _():
    ic, pmf, fns = _benes()
    return f1.moment_filter_rms(lambda x, order: x, pmf, ic.rms, _bits((T,)))


@case('1d_refuse_transition_not_forwarding_mean')
def _():
    ic, pmf, fns = _benes()
    return f1.moment_filter_cms(lambda x, order, mean: fns[1](x, order, 0.), fns[3], pmf, ic.cms, ic.mean, _bits((T,)))


@case('1d_refuse_mean_of_another_model')
def _():
    ic, pmf, fns = _benes()
    other = _benes(order=3)[2]
    return f1.moment_filter_cms(fns[1], other[3], pmf, ic.cms, ic.mean, _bits((T,)))


@case('1d_refuse_hand_written_mean_disagrees')
def _():
    _, c, _, _, _ = m1.sde_cond_moments_normal(lambda x: 0.9 * x, lambda x: 0.2)
    ic = s1.benes_bernoulli(3)[3]
    return f1.moment_filter_cms(c, lambda x: 0.8 * x, lambda y, x: stats.norm_pdf(y, x, 1.), ic.cms, ic.mean, _grid((T,)))


@case('1d_refuse_untraceable_likelihood')
def _():
    ic, pmf, fns = _benes()
    return f1.moment_filter_rms(fns[0], lambda y, x: 1., ic.rms, _bits((T,)))


@case('1d_refuse_likelihood_batch')
def _():
    ic, c, mu, pdf = _well(3., np.array([1., 3.]))
    return f1.moment_filter_cms(c, mu, pdf, ic.cms, ic.mean, _grid((B, T), 5, 1.))


@case('1d_refuse_ys_rank')
def _():
    return _call_1d('raw', _bits((2, B, T)), False)


@case('1d_refuse_ms0_batch')
def _():
    ic, pmf, fns = _benes()
    return f1.moment_filter_rms(fns[0], pmf, np.tile(ic.rms, (B + 1, 1)), _bits((B, T)))


@case('1d_refuse_mean0_shape')
def _():
    ic, pmf, fns = _benes()
    return f1.moment_filter_cms(fns[1], fns[3], pmf, np.tile(ic.cms, (B, 1)), np.zeros(B + 1), _bits((B, T)))


@case('1d_refuse_squeezed_ys_with_per_replicate_parameters')
def _():
    ic, c, mu, pdf = _well(np.array([0.5, 2., 4.5]), 3.)
    return f1.moment_filter_cms(c, mu, pdf, ic.cms, ic.mean, _grid((T,), 5, 1.))


@case('1d_refuse_N_out_of_range')
def _():
    ic, pmf, fns = _benes()
    return f1.moment_filter_rms(fns[0], pmf, ic.rms[:2], _bits((T,)))


# ---- d = 2, N = 2 ----
def _pp(N=2):
    mi, inds = gen_mi(2, 2 * N - 1), gen_inds(N, 2)
    dt, _, _, gs, drift, disp, _, pmf, _ = snd.prey_predator(mi)
    return mi, inds, dt, gs, drift, disp, pmf


def _pp_family(family, mi, dt, drift, disp):
    if family == 'tme_normal_2':
        return mnd.sde_cond_moments_tme_normal(drift, disp, dt, 2, mi), 'index'
    return mnd.sde_cond_moments_tme(drift, disp, dt, {'tme_2': 2, 'tme_3': 3}[family]), 'multi-index'


def _call_nd(mode, fns, sig, pdf, ys, mi, inds, rms, cms, mean, batched_ms0=False, **kw):
    """One N-D public call; scaled mode starts from the marginal standard deviations."""
    d = mi.shape[1]
    nb = np.shape(ys)[0]
    rep = (lambda v: np.tile(v, (nb, 1)) * (1. + 0.01 * np.arange(nb))[:, None]) if batched_ms0 else (lambda v: v)
    if mode == 'raw':
        return fnd.moment_filter_nd_rms((fns[0], sig), pdf, ys, (mi, inds), rep(rms), **kw)
    if mode == 'central':
        return fnd.moment_filter_nd_cms((fns[1], sig), fns[3], pdf, ys, (mi, inds), rep(cms), rep(mean), **kw)
    second = [int(np.where((mi == 2 * np.eye(d, dtype=int)[k]).all(axis=1))[0][0]) for k in range(d)]
    scale0 = np.sqrt(cms[second])
    return fnd.moment_filter_nd_scms((fns[2], sig), fns[4], pdf, ys, (mi, inds), rep(cms / np.prod(scale0 ** mi, axis=-1)),
                                     rep(mean), rep(scale0), **kw)


def _call_pp(mode, family, ys, pdf=None, **kw):
    mi, inds, dt, gs, drift, disp, pmf = _pp()
    fns, sig = _pp_family(family, mi, dt, drift, disp)
    return _call_nd(mode, fns, sig, pdf or pmf, ys, mi, inds, gs.rms, gs.cms, gs.mean, **kw)


for _family in ('tme_2', 'tme_3', 'tme_normal_2'):
    for _mode in ('raw', 'central', 'scaled'):
        CASES[f'nd2_{_family}_{_mode}_T'] = lambda m=_mode, f=_family: _call_pp(m, f, _bits((T,)))
        CASES[f'nd2_{_family}_{_mode}_BT'] = lambda m=_mode, f=_family: _call_pp(m, f, _bits((B, T)))
CASES['nd2_tme_2_scaled_BT_ms0B'] = lambda: _call_pp('scaled', 'tme_2', _bits((B, T)), batched_ms0=True)
CASES['nd2_tme_2_central_first_nan_stable'] = lambda: _call_pp('central', 'tme_2', _bits((B, T)), return_first_nan=True,
                                                               stable=True)
CASES['nd2_tme_2_raw_ys_BT1'] = lambda: _call_pp('raw', 'tme_2', _bits((B, T, 1)))


def _two_gauss(y, x):
    return math.prod(stats.norm_pdf(y, x, 1.5))


CASES['nd2_two_gaussian_factors_T2'] = lambda: _call_pp('central', 'tme_2', _grid((T, 2)), _two_gauss)
CASES['nd2_two_gaussian_factors_BT2'] = lambda: _call_pp('scaled', 'tme_normal_2', _grid((B, T, 2)), _two_gauss)
CASES['nd2_bearing'] = lambda: _call_pp('central', 'tme_2', _grid((B, T)),
                                        lambda y, x: stats.norm_pdf(y, sym.arctan2(x[1], x[0]), 0.3))
CASES['nd2_per_replicate_likelihood'] = lambda: _call_pp(
    'central', 'tme_2', _bits((B, T)),
    lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-x[0] ** 3 + np.array([1., 0.5, 1.5])))))


def _pp_batch_closures(sigs=(0.05, 0.1, 0.2)):
    mi, inds, dt, gs, drift, _, pmf = _pp()
    per = [mnd.sde_cond_moments_tme(drift, lambda x, s=s: np.array([[s * x[0], 0.], [0., s * x[1]]], dtype=object), dt, 2)
           for s in sigs]
    return mi, inds, gs, pmf, mnd.batch_closures(per)


@case('nd2_batch_closures')
def _():
    mi, inds, gs, pmf, fns = _pp_batch_closures()
    return _call_nd('scaled', fns, 'multi-index', pmf, _bits((B, T)), mi, inds, gs.rms, gs.cms, gs.mean)


# ---- d = 3, N = 2 ----
def _lorenz(N=2):
    mi, inds = gen_mi(3, 2 * N - 1), gen_inds(N, 3)
    dt, _, _, gs, drift, disp, _, rae, _ = snd.lorenz_tracking(mi)
    return mi, inds, dt, gs, drift, disp, rae


def _call_l3(mode, family, pdf, ys, N=2, **kw):
    mi, inds, dt, gs, drift, disp, rae = _lorenz(N)
    if family == 'tme_normal_2':
        fns, sig = mnd.sde_cond_moments_tme_normal(drift, disp, dt, 2, mi), 'index'
    else:
        fns, sig = mnd.sde_cond_moments_tme(drift, disp, dt, int(family[-1]), d=3), 'multi-index'
    return _call_nd(mode, fns, sig, pdf if pdf is not None else rae, ys, mi, inds, gs.rms, gs.cms, gs.mean, **kw)


def _one(y, x):
    return stats.norm_pdf(y, x[0], 0.5)


def _two(y, x):
    return stats.norm_pdf(y[0], x[0], 0.5) * stats.poisson_pmf(y[1], sym.log(1. + sym.exp(x[2])))


def _three(y, x):
    return np.prod(stats.norm_pdf(y, x, 0.5))


def _mixed(y, x):
    return stats.norm_pdf(y[1], x[2], 0.5) * stats.norm_pdf(y[0], x[0] * x[1], 0.5)


for _family in ('tme_2', 'tme_normal_2'):
    for _mode in ('raw', 'central', 'scaled'):
        CASES[f'nd3_{_family}_{_mode}_one_factor_BT'] = lambda m=_mode, f=_family: _call_l3(m, f, _one, _grid((B, T)))
    CASES[f'nd3_{_family}_one_factor_T'] = lambda f=_family: _call_l3('central', f, _one, _grid((T,)))
    CASES[f'nd3_{_family}_two_factors'] = lambda f=_family: _call_l3('central', f, _two, _grid((B, T, 2), 5, 1.))
    CASES[f'nd3_{_family}_three_factors'] = lambda f=_family: _call_l3('scaled', f, _three, _grid((T, 3)))
    CASES[f'nd3_{_family}_joint_rae'] = lambda f=_family: _call_l3('central', f, None, _grid((B, T, 3)))
CASES['nd3_joint_rae_raw_T'] = lambda: _call_l3('raw', 'tme_2', None, _grid((T, 3)))
CASES['nd3_joint_rae_scaled_ms0B'] = lambda: _call_l3('scaled', 'tme_2', None, _grid((B, T, 3)), batched_ms0=True,
                                                      return_first_nan=True, stable=True)
CASES['nd3_mixed_single_and_joint'] = lambda: _call_l3('central', 'tme_2', _mixed, _grid((B, T, 2)))
CASES['nd3_joint_per_replicate'] = lambda: _call_l3(
    'central', 'tme_2', stats.batch_likelihoods([lambda y, x, k=k: stats.norm_pdf(y[1], x[0] * x[1] + k, 0.5 + k)
                                                 * stats.norm_pdf(y[0], x[2], 1. + k) for k in range(B)]), _grid((B, T, 2)))


@case('nd3_batch_closures')
def _():
    mi, inds, dt, gs, drift, _, _ = _lorenz()
    per = [mnd.sde_cond_moments_tme(drift, lambda x, s=s: np.diag([s, s, s]).astype(object), dt, 2, d=3)
           for s in (0.1, 0.2, 0.3)]
    return _call_nd('central', mnd.batch_closures(per), 'multi-index', _one, _grid((B, T)), mi, inds, gs.rms, gs.cms, gs.mean)


# ---- d = 1 through the N-D entry points ----
def _call_d1(mode, ys, pdf=None, N=3, **kw):
    mi, inds = gen_mi(1, 2 * N - 1, 0), gen_inds(N, 1)
    ic = s1.benes_bernoulli(N)[3]
    fns = mnd.sde_cond_moments_tme(lambda x: -x, lambda _: 0.7, 1e-2, 2, d=1)
    return _call_nd(mode, fns, 'multi-index', pdf or (lambda y, x: stats.norm_pdf(y, x, 1.)), ys, mi, inds, ic.rms, ic.cms,
                    np.array([ic.mean]), **kw)


for _mode in ('raw', 'central', 'scaled'):
    CASES[f'nd1_{_mode}_T'] = lambda m=_mode: _call_d1(m, _grid((T,)))
    CASES[f'nd1_{_mode}_BT1'] = lambda m=_mode: _call_d1(m, _grid((B, T, 1)), return_first_nan=True)


# ---- the in-kernel gradient ----
def _grad_model(P):
    dt, _, _, ic, drift, disp, _, pmf, _ = s1.well_poisson(3., 3)
    _, c, _, mu, _ = m1.sde_cond_moments_tme_normal(lambda x: drift(x, P[:, 0]), disp, dt, 2, 3)
    return c, mu, (lambda y, x: pmf(y, x, P[:, 1]))


def _call_grad(params, ys, **kw):
    ic = s1.well_poisson(3., 3)[3]
    return estimation.nell_and_grad_forward(_grad_model, np.asarray(params), ic.cms, ic.mean, ys, **kw)


_THETAS = [[2.2, 2.7], [3.0, 3.0], [1.5, 4.0]]
for _tan in ('complex-step', 'stencil'):
    CASES[f'grad_{_tan}_P_T'] = lambda t=_tan: _call_grad(_THETAS[0], _grid((T,), 5, 1.), tangents=t)
    CASES[f'grad_{_tan}_P_RT'] = lambda t=_tan: _call_grad(_THETAS[0], _grid((B, T), 5, 1.), tangents=t)
    CASES[f'grad_{_tan}_RP_RT'] = lambda t=_tan: _call_grad(_THETAS, _grid((B, T), 5, 1.), tangents=t, return_first_nan=True)
    CASES[f'grad_{_tan}_RP_T'] = lambda t=_tan: _call_grad(_THETAS, _grid((T,), 5, 1.), tangents=t)
CASES['grad_refuse_row_count'] = lambda: _call_grad(_THETAS, _grid((B + 1, T), 5, 1.))
CASES['grad_refuse_tangents'] = lambda: _call_grad(_THETAS[0], _grid((T,), 5, 1.), tangents='adjoint')


@case('grad_scaled_tanh_operator_tables')
def _():
    ic = s1.benes_bernoulli(3)[3]

    def model(P):
        fns = m1.sde_cond_moments_tme(lambda x: P[:, 0] * sym.tanh(x), lambda _: P[:, 1], 1e-2, 2)
        return fns[2], fns[4], (lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-P[:, 2] * x ** 3))))
    return estimation.nell_and_grad_forward(model, np.array([0.9, 1.1, 0.25]), ic.scms, ic.mean, _bits((T,)),
                                            scale0=math.sqrt(ic.variance), mode='scaled')


# ---- refusals of multi_dims.filtering ----
def _pp_cms(trans, mean_fn, pdf, ys, ms0=None, mean0=None, order=None):
    mi, inds, dt, gs, drift, disp, pmf = _pp()
    return fnd.moment_filter_nd_cms(trans, mean_fn, pdf or pmf, ys, order or (mi, inds), gs.cms if ms0 is None else ms0,
                                    gs.mean if mean0 is None else mean0)


def _pp_fns(family='tme_2'):
    mi, inds, dt, gs, drift, disp, pmf = _pp()
    return _pp_family(family, mi, dt, drift, disp)[0]


CASES['nd_refuse_unknown_signature'] = lambda: _pp_cms((_pp_fns()[1], 'indices'), _pp_fns()[3], None, _bits((T,)))
CASES['nd_refuse_untraceable_transition'] = lambda: _pp_cms((lambda x, idx, mean: x, 'multi-index'), _pp_fns()[3], None,
                                                            _bits((T,)))


@case('nd_refuse_transition_not_forwarding_mean')
def _():
    fns = _pp_fns()
    return _pp_cms((lambda x, idx, mean: fns[0](x, idx), 'multi-index'), fns[3], None, _bits((T,)))


CASES['nd_refuse_signature_of_another_family'] = lambda: _pp_cms((_pp_fns()[1], 'index'), _pp_fns()[3], None, _bits((T,)))


@case('nd_refuse_index_table_mismatch')
def _():
    fns = _pp_fns('tme_normal_2')
    return _pp_cms((fns[1], 'index'), fns[3], None, _bits((T,)), order=(gen_mi(2, 5), gen_inds(3, 2)))


@case('nd_refuse_mean_closure_from_another_call')
def _():
    return _pp_cms((_pp_fns()[1], 'multi-index'), _pp_fns()[3], None, _bits((T,)))


@case('nd_refuse_mean_var_closure_from_another_call')
def _():
    mi, inds, dt, gs, drift, disp, pmf = _pp()
    fns = _pp_fns()
    return fnd.moment_filter_nd_scms((fns[2], 'multi-index'), fns[3], pmf, _bits((T,)), (mi, inds), gs.cms, gs.mean,
                                     np.ones(2))


def _refuse_lik(pdf, ys=None):
    fns = _pp_fns()
    return _pp_cms((fns[1], 'multi-index'), fns[3], pdf, _bits((T,)) if ys is None else ys)


CASES['nd_refuse_likelihood_vector'] = lambda: _refuse_lik(lambda y, x: stats.norm_pdf(y, x, 1.))
CASES['nd_refuse_untraceable_likelihood'] = lambda: _refuse_lik(lambda y, x: 1.)
CASES['nd_refuse_joint_factor_at_d2'] = lambda: _refuse_lik(lambda y, x: stats.norm_pdf(y, x[0] * x[1], 0.5))
CASES['nd_refuse_too_many_factors_d2'] = lambda: _refuse_lik(
    lambda y, x: stats.norm_pdf(y[0], x[0], 1.) * stats.norm_pdf(y[1], x[1], 1.) * stats.norm_pdf(y[2], x[0], 2.))
CASES['nd_refuse_too_many_factors_d3'] = lambda: _call_l3(
    'central', 'tme_2', lambda y, x: math.prod(stats.norm_pdf(y[k], x[k % 3], 0.5 + k) for k in range(4)), _grid((T, 4)))
CASES['nd_refuse_too_many_joint_factors'] = lambda: _call_l3(
    'central', 'tme_2', lambda y, x: np.prod([stats.norm_pdf(y[k], x[0] * x[1] + k, 0.5) for k in range(4)]), _grid((T, 4)))
CASES['nd_refuse_too_many_measurement_columns'] = lambda: _call_l3(
    'central', 'tme_2', lambda y, x: stats.norm_pdf(y[6], x[0] * x[1], 0.5), _grid((T, 7)))
CASES['nd_refuse_likelihood_batch'] = lambda: _refuse_lik(
    lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-x[0] ** 3 + np.array([1., 0.5])))), _bits((B, T)))
CASES['nd_refuse_squeezed_ys_with_per_replicate_likelihood'] = lambda: _refuse_lik(
    lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-x[0] ** 3 + np.array([1., 0.5, 1.5])))))
CASES['nd_refuse_ys_rank_scalar'] = lambda: _refuse_lik(None, _bits((2, B, T, 2)))
CASES['nd_refuse_ys_rank_vector'] = lambda: _refuse_lik(_two_gauss, _grid((T,)))


@case('nd_refuse_tme_order_4_kappa')
def _():
    mi, inds, dt, gs, drift, disp, pmf = _pp()
    fns = mnd.sde_cond_moments_tme(drift, disp, dt, 4)
    return _pp_cms((fns[1], 'multi-index'), fns[3], None, _bits((T,)))


def _pp_degree(deg, family):
    mi, inds, dt, gs, _, disp, pmf = _pp()
    drift = lambda x: -x ** deg      # noqa: E731
    fns, sig = _pp_family(family, mi, dt, drift, disp)
    return fnd.moment_filter_nd_cms((fns[1], sig), fns[3], pmf, _bits((T,)), (mi, inds), gs.cms, gs.mean)


CASES['nd_refuse_extent_operator_16_rows'] = lambda: _pp_degree(4, 'tme_2')
CASES['nd_refuse_extent_operator_29_rows'] = lambda: _pp_degree(3, 'tme_3')
CASES['nd_refuse_extent_gaussian'] = lambda: _pp_degree(4, 'tme_normal_2')


@case('nd_refuse_batch_closures_batch')
def _():
    mi, inds, gs, pmf, fns = _pp_batch_closures((0.05, 0.1))
    return _call_nd('central', fns, 'multi-index', pmf, _bits((B, T)), mi, inds, gs.rms, gs.cms, gs.mean)


@case('nd_refuse_squeezed_ys_with_batch_closures')
def _():
    mi, inds, gs, pmf, fns = _pp_batch_closures()
    return _call_nd('central', fns, 'multi-index', pmf, _bits((T,)), mi, inds, gs.rms, gs.cms, gs.mean)


@case('nd_refuse_squeezed_ys_with_one_batched_table')
def _():
    mi, inds, gs, pmf, fns = _pp_batch_closures((0.05,))
    return _call_nd('central', fns, 'multi-index', pmf, _bits((T,)), mi, inds, gs.rms, gs.cms, gs.mean)


CASES['nd_refuse_squeezed_ys_with_one_batched_likelihood'] = lambda: _refuse_lik(
    lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-x[0] ** 3 + np.array([1.])))))


@case('nd_refuse_moment_count')
def _():
    fns = _pp_fns()
    mi, inds, dt, gs, *_ = _pp()
    return _pp_cms((fns[1], 'multi-index'), fns[3], None, _bits((T,)), ms0=gs.cms[:-1])


@case('nd_refuse_table_of_another_dimension')
def _():
    fns = _pp_fns()
    mi3 = gen_mi(3, 3)
    return _pp_cms((fns[1], 'multi-index'), fns[3], None, _bits((T,)), ms0=np.zeros(mi3.shape[0]),
                   order=(mi3, gen_inds(2, 3)))


@case('nd_refuse_unsupported_order_d2')
def _():
    fns = _pp_fns()
    mi = gen_mi(2, 15)
    return _pp_cms((fns[1], 'multi-index'), fns[3], None, _bits((T,)), ms0=np.zeros(mi.shape[0]), order=(mi, gen_inds(8, 2)))


CASES['nd_refuse_unsupported_order_d3'] = lambda: _call_l3('central', 'tme_2', _one, _grid((T,)), N=5)


@case('nd_refuse_d4')
def _():
    mi4, inds4 = gen_mi(4, 3), gen_inds(2, 4)
    fns = mnd.sde_cond_moments_tme(lambda x: -x, lambda x: np.eye(4).astype(object), 0.01, 1, d=4)
    return fnd.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], _one, _grid((T,)), (mi4, inds4), np.zeros(mi4.shape[0]),
                                    np.zeros(4))


@case('nd_refuse_ms0_batch')
def _():
    fns = _pp_fns()
    mi, inds, dt, gs, *_ = _pp()
    return _pp_cms((fns[1], 'multi-index'), fns[3], None, _bits((B, T)), ms0=np.tile(gs.cms, (B + 1, 1)))


CASES['nd_refuse_d1_two_factors'] = lambda: _call_d1(
    'central', _grid((T, 2)), lambda y, x: stats.norm_pdf(y[0], x, 1.) * stats.norm_pdf(y[1], x, 2.))
CASES['nd_refuse_bearing_at_d3'] = lambda: _call_l3(
    'central', 'tme_2', lambda y, x: stats.norm_pdf(y, sym.arctan2(x[1], x[0]), 0.3), _grid((B, T)))
CASES['nd_refuse_tme_order_3_at_d3'] = lambda: _call_l3('central', 'tme_3', _one, _grid((T,)))


@case('nd_refuse_extent_d3')
def _():
    mi, inds, dt, gs, _, disp, _ = _lorenz()
    fns = mnd.sde_cond_moments_tme(lambda x: -x ** 6, disp, dt, 1, d=3)
    return fnd.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], _one, _grid((T,)), (mi, inds), gs.cms, gs.mean)


@case('nd_refuse_extent_before_order_at_d3')
def _():
    mi, inds, dt, gs, _, disp, _ = _lorenz()
    fns = mnd.sde_cond_moments_tme(lambda x: -x ** 3, disp, dt, 3, d=3)
    return fnd.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], _one, _grid((T,)), (mi, inds), gs.cms, gs.mean)


@case('nd_refuse_order_before_extent_at_d2')
def _():
    mi, inds, dt, gs, _, disp, pmf = _pp()
    fns = mnd.sde_cond_moments_tme(lambda x: -x ** 3, disp, dt, 4)
    return fnd.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], pmf, _bits((T,)), (mi, inds), gs.cms, gs.mean)


@case('nd_refuse_batch_closures_batch_d3')
def _():
    mi, inds, dt, gs, drift, _, _ = _lorenz()
    per = [mnd.sde_cond_moments_tme(drift, lambda x, s=s: np.diag([s, s, s]).astype(object), dt, 2, d=3) for s in (0.1, 0.2)]
    return _call_nd('central', mnd.batch_closures(per), 'multi-index', _one, _grid((B, T)), mi, inds, gs.rms, gs.cms, gs.mean)


CASES['nd_refuse_joint_batch'] = lambda: _call_l3(
    'central', 'tme_2', stats.batch_likelihoods([lambda y, x, k=k: stats.norm_pdf(y, x[0] * x[1] + k, 0.5) for k in range(2)]),
    _grid((B, T)))
CASES['nd_refuse_squeezed_ys_with_per_replicate_joint'] = lambda: _call_l3(
    'central', 'tme_2', stats.batch_likelihoods([lambda y, x, k=k: stats.norm_pdf(y, x[0] * x[1] + k, 0.5) for k in range(B)]),
    _grid((T,)))


# ---------------------------------------------------------------------------------------------------------------------
# running the cases, the file
# ---------------------------------------------------------------------------------------------------------------------
def _store(out, key, a):
    """-> the JSON description of an array; arrays up to BIG elements also go to `out` under `key`."""
    a = np.asarray(a)
    desc = {'dtype': a.dtype.str, 'shape': list(a.shape)}
    if a.size > BIG:
        desc['sha256'] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    else:
        out[key] = np.ascontiguousarray(a)
    return desc


def record(monkeypatch):
    """Run every case under the recorder -> {key: array}: '<case>/meta' is a JSON text, the rest are the small arrays."""
    out = {}
    for name, fn in CASES.items():
        with monkeypatch.context() as mp:
            rec = install(mp)
            meta = {}
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter('always')
                try:
                    res = fn()
                    meta['returned'] = [_store(out, f'{name}/ret{k}', v) for k, v in enumerate(res)]
                except Exception as e:       # noqa: BLE001  (the refusals are part of the record)
                    meta['raised'] = [type(e).__name__, str(e)]
            meta['warnings'] = [[w.category.__name__, str(w.message)] for w in caught]
            meta['calls'] = [{'entry': entry, 'args': args,
                              'arrays': {k: _store(out, f'{name}/call{c}/{k}', v) for k, v in arrays.items()}}
                             for c, (entry, args, arrays) in enumerate(rec.calls)]
        out[f'{name}/meta'] = np.array(json.dumps(meta, sort_keys=True))
    return out


def check_coverage(rec):
    """Every case that returns made exactly one C call, only the cases named as refusals raise, and all entry points are
    reached, mfs_filter_1d also from the d = 1 route of the N-D filters."""
    reached = set()
    for name in CASES:
        meta = json.loads(str(rec[f'{name}/meta']))
        if 'returned' in meta:
            assert len(meta['calls']) == 1, (name, len(meta['calls']))
            reached.add((name.split('_')[0], meta['calls'][0]['entry']))
        else:
            assert '_refuse_' in name and not meta['calls'], (name, meta['raised'])
    assert {e for _, e in reached} == set(ENTRY_POINTS), reached
    assert ('nd1', 'mfs_filter_1d') in reached and ('1d', 'mfs_filter_1d') in reached


def write(path, arrays):
    """An .npz with fixed member timestamps (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[key], allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    import pytest
    rec = record(pytest.MonkeyPatch())
    check_coverage(rec)
    write(PATH, rec)
    refusals = sum('raised' in json.loads(str(rec[f'{n}/meta'])) for n in CASES)
    print(f'host_calls.npz: {len(CASES)} cases ({refusals} refusals), {os.path.getsize(PATH) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
