"""Cases, directions and the CPU reference for the NLL gradient kernel (C entry mfs_filter_1d_grad,
mfs_amd/csrc/filter1d_grad.hpp).

The entry point takes the table tangents `dcoef` / `dlik` as plain arrays, so a test may pass ANY direction in table space.  For
direction p the kernel's out_grad[b][p] must equal d/ds NLL(coef + s D_p, lik + s E_p) at s = 0.  Here D_p = coef * U_p and
E_p = lik * V_p with U_p, V_p uniform in [-1, 1], seeded from (model, mode, N, p): every non-zero entry of every table row moves
on its own (a tangent dropped for one row cannot hide behind the others), zeros stay zero.

Reference: the CPU C port of the filter (oracle.c_oracle.filter_1d) at s = +-h and +-2h, Richardson-combined as
(4 d_h - d_2h) / 3, all 4P + 1 table sets of every replicate in one batched call.  It shares no code with the device.
`reference_spread` is the condition the reference itself has to meet before a device result is held against it: the values at
h = 1e-3, 3e-4 and 1e-4 agree within SPREAD_BOUND of max_p |g_ref|.  tests/test_host_gradient_ref.py checks it for every case
of `ALL_CASES` without a GPU; tests/test_gpu_gradient_envelope.py runs the same list on the device."""
import ctypes as C
import dataclasses
import functools
import math
import zlib

import numpy as np

from mfs_amd import _lib, stats, sym, synth
from mfs_amd.one_dim import filtering, moments, ss_models
from mfs_amd.utils import GaussianSum1D
from oracle import c_oracle
from tests import brute_force_ref as R

MODES = ('raw', 'central', 'scaled')
STEPS = (1e-3, 3e-4, 1e-4)      # the three steps of the condition on the reference
H_REF = STEPS[1]                # ... and the one the device is held against
SPREAD_BOUND = 1e-7
GRAD_BOUND = 2e-6               # |g - g_ref| <= GRAD_BOUND max_p |g_ref| per replicate: the project's bound at N = 15
T_DEFAULT = 32
T_LONG = 300                    # the warm-start runs (the reference meets its condition there; see the host test)


def nell_rtol(N):
    """NLL against the C port and against the plain device kernel: the bounds tests/test_gpu_gradient.py uses at N = 5, 7, 15."""
    return 1e-9 if N <= 8 else 1e-8


def filters_per_wave(N):
    """A filter is a group of 8 lanes up to N = 8 and of 16 lanes above."""
    return 8 if N <= 8 else 4


# ---------------------------------------------------------------------------------------------------------------------
# models: tag -> closures of the shipped factories, initial law, measurements
# ---------------------------------------------------------------------------------------------------------------------
def _cubic_logistic_pmf(y, x):
    """Bernoulli-logistic with all four parameters non-zero (the shipped Benes model has the cubic term alone)."""
    return stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-(0.1 + 0.3 * x - 0.2 * x ** 2 + 0.2 * x ** 3))))


def _closures(model, N):
    """-> (the factory's five closures, measurement pdf, initial law, dt)."""
    if model in ('A', 'A2', 'C'):
        dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli(N)
        if model == 'A':
            return moments.sde_cond_moments_tme(drift, dispersion, dt, 3), pmf, ic, dt
        if model == 'A2':
            return moments.sde_cond_moments_tme(drift, dispersion, dt, 2), _cubic_logistic_pmf, ic, dt
        return moments.sde_cond_moments_tme_normal(drift, dispersion, dt, 3, N), _cubic_logistic_pmf, ic, dt
    if model in ('B', 'E'):
        dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.well_poisson(3., N)
        f = (moments.sde_cond_moments_tme_normal(lambda x: drift(x, 3.), dispersion, dt, 2, N) if model == 'B' else
             moments.sde_cond_moments_tme(lambda x: drift(x, 3.), dispersion, dt, 2))
        return f, (lambda y, x: pmf(y, x, 3.)), ic, dt
    if model == 'D':
        F, Sigma = math.exp(-R.OU_DT / R.OU_ELL), R.OU_SIGMA ** 2 * (1 - math.exp(-2 * R.OU_DT / R.OU_ELL))
        f = moments.sde_cond_moments_normal(lambda x: F * x, lambda x: Sigma + 0. * x, N)
        ic = GaussianSum1D.new(means=[0.], variances=[R.OU_SIGMA ** 2], weights=[1.], N=N)
        return f, (lambda y, x: stats.norm_pdf(y, x + 0.05, math.sqrt(R.OU_R))), ic, R.OU_DT
    raise ValueError(model)


@dataclasses.dataclass(frozen=True)
class Base:
    tables: object
    lik: object
    coef: np.ndarray        # (n_rows, J + 1)
    lp: np.ndarray          # (n_lik,)
    J: int
    m0: np.ndarray          # (2N,)
    mean0: float
    scale0: float
    dt: float


@functools.lru_cache(maxsize=None)
def base(model, mode, N):
    """The traced base point of (model, mode, N): traced once."""
    f, pmf, ic, dt = _closures(model, N)
    trans, mean_fn = {'raw': (f[0], None), 'central': (f[1], f[3]), 'scaled': (f[2], f[4])}[mode]
    tables, lik = filtering.trace_model(mode, trans, mean_fn, pmf)
    coef, J = tables.table(1)
    lp = np.ascontiguousarray(lik.params, dtype=np.float64)
    assert coef.ndim == 2 and lp.ndim == 1
    m0 = {'raw': ic.rms, 'central': ic.cms, 'scaled': ic.scms}[mode]
    for a in (coef, lp, m0):
        a.setflags(write=False)
    return Base(tables, lik, coef, lp, J, m0, float(ic.mean), math.sqrt(ic.variance), dt)


@functools.lru_cache(maxsize=None)
def measurements(model, B, T, seed):
    if model in ('A', 'A2', 'C'):
        ys = synth.benes_bernoulli_batch(B, T, 1e-2, seed=seed)[0]
    elif model in ('B', 'E'):
        ys = synth.well_poisson_batch(B, T, p1=3., p2=3., dt=1e-2, seed=seed)[0]
    else:
        ys = synth.ou_gaussian_batch(B, T, dt=R.OU_DT, ell=R.OU_ELL, sigma=R.OU_SIGMA, R=R.OU_R, seed=seed)[0]
    ys.setflags(write=False)
    return ys


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    model: str
    mode: str
    N: int
    P: int
    B: int
    T: int = T_DEFAULT
    coef_batched: bool = False
    lik_batched: bool = False
    m0_batched: bool = False
    seed: int = 3

    @property
    def id(self):
        flags = ''.join(c for c, on in zip('clm', (self.coef_batched, self.lik_batched, self.m0_batched)) if on)
        return f'{self.group}-{self.model}-{self.mode}-N{self.N}-P{self.P}-B{self.B}-T{self.T}' + (f'-{flags}' if flags else '')


# (measurement seed, T) of the cases whose reference does not meet its condition at the default seed and T = 32 (or T_LONG):
# the first seed in 0..23 at the longest T of 32, 16, 8, 4, 2, 1 (300, 150, 75 for the long runs) at which no replicate
# poisons in the C port and the spread stays below half of SPREAD_BOUND.  What shortens T: the well--Poisson NLL is strongly
# curved along a direction that moves the drift's linear coefficient by up to 0.1 % per step h; and a single Gaussian (model D)
# has the worst-conditioned Hankel matrices of all the models -- from N = 14 on the fp64 filter poisons within a few steps
# whatever the data, in the C port as on the device, so that only the first step can be held against a reference.
_RUNS = {
    ('matrix', 'B', 'raw', 2): (8, 32), ('matrix', 'B', 'raw', 3): (7, 32), ('matrix', 'B', 'raw', 9): (0, 32),
    ('matrix', 'B', 'raw', 15): (6, 16), ('matrix', 'B', 'raw', 16): (20, 32),
    ('matrix', 'B', 'central', 2): (4, 32), ('matrix', 'B', 'central', 3): (4, 32), ('matrix', 'B', 'central', 9): (0, 32),
    ('matrix', 'B', 'central', 15): (0, 32), ('matrix', 'B', 'central', 16): (0, 32),
    ('matrix', 'B', 'scaled', 2): (4, 32), ('matrix', 'B', 'scaled', 8): (1, 32), ('matrix', 'B', 'scaled', 15): (0, 32),
    ('matrix', 'B', 'scaled', 16): (0, 32),
    ('matrix', 'D', 'raw', 2): (0, 32), ('matrix', 'D', 'raw', 8): (0, 16), ('matrix', 'D', 'raw', 9): (7, 4),
    ('matrix', 'D', 'raw', 15): (0, 1), ('matrix', 'D', 'raw', 16): (0, 1),
    ('matrix', 'D', 'central', 2): (0, 32), ('matrix', 'D', 'central', 3): (0, 32), ('matrix', 'D', 'central', 8): (0, 32),
    ('matrix', 'D', 'central', 9): (0, 4), ('matrix', 'D', 'central', 15): (0, 1), ('matrix', 'D', 'central', 16): (0, 1),
    ('matrix', 'D', 'scaled', 2): (0, 32), ('matrix', 'D', 'scaled', 3): (0, 32), ('matrix', 'D', 'scaled', 8): (0, 32),
    ('matrix', 'D', 'scaled', 9): (12, 32), ('matrix', 'D', 'scaled', 15): (0, 1), ('matrix', 'D', 'scaled', 16): (0, 1),
    ('matrix', 'E', 'raw', 8): (20, 32), ('matrix', 'E', 'raw', 9): (22, 32), ('matrix', 'E', 'central', 9): (0, 32),
    ('matrix', 'E', 'scaled', 8): (0, 32), ('matrix', 'E', 'scaled', 9): (0, 32),
    ('long', 'A', 'central', 9): (7, 300), ('long', 'A', 'central', 16): (0, 75),
}


def _case(group, model, mode, N, P, B, T=T_DEFAULT, **kw):
    seed, T = _RUNS.get((group, model, mode, N), (kw.pop('seed', 3), T))
    return Case(group, model, mode, N, P, B, T=T, seed=seed, **kw)


def _no_rule(model, N):
    """The TME-2 operator tables of the well's cubic drift (model E) predict, from the initial law, a moment sequence whose
    Hankel matrix is not positive definite at N = 15 and 16: the filter poisons in its first step whatever the measurements,
    so there is no gradient to test -- these orders are held to that documented outcome instead (POISON_AT_START)."""
    return model == 'E' and N >= 15


EVERY_INSTANTIATION = [_case('inst', 'A', 'central', N, P, 3) for N in range(2, 17) for P in range(1, 5)]
MATRIX_N = (2, 3, 8, 9, 15, 16)
MATRIX = [_case('matrix', m, mode, N, 2, 3) for m in ('A2', 'B', 'C', 'D', 'E') for mode in MODES for N in MATRIX_N
          if not _no_rule(m, N)]
POISON_AT_START = [Case('nan0', 'E', mode, N, 2, 3) for mode in MODES for N in MATRIX_N if _no_rule('E', N)]
BATCHING = [_case('flags', 'B', 'central', N, 2, 5, coef_batched=cb, lik_batched=lb, seed=23)
            for N in (7, 9) for cb in (False, True) for lb in (False, True)] + \
           [_case('flags', 'B', 'scaled', N, 2, 5, m0_batched=True, seed=23) for N in (7, 9)]
GEOMETRY_N = (8, 9, 16)


def geometry_batches(N):
    fpw = filters_per_wave(N)
    return (1, fpw - 1, fpw, fpw + 1, 2 * fpw + 3)


GEOMETRY = [_case('geom', 'A', 'central', N, 2, geometry_batches(N)[-1], seed=13) for N in GEOMETRY_N]
LONG = [_case('long', m, 'central', N, 2, 2, T=T_LONG) for m in ('A', 'B') for N in (8, 9, 16)]
ALL_CASES = EVERY_INSTANTIATION + MATRIX + BATCHING + GEOMETRY + LONG      # every case that is held against the reference


# ---------------------------------------------------------------------------------------------------------------------
# inputs of a case: tables, directions, initial law, measurements
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Inputs:
    coef: np.ndarray        # (B, n_rows, J + 1): replicate b's tables (equal rows unless coef_batched)
    lp: np.ndarray          # (B, n_lik)
    dcoef: np.ndarray       # (B, P, n_rows, J + 1)
    dlik: np.ndarray        # (B, P, n_lik)
    m0: np.ndarray          # (B, 2N)
    mean0: np.ndarray       # (B,)
    scale0: np.ndarray      # (B,)
    ys: np.ndarray          # (B, T)


def _direction_rng(case, p):
    return np.random.default_rng([zlib.crc32(f'{case.model}/{case.mode}'.encode()), case.N, p])


@functools.lru_cache(maxsize=None)
def inputs(case):
    bs = base(case.model, case.mode, case.N)
    B, P = case.B, case.P
    grow = 1. + 0.02 * np.arange(B)
    coef = np.repeat(bs.coef[None], B, axis=0) * (grow[:, None, None] if case.coef_batched else 1.)
    lp = np.repeat(bs.lp[None], B, axis=0) * (grow[:, None] if case.lik_batched else 1.)
    dcoef, dlik = np.empty((B, P) + bs.coef.shape), np.empty((B, P) + bs.lp.shape)
    for p in range(P):
        rng = _direction_rng(case, p)
        U = rng.uniform(-1., 1., ((B if case.coef_batched else 1),) + bs.coef.shape)
        V = rng.uniform(-1., 1., ((B if case.lik_batched else 1),) + bs.lp.shape)
        dcoef[:, p] = coef * U
        dlik[:, p] = lp * V
    m0 = np.repeat(bs.m0[None], B, axis=0)
    mean0, scale0 = np.full((B,), bs.mean0), np.full((B,), bs.scale0)
    if case.m0_batched:
        mean0 = mean0 + 0.01 * np.arange(B)
        scale0 = scale0 * grow
    ys = measurements(case.model, B, case.T, case.seed)
    out = Inputs(coef, lp, dcoef, dlik, m0, mean0, scale0, ys)
    for a in dataclasses.astuple(out):
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the C-port reference
# ---------------------------------------------------------------------------------------------------------------------
def _kinds(bs):
    return (_lib.TRANS[bs.tables.kind], _lib.UMAP[bs.tables.umap], bs.tables.n_terms, bs.tables.mean_x_coef,
            _lib.LIK[bs.lik.kind])


def cport_nell(case, coef, lp, m0, mean0, scale0, ys):
    """NLL of the C port, one table set / initial law / measurement row per replicate (leading axis everywhere)."""
    bs = base(case.model, case.mode, case.N)
    kind, umap, K, mxc, lik_kind = _kinds(bs)
    return c_oracle.filter_1d(MODES.index(case.mode), case.N, ys, m0, mean0, scale0, kind, umap, K, coef, mxc, lik_kind, lp,
                              want_moments=False)[3]


def reference_at(case, h):
    """-> (nell (B,), grad (B, P)) of the C port: Richardson-combined central differences of steps h and 2h."""
    x = inputs(case)
    B, P = case.B, case.P
    offs = np.array([0.] + [s * h for _ in range(P) for s in (1., -1., 2., -2.)])         # (4P + 1,)
    sel = np.zeros((4 * P + 1, P))
    for p in range(P):
        sel[1 + 4 * p:5 + 4 * p, p] = 1.
    w = offs[:, None] * sel                                                                  # (S, P): the s of each table set
    coef = x.coef[:, None] + np.einsum('sp,bp...->bs...', w, x.dcoef)                        # (B, S, rows, J + 1)
    lp = x.lp[:, None] + np.einsum('sp,bp...->bs...', w, x.dlik)
    S = 4 * P + 1
    rep = lambda a: np.repeat(a, S, axis=0)                                                  # noqa: E731
    v = cport_nell(case, coef.reshape((B * S,) + coef.shape[2:]), lp.reshape(B * S, -1), rep(x.m0), rep(x.mean0),
                   rep(x.scale0), rep(x.ys)).reshape(B, S)
    q = v[:, 1:].reshape(B, P, 4)
    d1, d2 = (q[..., 0] - q[..., 1]) / (2 * h), (q[..., 2] - q[..., 3]) / (4 * h)
    return v[:, 0].copy(), (4. * d1 - d2) / 3.


@functools.lru_cache(maxsize=None)
def reference(case):
    nell, grad = reference_at(case, H_REF)
    nell.setflags(write=False)
    grad.setflags(write=False)
    return nell, grad


def reference_spread(case):
    """-> (B,): max over directions and pairs of steps of |g_h - g_h'|, over max_p |g_ref|, per replicate."""
    g = np.stack([reference_at(case, h)[1] for h in STEPS])                                  # (3, B, P)
    assert np.all(np.isfinite(g)), f'{case.id}: the C port poisons'
    return (g.max(axis=0) - g.min(axis=0)).max(axis=-1) / np.abs(reference(case)[1]).max(axis=-1)


# ---------------------------------------------------------------------------------------------------------------------
# the device, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _model_struct(case, coef, lp, coef_batched, lik_batched):
    bs = base(case.model, case.mode, case.N)
    coef = np.ascontiguousarray(coef if coef_batched else coef[0])
    lp = np.ascontiguousarray(lp if lik_batched else lp[0])
    return filtering.fill_model_struct(bs.tables, bs.lik, bs.J, coef, lp, coef_batched, lik_batched)


def _start(m0, mean0, scale0, m0_batched):
    if m0_batched:
        return tuple(np.ascontiguousarray(a) for a in (m0, mean0, scale0))
    return tuple(np.ascontiguousarray(a) for a in (m0[0], mean0[:1], scale0[:1]))


def device_grad_raw(case, x, rows=None, coef_batched=None, lik_batched=None, m0_batched=None):
    """mfs_filter_1d_grad on replicates `rows` of the inputs `x` -> (rc, nell, grad, first_nan).  The batching flags
    default to the case's; a flag that is off passes replicate rows[0]'s array as the shared one."""
    rows = np.arange(x.ys.shape[0]) if rows is None else np.atleast_1d(rows)
    cb = case.coef_batched if coef_batched is None else coef_batched
    lb = case.lik_batched if lik_batched is None else lik_batched
    mb = case.m0_batched if m0_batched is None else m0_batched
    m, keep = _model_struct(case, x.coef[rows], x.lp[rows], cb, lb)
    dcoef = np.ascontiguousarray(x.dcoef[rows] if cb else x.dcoef[rows[0]])
    dlik = np.ascontiguousarray(x.dlik[rows] if lb else x.dlik[rows[0]])
    m0, mean0, scale0 = _start(x.m0[rows], x.mean0[rows], x.scale0[rows], mb)
    ys = np.ascontiguousarray(x.ys[rows])
    B, T = ys.shape
    P = x.dcoef.shape[1]
    nell, grad, fn = np.full((B,), -7.), np.full((B, P), -7.), np.full((B,), -7, dtype=np.int32)
    rc = _lib.lib().mfs_filter_1d_grad(C.byref(m), _lib.ptr(dcoef), _lib.ptr(dlik), P, _lib.MODE[case.mode], case.N, T, B,
                                       _lib.ptr(m0), int(mb), _lib.ptr(mean0), _lib.ptr(scale0), _lib.ptr(ys),
                                       _lib.ptr(nell), _lib.ptr(grad), _lib.ptr(fn), 0, None)
    del keep
    return rc, nell, grad, fn


def device_grad(case, x=None, **kw):
    rc, nell, grad, fn = device_grad_raw(case, inputs(case) if x is None else x, **kw)
    _lib.check(rc)
    return nell, grad, fn


def device_plain(case, x=None):
    """The plain filter kernel (mfs_filter_1d) on the same model struct -> (nell, first_nan)."""
    x = inputs(case) if x is None else x
    m, keep = _model_struct(case, x.coef, x.lp, case.coef_batched, case.lik_batched)
    m0, mean0, scale0 = _start(x.m0, x.mean0, x.scale0, case.m0_batched)
    ys = np.ascontiguousarray(x.ys)
    B, T = ys.shape
    nell, fn = np.empty((B,)), np.empty((B,), dtype=np.int32)
    _lib.check(_lib.lib().mfs_filter_1d(C.byref(m), _lib.MODE[case.mode], case.N, T, B, _lib.ptr(m0), int(case.m0_batched),
                                        _lib.ptr(mean0), _lib.ptr(scale0), _lib.ptr(ys), 0, None, None, None,
                                        _lib.ptr(nell), _lib.ptr(fn), 0, None))
    del keep
    return nell, fn
