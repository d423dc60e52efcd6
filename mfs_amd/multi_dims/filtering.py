"""The N-D moment filters on MI355X, mirroring `mfs.multi_dims.filtering`.

Same names, positional order and return tuples as the reference (mfs/multi_dims/filtering.py:283-288, 210-217,
33-41); both closure signatures ('multi-index' for sde_cond_moments_tme, 'index' for the Normal closures, :245-249).
d = 2 runs on `filternd_kernel` (mfs_amd/csrc/filternd_kernel.hpp), d = 3 on `filternd3_kernel` (filternd3_kernel.hpp, N = 2..4,
TME order <= 2 operator tables or a Normal closure, likelihood factors of one component each and / or joint factors of all
three components); d = 1 is routed to the 1-D kernels (the reference
guarantees the d = 1 N-D path equals the 1-D path, tests/test_filtering.py:304-329).  Extensions over the reference:
`ys` may carry a leading replicate axis -- (B, T) for scalar measurements, (B, T, ny) for vector ones -- initial
moments may be (z,) shared or (B, z), model parameters may be per-replicate.  No CPU fallback.

The measurement likelihood must be a product of factors, each a function of ONE state component and one measurement
column: `bernoulli.pmf(y, logistic(x[0]))` (mfs/multi_dims/ss_models.py:63-67) or
`math.prod(norm.pdf(y, x, sd))` on vector y, x (reference tests/test_filtering.py:44-46).  At d = 3 a factor may also read
all three components: `norm_pdf(y, x[0] * x[1], sd)`, `norm_pdf(y[0], sym.sqrt(p), sd)`, `norm_pdf(y[1], sym.arctan2(p, q), sd)`
with p, q polynomials of per-variable degree <= 3 (include/mfs_hip.h, mfs_joint_nd3); up to 3 of them multiply the others.
"""
import ctypes as C
from typing import Callable, NamedTuple, Tuple

import numpy as np

from mfs_amd import _lib, sym
from mfs_amd.multi_dims.moments import TransitionRefND

__all__ = ['moment_filter_nd_rms', 'moment_filter_nd_cms', 'moment_filter_nd_scms']


def _trace_transition(fn_and_flag, mode, moments_partial_order=None):
    fn, signature = fn_and_flag
    if signature not in ('multi-index', 'index'):
        raise sym.NotDeviceDescribable(f"unknown transition-moment signature {signature!r}")
    second = sym.ORDER
    if mode == 'raw':
        ref = fn(sym.X, second)
        ok = isinstance(ref, TransitionRefND) and ref.mean is None
    elif mode == 'scaled':
        ref = fn(sym.X, second, sym.MEAN, sym.SCALE)
        ok = isinstance(ref, TransitionRefND) and ref.mean is sym.MEAN and ref.scale is sym.SCALE
    else:
        ref = fn(sym.X, second, sym.MEAN)
        ok = isinstance(ref, TransitionRefND) and ref.mean is sym.MEAN
    if not isinstance(ref, TransitionRefND):
        raise sym.NotDeviceDescribable('the transition-moment callable is not device-describable; build it with '
                                       'mfs_amd.multi_dims.moments.sde_cond_moments_tme / _tme_normal / '
                                       '_euler_maruyama')
    if not ok:
        raise sym.NotDeviceDescribable('the transition-moment callable does not forward its mean / scale arguments')
    gaussian = ref.tables.is_gaussian
    if gaussian != (signature == 'index'):
        raise sym.NotDeviceDescribable(f"signature {signature!r} does not match the closure: the Normal closures take "
                                       "'index', sde_cond_moments_tme takes 'multi-index' "
                                       '(mfs/multi_dims/filtering.py:245-249)')
    if gaussian and moments_partial_order is not None:
        # an 'index' closure looks moments up in the table it was built for (mfs/multi_dims/moments.py:293-300)
        built_for = np.asarray(fn.multi_indices)
        if built_for.shape != np.asarray(moments_partial_order[0]).shape or \
                np.any(built_for != np.asarray(moments_partial_order[0])):
            raise ValueError("the 'index' closure was built for a different multi-index table than the filter's")
    return ref.tables


def _trace_likelihood(fn, d):
    """Call the measurement model with the measurement placeholder and the d tagged state components; returns the list
    of likelihood factors (each with .component and .ycol)."""
    xs = sym.state_vector(d)
    spec = fn(sym.Y, xs if d > 1 else xs[0])
    if isinstance(spec, sym.LikelihoodVector):
        if len(spec) == 1:
            spec = spec.factors[0]
        else:
            raise sym.NotDeviceDescribable('measurement_cond_pdf returned one value per component; reduce it with '
                                           'math.prod(...) as the reference does (tests/test_filtering.py:44-46)')
    if not isinstance(spec, (sym.LikelihoodSpec, sym.LikelihoodProduct)):
        raise sym.NotDeviceDescribable(
            f'measurement_cond_pdf returned {type(spec).__name__} when traced; use mfs_amd.stats.bernoulli_pmf / '
            'poisson_pmf / norm_pdf with mfs_amd.sym.exp / log (mfs_amd has no CPU path for arbitrary callables)')
    factors = spec.factors
    joint = [f for f in factors if isinstance(f, sym.JointLikelihoodSpec)]
    if joint and d != 3:
        raise sym.NotDeviceDescribable('joint polynomial likelihood factors run at d = 3 only')
    if len(joint) > _lib.ND3_MAX_JOINT:
        raise sym.NotDeviceDescribable(f'{len(joint)} joint likelihood factors; the device takes at most {_lib.ND3_MAX_JOINT}')
    most = _lib.ND3_MAX_FACTORS if d == 3 else _lib.ND_MAX_FACTORS
    single = len(factors) - len(joint)
    if not (0 if joint else 1) <= single <= most:
        raise sym.NotDeviceDescribable(f'{single} likelihood factors; the device takes 1..{most}')
    return factors


class _Layout(NamedTuple):
    """What differs between the d = 2 and d = 3 model descriptors (include/mfs_hip.h: mfs_model_nd, mfs_model_nd3)."""
    d: int
    struct: type
    kappas: list                # derivative multi-indices in the row order of the operator table
    max_order: int              # the TME order whose terms that list holds
    gauss_terms: int            # polynomials of a Normal closure: d means + d (d + 1) / 2 covariances
    fixed_terms: int            # n_terms of an operator table; 0: as many as the table uses
    max_extent: dict            # rows of the table (the d variance rows of scaled mode last) -> largest coefficient extent


_LAYOUTS = {
    2: _Layout(2, _lib.MfsModelNd, _lib.ND_KAPPAS, 3, 5, 0,
               {_lib.ND_ROWS: _lib.ND_MAX_EXTENT, _lib.ND_ROWS_MAX: _lib.ND_MAX_EXTENT_HI}),
    3: _Layout(3, _lib.MfsModelNd3, _lib.ND3_KAPPAS, 2, _lib.ND3_GAUSS_TERMS, _lib.ND3_TERMS,
               {_lib.ND3_ROWS: _lib.ND3_MAX_EXTENT}),
}
# the refusals' wording, kept as it was when each dimension had its own builder
_KAPPA_REFUSAL = {2: 'on the device', 3: 'at d = 3'}
_EXTENT_REFUSAL = {(2, True): 'MFS_ND_MAX_EXTENT = {}', (3, True): 'MFS_ND3_MAX_EXTENT = {}', (3, False): 'MFS_ND3_MAX_EXTENT = {}'}


def _lead(what, batched_over, B):
    """Leading axis of a table: () when shared, (B,) when per-replicate -- `batched_over` lists the replicate counts found."""
    for n in batched_over:
        if n != B:
            raise ValueError(f'{what} are batched over {n} replicates, the filter batch is {B}')
    return (B,) if batched_over else ()


def _attach(struct, **tables):
    """Point the named fields of a descriptor at C-contiguous tables -> (struct, tables): the struct holds raw pointers, so
    the caller keeps the tuple referenced until the C call has returned."""
    keep = tuple(np.ascontiguousarray(t) for t in tables.values())
    for name, t in zip(tables, keep):
        setattr(struct, name, t.ctypes.data_as(_lib.c_double_p))
    return struct, keep


def _lik_params(factors, B):
    """[n_factors][MAX_LIK], or [B][n_factors][MAX_LIK] when a factor has per-replicate parameters -> (array, batched)."""
    nf = len(factors)
    lik_batched = any(np.asarray(f.params).ndim > 1 for f in factors)
    lp = np.zeros(((B,) if lik_batched else ()) + (nf, _lib.MAX_LIK))
    for i, f in enumerate(factors):
        prm = np.asarray(f.params, dtype=np.float64)
        if prm.ndim > 2 or (prm.ndim == 2 and prm.shape[0] != B):
            raise ValueError(f'likelihood parameters are batched with shape {prm.shape[:-1]}, the filter batch is {B}')
        lp[..., i, :prm.shape[-1]] = prm
    return lp, lik_batched


def _build_model(L, tables, factors, B, ny=None):
    """The model descriptor of layout `L` from a transition family and the single-component factors of its likelihood."""
    d = L.d
    dense, D = tables.dense_table()         # (B?, terms, D, .., D): a leading axis for per-replicate drift / dispersion
    lead = _lead('transition tables', [dense.shape[0]] if dense.ndim == d + 2 else [], B)

    def flat(a):                            # the d coefficient axes as one
        return a.reshape(a.shape[:-d] + (-1,))

    def check_extent(n_rows):
        if D > L.max_extent[n_rows]:
            limit = _EXTENT_REFUSAL.get((d, tables.is_gaussian), 'the device limit {}').format(L.max_extent[n_rows])
            raise sym.NotDeviceDescribable(f'coefficient extent {D} exceeds {limit}')

    one_layout = len(L.max_extent) == 1
    if one_layout:                          # the limit does not wait for the row count
        check_extent(*L.max_extent)
    if tables.is_gaussian:
        kind, n_terms, rows_of = _lib.ND_TRANS_GAUSSIAN, L.gauss_terms, range(L.gauss_terms)   # means, then covariances
    else:
        kind, rows_of = _lib.ND_TRANS_OPERATOR, []
        for kap in tables.kappas:
            kap = tuple(int(v) for v in kap)
            if kap not in L.kappas:
                raise sym.NotDeviceDescribable(f'derivative term {kap} needs |kappa| <= {2 * L.max_order}, i.e. tme_order <= '
                                               f'{L.max_order} {_KAPPA_REFUSAL[d]}')
            rows_of.append(L.kappas.index(kap))
        n_terms = L.fixed_terms or max(rows_of, default=-1) + 1
    # d = 2 chooses the 16-row (|kappa| <= 4) or the 29-row layout (TME order 3) by the terms the table uses
    n_rows = next(iter(L.max_extent)) if one_layout else _lib.nd_table_rows(n_terms)
    check_extent(n_rows)
    coef = np.zeros(lead + (n_rows,) + (D,) * d)
    for t, row in enumerate(rows_of):
        flat(coef)[..., row, :] = flat(dense)[..., t, :]
    if not tables.is_gaussian:
        flat(coef)[..., n_rows - d:, :] = flat(tables.var_blocks(D))   # diagonal of tme.mean_and_cov (scaled mode)
    lp, lik_batched = _lik_params(factors, B)
    m = L.struct()
    if hasattr(m, 'd'):
        m.d = d
    m.trans_kind, m.n_terms, m.extent = kind, n_terms, D
    m.n_factors = len(factors)
    m.ny = max(f.ycol for f in factors) + 1 if ny is None else ny
    for i, f in enumerate(factors):
        m.fac_kind[i], m.fac_component[i], m.fac_ycol[i] = _lib.LIK[f.kind], int(f.component), int(f.ycol)
        m.fac_n_par[i] = int(np.asarray(f.params).shape[-1])
    m.coef_batched, m.lik_batched = int(bool(lead)), int(lik_batched)
    return _attach(m, coef=coef, lik=lp)


def _model_struct(tables, factors, B=1):
    """mfs_model_nd of a d = 2 transition family and its likelihood factors -> (struct, (coef, lik))."""
    if tables.d != 2:
        raise sym.NotDeviceDescribable('the device N-D kernel is for d = 2')
    if isinstance(factors, sym.LikelihoodSpec):
        factors = [factors]
    return _build_model(_LAYOUTS[2], tables, factors, B)


def _model_struct3(tables, factors, B=1, ny=None):
    """mfs_model_nd3 of a d = 3 transition family and the single-component factors of its likelihood (include/mfs_hip.h);
    `ny` when joint factors (_joint_struct3) read further measurement columns."""
    if isinstance(factors, sym.LikelihoodSpec):
        factors = [factors]
    for f in factors:
        if f.kind == 'bearing_gaussian' or int(f.component) not in (0, 1, 2):
            raise sym.NotDeviceDescribable('at d = 3 every likelihood factor reads one state component (no joint factors)')
    return _build_model(_LAYOUTS[3], tables, factors, B, ny)


def _joint_struct3(joints, B=1):
    """mfs_joint_nd3 of the joint factors of a d = 3 likelihood (include/mfs_hip.h)."""
    lead = _lead('joint likelihood factors', [f.coef.shape[0] for f in joints if f.coef.ndim > 4], B)
    E = max(f.coef.shape[-1] for f in joints)
    if E > _lib.ND3_JOINT_MAX_EXTENT:
        raise sym.NotDeviceDescribable(f'joint polynomial extent {E} exceeds MFS_ND3_JOINT_MAX_EXTENT = '
                                       f'{_lib.ND3_JOINT_MAX_EXTENT}')
    coef, par = np.zeros(lead + (len(joints), 2, E, E, E)), np.zeros(lead + (len(joints),))
    j = _lib.MfsJointNd3()
    j.n_joint, j.extent, j.batched = len(joints), E, int(bool(lead))
    for i, f in enumerate(joints):
        e = f.coef.shape[-1]
        coef[..., i, :, :e, :e, :e] = f.coef
        par[..., i] = f.params[..., 0]
        j.kind[i], j.link[i], j.ycol[i] = _lib.LIK[f.kind], _lib.ND3_LINK[f.link], int(f.ycol)
    return _attach(j, coef=coef, par=par)


def _split_ys(ys, ny):
    """-> (ys (B, T, ny) contiguous float64, squeeze): (T,) / (B, T) for scalar measurements, (T, ny) / (B, T, ny) for
    vector ones (the reference's ys_2d is (T, 2))."""
    ys = np.asarray(ys, dtype=np.float64)
    if ny == 1:
        if ys.ndim == 3 and ys.shape[-1] == 1:
            ys = ys[..., 0]
        if ys.ndim not in (1, 2):
            raise ValueError(f'ys must have shape (T,) or (B, T) for scalar measurements, got {ys.shape}')
        squeeze = ys.ndim == 1
        ys3 = (ys[None, :] if squeeze else ys)[..., None]
    else:
        if ys.ndim not in (2, 3) or ys.shape[-1] < ny:
            raise ValueError(f'ys must have shape (T, {ny}) or (B, T, {ny}) for this likelihood, got {ys.shape}')
        squeeze = ys.ndim == 2
        ys3 = (ys[None] if squeeze else ys)[..., :ny]
    return np.ascontiguousarray(ys3), squeeze


def _run_1d(mode, tables, factors, ys, ms0, mean0, scale0, stable, device):
    """d = 1: the N-D filter IS the 1-D filter (reference tests/test_filtering.py:304-329) -- run the 1-D kernels, without
    the component axis of mean0 / scale0 on the way in and with it on means / scales on the way out."""
    from mfs_amd.one_dim import filtering as f1
    t1 = tables.as_one_dim()
    if len(factors) != 1:
        raise sym.NotDeviceDescribable('a d = 1 filter takes a single likelihood factor')
    ys = np.asarray(ys, dtype=np.float64)
    if ys.ndim >= 2 and ys.shape[-1] == 1:
        ys = ys[..., 0]
    m0 = None if mean0 is None else np.asarray(mean0, dtype=np.float64)[..., 0]
    s0 = None if scale0 is None else np.asarray(scale0, dtype=np.float64)[..., 0]
    (m, means, scales, nell, fn), squeeze = f1._run(mode, t1, factors[0], ms0, m0, s0, ys, stable, device)
    return (m, None if means is None else means[..., None], None if scales is None else scales[..., None], nell, fn), squeeze


def _resolve_shape(d, factors, ys, inds, ms0):
    """Validate a d = 2, 3 call against what the device runs -> (N, B, T, batched, ny, ys (B, T, ny), squeeze)."""
    s = inds.shape[1]
    if d == 3:
        N = next((n for n in range(_lib.ND3_MIN_N, _lib.ND3_MAX_N + 1) if n * (n + 1) * (n + 2) // 6 == s), None)
        if N is None:
            raise sym.NotDeviceDescribable(f'the device d = 3 path supports {_lib.ND3_MIN_N} <= N <= {_lib.ND3_MAX_N} '
                                           f'(got s = {s})')
    else:
        N = next((n for n in range(2, 8) if n * (n + 1) // 2 == s), None)
        if d != 2 or N is None:
            raise sym.NotDeviceDescribable(f'the device N-D path supports d <= 3 with 2 <= N <= 7 at d = 2, 2 <= N <= 4 '
                                           f'at d = 3 (got d = {d}, s = {s})')
    ny = max(f.ycol for f in factors) + 1
    if ny > _lib.ND3_JOINT_MAX_NY and any(isinstance(f, sym.JointLikelihoodSpec) for f in factors):
        raise sym.NotDeviceDescribable(f'{ny} measurement columns; the device takes at most {_lib.ND3_JOINT_MAX_NY}')
    ys3, squeeze = _split_ys(ys, ny)
    B, T = ys3.shape[:2]
    batched = ms0.ndim == 2
    if batched and ms0.shape[0] != B:
        raise ValueError(f'initial moments batch {ms0.shape[0]} does not match ys batch {B}')
    return N, B, T, batched, ny, ys3, squeeze


def _descriptors(d, tables, factors, B, ny, squeeze):
    """-> (the byref arguments that open the C call, the arrays they point into)."""
    joints = [f for f in factors if isinstance(f, sym.JointLikelihoodSpec)]     # d = 3 only (_trace_likelihood)
    if joints:
        model, keep = _model_struct3(tables, [f for f in factors if f not in joints], B, ny=ny)
        joint, keep_joint = _joint_struct3(joints, B)
        head, keep = (model, joint), keep + keep_joint
    else:
        model, keep = (_model_struct3 if d == 3 else _model_struct)(tables, factors, B)
        head = (model,)
    if squeeze and (model.coef_batched or model.lik_batched or (joints and joint.batched)):
        raise ValueError('per-replicate model parameters need ys with a leading replicate axis')
    return head, keep


def _run_nd(mode, tables, factors, ys, moments_partial_order, ms0, mean0, stable, device, scale0=None):
    """-> ((moments, means, scales, nell, first_nan) with the replicate axis, None where `mode` has none; squeeze)."""
    multi_indices, inds = moments_partial_order
    multi_indices = np.asarray(multi_indices)
    ms0 = np.ascontiguousarray(ms0, dtype=np.float64)
    if multi_indices.shape[0] != ms0.shape[-1]:  # the reference's only raise (mfs/multi_dims/filtering.py:238-239)
        raise ValueError(f'The size of multi_indices {multi_indices.shape[0]} must match that of cms0 {ms0.shape[-1]}.')
    d = multi_indices.shape[-1]
    if d != tables.d:
        raise ValueError(f'the transition closure is {tables.d}-dimensional, the multi-index table {d}-dimensional')
    if d == 1:
        return _run_1d(mode, tables, factors, ys, ms0, mean0, scale0, stable, device)
    inds = np.asarray(inds)
    N, B, T, batched, ny, ys3, squeeze = _resolve_shape(d, factors, ys, inds, ms0)
    z = multi_indices.shape[0]

    def start(v, wanted):                   # mean0 / scale0 as (d,) or (B, d) like the initial moments
        shape = (B, d) if batched else (d,)
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shape)) if wanted else None

    mean_a, scale_a = start(mean0, mode != 'raw'), start(scale0, mode == 'scaled')
    head, keep = _descriptors(d, tables, factors, B, ny, squeeze)
    mi32 = np.ascontiguousarray(multi_indices, dtype=np.int32)
    inds32 = np.ascontiguousarray(inds, dtype=np.int32)
    out_m = _lib.pinned_empty((B, T, z), device=device)
    out_mean = _lib.pinned_empty((B, T, d), device=device) if mode != 'raw' else None
    out_scale = _lib.pinned_empty((B, T, d), device=device) if mode == 'scaled' else None
    out_nell, out_fn = np.empty((B,)), np.empty((B,), dtype=np.int32)
    L = _lib.lib()
    entry = L.mfs_filter_nd3_joint if len(head) == 2 else L.mfs_filter_nd3 if d == 3 else L.mfs_filter_nd
    _lib.check(entry(*(C.byref(h) for h in head), _lib.MODE[mode], N, T, B, z, _lib.ptr(mi32), _lib.ptr(inds32),
                     _lib.ptr(ms0), int(batched), _lib.ptr(mean_a), _lib.ptr(scale_a), _lib.ptr(ys3),
                     int(bool(stable)), _lib.ptr(out_m), _lib.ptr(out_mean), _lib.ptr(out_scale),
                     _lib.ptr(out_nell), _lib.ptr(out_fn), device, None))
    del keep
    return (out_m, out_mean, out_scale, out_nell, out_fn), squeeze


def moment_filter_nd_rms(state_cond_raw_moments: Tuple[Callable, str], measurement_cond_pdf: Callable, ys,
                         moments_partial_order, rms0, stable: bool = False, *, device: int = 0,
                         return_first_nan: bool = False):
    """Filtering with raw moments (mfs/multi_dims/filtering.py:283-344): returns (rmss (T, z), nell)."""
    tables = _trace_transition(state_cond_raw_moments, 'raw', moments_partial_order)
    lik = _trace_likelihood(measurement_cond_pdf, tables.d)
    return _lib.shape_outputs(*_run_nd('raw', tables, lik, ys, moments_partial_order, rms0, None, stable, device),
                              return_first_nan)


def moment_filter_nd_cms(state_cond_central_moments: Tuple[Callable, str], state_cond_mean: Callable,
                         measurement_cond_pdf: Callable, ys, moments_partial_order, cms0, mean0,
                         stable: bool = False, *, device: int = 0, return_first_nan: bool = False):
    """Filtering with central moments (mfs/multi_dims/filtering.py:210-280): returns (cmss, means (T, d), nell)."""
    tables = _trace_transition(state_cond_central_moments, 'central', moments_partial_order)
    ref = state_cond_mean(sym.X)
    if not (isinstance(ref, TransitionRefND) and ref.tables is tables):
        raise sym.NotDeviceDescribable('state_cond_mean must come from the same sde_cond_moments_* call as the '
                                       'conditional central moments')
    lik = _trace_likelihood(measurement_cond_pdf, tables.d)
    return _lib.shape_outputs(*_run_nd('central', tables, lik, ys, moments_partial_order, cms0, mean0, stable, device),
                              return_first_nan)


def moment_filter_nd_scms(state_cond_scms: Tuple[Callable, str], state_cond_mean_vars: Callable,
                          measurement_cond_pdf: Callable, ys, moments_partial_order, scms0, mean0, scale0,
                          stable: bool = False, *, device: int = 0, return_first_nan: bool = False):
    """Filtering with scaled central moments (mfs/multi_dims/filtering.py:33-207): returns
    (scmss (T, z), means (T, d), scales (T, d), nell)."""
    tables = _trace_transition(state_cond_scms, 'scaled', moments_partial_order)
    ref = state_cond_mean_vars(sym.X)
    if not (isinstance(ref, TransitionRefND) and ref.tables is tables and ref.which == 'mean_var'):
        raise sym.NotDeviceDescribable('state_cond_mean_vars must be the mean-and-variance closure of the same '
                                       'sde_cond_moments_* call as the conditional scaled moments')
    lik = _trace_likelihood(measurement_cond_pdf, tables.d)
    return _lib.shape_outputs(*_run_nd('scaled', tables, lik, ys, moments_partial_order, scms0, mean0, stable, device,
                                       scale0), return_first_nan)
