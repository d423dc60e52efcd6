"""Support for the tests that reach the kernels through the plan API of the C ABI (include/mfs_hip.h, mfs_plan_*): one runner
for 1-D plans, one for N-D plans, one bit-for-bit comparison, one context manager for the build switches that a plan reads
when it is created (csrc/capi_1d.hip), and the models and inputs that several of those test files share.  A plain module:
no fixtures, nothing happens on import, and the library is loaded only by the two runners."""
import collections
import contextlib
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt

from mfs_amd import _lib, stats, synth
from mfs_amd._lib import BUILD, TRAITS
from mfs_amd.one_dim import filtering, moments, ss_models
from mfs_amd.utils import GaussianSum1D
from tests import one_dim_support


# ---- results ------------------------------------------------------------------------------------------------------------
class Outputs(collections.namedtuple('Outputs', 'moments means scales nell first_nan')):
    """What one run of a plan wrote, downloaded; None stands for an output the run was not given a buffer for."""
    __slots__ = ()

    def rows(self, idx):
        """The same record restricted to (or reordered by) replicates `idx`."""
        return Outputs(*(None if x is None else x[idx] for x in self))


# what a 1-D plan says about itself: mfs_plan_1d_kernel_build / _traits / _partner and mfs_plan_1d_geometry
Report1d = collections.namedtuple('Report1d', 'build traits partner lanes_per_filter filters_per_block grid lds_bytes')
# mfs_plan_nd_geometry / mfs_plan_nd3_geometry
ReportNd = collections.namedtuple('ReportNd', 'threads_per_filter grid lds_bytes')

CENTRAL_OUTPUTS = ('moments', 'means', 'nell', 'first_nan')


def assert_same_bits(a, b, what='', names=None):
    """Two result records, or two sequences of arrays, hold the same bits: as many outputs on either side, None only against
    None, equal shapes and dtypes, float arrays with NaNs in the same places (a poisoned replicate is NaN-filled from its first
    bad step on) and the same bit patterns everywhere else, integer arrays equal.  `what` and `names` label a failure."""
    names = names or getattr(a, '_fields', None)
    a, b = list(a), list(b)
    assert len(a) == len(b), f'{what}: {len(a)} outputs against {len(b)}'
    for i, (x, y) in enumerate(zip(a, b)):
        label = f'{what}: {names[i] if names else f"output {i}"}'
        if x is None or y is None:
            assert x is None and y is None, f'{label} is present on one side only'
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, f'{label}: {x.dtype}{x.shape} against {y.dtype}{y.shape}'
        if x.dtype.kind == 'f':
            nx, ny = np.isnan(x), np.isnan(y)
            npt.assert_array_equal(nx, ny, err_msg=f'{label}: NaN positions')
            bits = np.dtype(f'u{x.dtype.itemsize}')
            npt.assert_array_equal(x[~nx].view(bits), y[~ny].view(bits), err_msg=label)
        else:
            npt.assert_array_equal(x, y, err_msg=label)


# ---- the build switches -------------------------------------------------------------------------------------------------
SWITCHES = ('MFS_FAST_BUILD', 'MFS_FAST_TRAITS', 'MFS_FAST_PARTNER', 'MFS_PREDICT_RULE', 'MFS_SOLVER', 'MFS_LANES_PER_FILTER')


@contextlib.contextmanager
def build_switches(monkeypatch, **given):
    """Inside the block every variable of SWITCHES is unset except those given (`MFS_FAST_BUILD='generic'`, ...); on the way
    out, by return or by exception, the environment is what it was.  The switches are read when a plan is created, so a
    plan created inside the block picks what the block says and nothing that an earlier test or the caller's shell left."""
    assert set(given) <= set(SWITCHES), given
    with monkeypatch.context() as patch:
        for name in SWITCHES:
            patch.delenv(name, raising=False)
        for name, value in given.items():
            patch.setenv(name, value)
        yield


def three_builds(monkeypatch, run, **env):
    """[run() on the default plan, on the specialised build with run-time traits, on the generic build], each under `env`
    (MFS_PREDICT_RULE, say) and nothing else."""
    results = []
    for switch in ({}, {'MFS_FAST_TRAITS': 'runtime'}, {'MFS_FAST_BUILD': 'generic'}):
        with build_switches(monkeypatch, **env, **switch):
            results.append(run())
    return results


# ---- the runners --------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _handle(create, destroy):
    """A library object that is destroyed however the block ends; its destructor's return code is checked if the block
    ended well (a failure inside the block is the one to report)."""
    h = C.c_void_p()
    _lib.check(create(C.byref(h)))
    try:
        yield h
    finally:
        rc = destroy(h)
    _lib.check(rc)


def _ints(call, plan, n):
    v = [C.c_int(-1) for _ in range(n)]
    _lib.check(call(plan, *[C.byref(x) for x in v]))
    return [x.value for x in v]


def _upload_start(B, d, m0, mean0, scale0):
    """(d_m0, m0_batched, d_mean0, d_scale0 | None) for states of dimension d.  The one rule for m0_batched: m0 with a
    leading replicate axis, (B, z), is a start per replicate; (z,) is one start shared by the batch.  mean0 and scale0 follow
    m0: a value given for a single replicate is repeated B times next to a batched m0."""
    batched = np.ndim(m0) == 2
    shape = ((B,) if batched else (1,) if d == 1 else ()) + ((d,) if d > 1 else ())

    def follow(v):
        return None if v is None else _lib.DeviceBuffer.from_array(np.broadcast_to(np.asarray(v, dtype=np.float64), shape))
    return _lib.DeviceBuffer.from_array(np.asarray(m0, dtype=np.float64)), int(batched), follow(mean0), follow(scale0)


def _run_once(L, run, plan, start, d_ys, shapes, outputs, zero_fill, stream):
    """One mfs_plan_*_run into fresh buffers for `outputs` (NULL for the rest), synchronised and downloaded."""
    assert set(outputs) <= set(Outputs._fields), outputs
    d_m0, batched, d_mean0, d_scale0 = start
    bufs = {}
    for name in outputs:
        bufs[name] = _lib.DeviceBuffer(int(np.prod(shapes[name])) * (4 if name == 'first_nan' else 8))
        if zero_fill and name in ('means', 'scales'):
            _lib.check(L.mfs_memset(bufs[name].ptr, 0, bufs[name].nbytes, None))
    if zero_fill:
        _lib.check(L.mfs_device_synchronize())
    p = lambda buf: buf.ptr if buf is not None else None      # noqa: E731
    _lib.check(run(plan, d_m0.ptr, batched, p(d_mean0), p(d_scale0), d_ys.ptr,
                   *[p(bufs.get(name)) for name in Outputs._fields], stream))
    _lib.check(L.mfs_stream_synchronize(stream) if stream is not None else L.mfs_device_synchronize())
    return Outputs(*(bufs[name].to_array(shapes[name], np.int32 if name == 'first_nan' else np.float64) if name in bufs
                     else None for name in Outputs._fields))


def run_plan_1d(model, N, T, B, *, mode='central', stable=0, chunk=0, m0=None, mean0=None, scale0=None, ys=None,
                outputs=CENTRAL_OUTPUTS, zero_fill=False, runs=1):
    """Create a 1-D plan, read back what it picked, run it `runs` times on device-resident buffers and destroy it:
    (Report1d, [Outputs of each run]).  runs=0 only creates and describes the plan, and then needs no start state or ys.

    model     (tables, lik) as filtering.trace_model returns them, or (mfs_model_1d, keep-alive) built beforehand
    m0        (2N,): one start shared by the batch (m0_batched = 0); (B, 2N): a start per replicate (m0_batched = 1).  This
              shape is the only thing the flag is derived from.  mean0 and scale0 follow it; scalars are repeated.
    outputs   the buffers passed to the run, of Outputs._fields; the others are NULL and come back as None
    zero_fill means and scales are zeroed before each run (a mode that does not write one of them must leave it alone)
    Every run writes into fresh buffers on a stream of its own plan, and downloads them.  The plan and the stream are
    destroyed even if a check in between fails."""
    L = _lib.lib()
    desc, keep = model if isinstance(model[0], _lib.MfsModel1d) else filtering.build_model_struct(*model, B)
    with _handle(lambda p: L.mfs_plan_1d_create(p, C.byref(desc), _lib.MODE[mode], N, T, B, stable, chunk, 0),
                 L.mfs_plan_1d_destroy) as plan:
        report = Report1d(*_ints(L.mfs_plan_1d_kernel_build, plan, 1), *_ints(L.mfs_plan_1d_kernel_traits, plan, 1),
                          *_ints(L.mfs_plan_1d_kernel_partner, plan, 1), *_ints(L.mfs_plan_1d_geometry, plan, 4))
        results = []
        if runs:
            start = _upload_start(B, 1, m0, mean0, scale0)
            d_ys = _lib.DeviceBuffer.from_array(ys)
            shapes = {'moments': (B, T, 2 * N), 'means': (B, T), 'scales': (B, T), 'nell': (B,), 'first_nan': (B,)}
            with _handle(L.mfs_stream_create, L.mfs_stream_destroy) as stream:
                for _ in range(runs):
                    results.append(_run_once(L, L.mfs_plan_1d_run, plan, start, d_ys, shapes, outputs, zero_fill, stream))
    del keep
    return report, results


def run_plan_nd(model, N, T, B, mi, inds, *, joint=None, mode='central', stable=0, m0, mean0, scale0=None, ys,
                outputs=(CENTRAL_OUTPUTS,)):
    """The N-D counterpart, for mfs_plan_nd_* (model: mfs_model_nd, d = 2), mfs_plan_nd3_* (mfs_model_nd3) and
    mfs_plan_nd3_create_joint (mfs_model_nd3 and `joint`: mfs_joint_nd3): (ReportNd, [Outputs of each run]).  `outputs` has
    one tuple of output names per run of the plan, so a second run may ask for less (NLL only).  The descriptors' keep-alives
    stay with the caller.  m0 of shape (z,) is shared, (B, z) per replicate, as for run_plan_1d; the runs go to the NULL
    stream and are followed by a device synchronisation, as a caller without a stream of its own would do it."""
    L = _lib.lib()
    d, z = mi.shape[1], mi.shape[0]
    mi32, inds32 = np.ascontiguousarray(mi, dtype=np.int32), np.ascontiguousarray(inds, dtype=np.int32)
    tail = (_lib.MODE[mode], N, T, B, z, _lib.ptr(mi32), _lib.ptr(inds32), stable, 0)
    if isinstance(model, _lib.MfsModelNd):
        assert joint is None and d == 2
        create = lambda p: L.mfs_plan_nd_create(p, C.byref(model), *tail)      # noqa: E731
        run, destroy, geometry = L.mfs_plan_nd_run, L.mfs_plan_nd_destroy, L.mfs_plan_nd_geometry
    else:
        assert isinstance(model, _lib.MfsModelNd3) and d == 3
        if joint is None:
            create = lambda p: L.mfs_plan_nd3_create(p, C.byref(model), *tail)      # noqa: E731
        else:
            create = lambda p: L.mfs_plan_nd3_create_joint(p, C.byref(model), C.byref(joint), *tail)      # noqa: E731
        run, destroy, geometry = L.mfs_plan_nd3_run, L.mfs_plan_nd3_destroy, L.mfs_plan_nd3_geometry
    with _handle(create, destroy) as plan:
        report = ReportNd(*_ints(geometry, plan, 3))
        start = _upload_start(B, d, m0, mean0, scale0)
        d_ys = _lib.DeviceBuffer.from_array(ys)
        shapes = {'moments': (B, T, z), 'means': (B, T, d), 'scales': (B, T, d), 'nell': (B,), 'first_nan': (B,)}
        results = [_run_once(L, run, plan, start, d_ys, shapes, names, False, None) for names in outputs]
    return report, results


# ---- shared models and inputs of the 1-D one-wave tests --------------------------------------------------------------------
# the (model, transition) pairs that have a fixed-traits build, and the traits code each must report
COMBOS = {'benes_tme3': TRAITS['central_tanh_bernoulli'], 'benes_tme_normal3': TRAITS['central_tanh_bernoulli'],
          'ou_normal': TRAITS['central_identity_gaussian']}


@functools.lru_cache(maxsize=None)
def combo_model(combo, N, mode='central'):
    """(ic, tables, lik, dt) of one model in one moment mode; traced once per session."""
    if combo.startswith('benes'):
        m = one_dim_support.benes(N, 'tme' if combo == 'benes_tme3' else 'tme_normal', 3)
        dt, ic, fns, pmf = m.dt, m.ic, m.fns, m.pmf
    else:   # the OU / Gaussian workload of the benchmark's config 3
        dt, ell, sigma = 0.1, 1., 0.5
        F, Sigma = np.exp(-dt / ell), sigma ** 2 * (1 - np.exp(-2 * dt / ell))
        ic = GaussianSum1D.new(means=[0.], variances=[sigma ** 2], weights=[1.], N=N)
        pmf = lambda y, x: stats.norm_pdf(y, x, 1.)   # noqa: E731
        fns = moments.sde_cond_moments_normal(lambda x: F * x, lambda x: Sigma)
    mean_fn = fns[3] if mode == 'central' else fns[4] if mode == 'scaled' else None
    tables, lik = filtering.trace_model(mode, fns[_lib.MODE[mode]], mean_fn, pmf)
    return ic, tables, lik, dt


@functools.lru_cache(maxsize=None)
def traced(combo, N):
    """(ic, tables, lik, dt) in central mode; traced once per session.  COMBOS and 'benes_tme2': Benes-Bernoulli with TME-2
    tables (4 operator terms), a specialised shape with run-time traits."""
    if combo != 'benes_tme2':
        return combo_model(combo, N)
    dt, ic, tables, lik = benes(N, 'tme', 2)
    return ic, tables, lik, dt


def benes(N, family, order):
    """(dt, ic, tables, lik) of Benes-Bernoulli in central mode with TME ('tme') or TME-normal ('tme_normal') tables."""
    m = one_dim_support.benes(N, family, order)
    tables, lik = filtering.trace_model('central', m.fns[1], m.fns[3], m.pmf)
    return m.dt, m.ic, tables, lik


def start(combo, N, nb):
    return np.tile(traced(combo, N)[0].cms, (nb, 1))


@functools.lru_cache(maxsize=None)
def bernoulli_ys(N, T, seed, B):
    return synth.benes_bernoulli_batch(B, T, ss_models.benes_bernoulli(N)[0], seed=seed)[0]


def unlike_replicates(combo, N, T):
    """One wave of four unlike replicates: (ys (4, T), m0 (4, 2N)).  0: ordinary measurements; 1: a surprise mid-run, which
    moves the posterior away from the prediction the eigenvalue iteration starts from, so this group needs more evaluations
    than its neighbours; 2: near-constant measurements; 3: a point-mass start, poisoned at step 0 (the second pivot of the first
    rule is 0, not > 0) -- as test_gpu_fast_traits.test_poisoned_group_next_to_live_groups builds it."""
    rng = np.random.default_rng(3200 + N)
    ys = np.empty((4, T))
    if combo == 'ou_normal':
        dt, ell, sigma = 0.1, 1., 0.5
        F, q = np.exp(-dt / ell), sigma * np.sqrt(1 - np.exp(-2 * dt / ell))
        x = np.empty(T)
        x[0] = sigma * rng.standard_normal()
        for t in range(1, T):
            x[t] = F * x[t - 1] + q * rng.standard_normal()
        ys[0] = x + rng.standard_normal(T)
        ys[1] = ys[0][::-1]
        ys[1, T // 2] = 9.                              # nine standard deviations of the measurement noise
        ys[2] = 0.25 + 1e-9 * rng.standard_normal(T)
        ys[3] = ys[0]
    else:
        full = synth.benes_bernoulli_batch(4, T, ss_models.benes_bernoulli(N)[0], seed=3300 + N)[0]
        ys[0] = full[0]
        ys[1, :T // 2], ys[1, T // 2:] = 1., 0.         # a long run of ones, then only zeros
        ys[2] = 0.
        ys[3] = full[3]
    m0 = start(combo, N, 4)
    m0[3, 1:] = 0.
    return ys, m0


# Poisoning mid-run: (N, T, seed) chosen with the CPU oracle (oracle/c) on Benes-Bernoulli, TME-3, B = 6: first poisoned steps
#   N = 14: [166, 157, 206, -, 213, -]    N = 15: [-, -, 118, 219, -, 91]    N = 16: [149, -, 123, -, 72, 121]
# so every wave (four replicates at N = 14, 15; two at N = 16) holds replicates that are poisoned mid-run, in whichever half
# of a step their pivot fails, next to replicates that live to T.
MID_RUN = {14: (300, 2943), 15: (300, 2952), 16: (200, 2966)}
MID_RUN_B = 6


def run_central(combo, N, ys, m0, *, chunk=0, moments_out=True):
    """One central-mode plan run of traced(combo, N) on (B, T) measurements and (B, 2N) start moments: (Report1d, Outputs)."""
    ic, tables, lik, _ = traced(combo, N)
    nb, nt = ys.shape
    report, (out,) = run_plan_1d((tables, lik), N, nt, nb, chunk=chunk, m0=m0, mean0=ic.mean, ys=ys,
                                 outputs=CENTRAL_OUTPUTS[0 if moments_out else 1:])
    return report, out


# ---- the partner-wave variant and the one-wave build it stands in for (test_gpu_fast_partner, test_gpu_partner_boundary) ----
FILTERS_PER_WORKGROUP = 16


def partner_variant(monkeypatch, combo, N, ys, m0, *, env=None, **kw):
    """The default plan: it must be the partner-wave variant, reported as the fixed-traits one-wave build."""
    with build_switches(monkeypatch, **(env or {})):
        report, out = run_central(combo, N, ys, m0, **kw)
    assert report[:3] == (BUILD['fast_one_wave_spec'], COMBOS[combo], 1)
    assert (report.filters_per_block, report.grid) == (FILTERS_PER_WORKGROUP, -(-ys.shape[0] // FILTERS_PER_WORKGROUP))
    return out


def one_wave_build(monkeypatch, combo, N, ys, m0, *, env=None, **kw):
    """The same plan with MFS_FAST_PARTNER=0: the fixed-traits one-wave build, four filters per single-wave block."""
    with build_switches(monkeypatch, MFS_FAST_PARTNER='0', **(env or {})):
        report, out = run_central(combo, N, ys, m0, **kw)
    assert report[:3] == (BUILD['fast_one_wave_spec'], COMBOS[combo], 0) and report.filters_per_block == 4
    return out


def partner_inputs(combo, N, nb, nt, poison=True):
    """Bernoulli measurements (a Gaussian law accepts 0 / 1 as well) and the model's start moments; replicate 1 starts from a
    point mass, so it is poisoned at step 0 -- in the cold rule of the main wave -- next to live replicates."""
    ys = synth.benes_bernoulli_batch(nb, nt, ss_models.benes_bernoulli(N)[0], seed=4100 + 16 * N + nb)[0]
    m0 = np.tile(combo_model(combo, N)[0].cms, (nb, 1))
    if poison and nb > 1:
        m0[1, 1:] = 0.
    return ys, m0
