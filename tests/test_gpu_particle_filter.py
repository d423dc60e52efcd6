"""The bootstrap particle filter on the device (mfs_particle_filter_1d) against the NumPy restatement of the reference on the same
random stream (tests/particle_filter_ref.py), and against the exact Kalman filter.

Tolerances, device against restatement: rtol 1e-9 on nell; |delta| <= 1e-9 (|mean| + sd) on means, samples and variances, with
(mean, sd) the restatement's of that replicate and step; atol 1e-11 on cf entries (the mean of n unit-modulus terms: n u of
summation plus a few ulp of sincos at |z x| <= 10, and <= 7 rotations of ~2 u each where the device rotates).  "Both NaN" counts
as agreement; first_nan must be equal.

Resampling is discrete: the two sides pick the same ancestors only while no target (i + u_i) / n lies within rounding of an
entry of the cumulative weights.  Both sides' prefix sums are within n u of exact, so every parity case asserts, on the
restatement alone, that its resampling margin is >= 16 n 2^-53; the seeds below were chosen so that it is (a seed that fails is
replaced, never skipped).
"""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib
from mfs_amd.classical_filters_smoothers import bootstrap_filter, gaussian_transition, stratified, systematic
from mfs_amd.one_dim import ss_models
from mfs_amd.one_dim.filtering import build_model_struct, _trace_likelihood
from mfs_amd.utils import GaussianSum1D
from tests import brute_force_ref as R
from tests import particle_filter_ref as P

pytestmark = pytest.mark.gpu

RESAMPLERS = {'stratified': stratified, 'systematic': systematic}


def _assert_result_close(res, ref, n, what):
    samples, means, variances, cfs, nell, first_nan, margin = ref
    assert margin >= P.margin_bound(n), f'{what}: resampling margin {margin:.3e} < {P.margin_bound(n):.3e}: choose another seed'
    scale = np.abs(means) + np.sqrt(variances)
    worst = {'nell': P.assert_close(res.nell, nell, np.abs(nell), f'{what} nell'),
             'means': P.assert_close(res.means, means, scale, f'{what} means'),
             'variances': P.assert_close(res.variances, variances, scale, f'{what} variances')}
    if res.samples is not None:
        worst['samples'] = P.assert_close(res.samples, samples, scale[..., None], f'{what} samples')
    if cfs is not None:
        worst['cf'] = P.assert_close(res.cfs, cfs, 1e-11, f'{what} cf', rtol=1.)
    print(f'{what}: margin {margin:.2e}; worst error / bound ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    npt.assert_array_equal(res.first_nan, first_nan)


# ---- the stream
@pytest.mark.parametrize('t', [0, 7])
@pytest.mark.parametrize('tag', [0, 1, 2])
def test_stream_matches_the_restatement(tag, t):
    L = _lib.lib()
    count = 5000
    for seed, draw in ((3, 0), (0xfedcba9876543210, 1)):
        u, z = np.empty(count), np.empty(count)
        _lib.check(L.mfs_pf_draws(seed, t, tag, draw, count, _lib.ptr(u), _lib.ptr(z), 0))
        ru, rz = P.draws(seed, np.arange(count), t, tag, draw)
        assert np.array_equal(u, ru), 'uniforms are not bit-equal'
        ulps = np.abs(z - rz) / np.spacing(np.abs(rz))
        print(f'tag {tag} t {t} seed {seed:#x}: normals differ by at most {ulps.max():.1f} ulp')
        assert ulps.max() <= 4.


# ---- parity sweep: one particle, the wave (63, 64, 65), one block and its edge (1024, 1500), one cf segment and its edge
# (4096, 5000).  Replicate b of a case has its own seed and measurements whatever B is, so its restatement is computed once.
SWEEP_DT, SWEEP_T = P.SWEEP_DT, 12
# n -> first seed where the default (1) leaves a target within 1.3 x the margin bound: seeds 1.. give 1.28 x the bound at
# n = 5000 and 1.01 x at n = 20 000; these give 24 x and 3.2 x
SWEEP_SEED0 = {5000: 21, 20000: 101}


def _sweep_seed(n, b):
    return SWEEP_SEED0.get(n, 1) + b


@functools.lru_cache(maxsize=None)
def _sweep_replicate(n, b, resampling, T=SWEEP_T):
    trans, init = P.sweep_model()
    ys = R.ou_data(T, np.random.default_rng(1000 * n + b), SWEEP_DT)
    ref = P.particle_filter_ref(lambda _: trans, lambda _: P.gauss_pdf, ys[None, :], lambda _: init, [_sweep_seed(n, b)], n,
                                resampling)
    return ys, ref


def _sweep_case(n, B, resampling, T=SWEEP_T):
    reps = [_sweep_replicate(n, b, resampling, T) for b in range(B)]
    ys = np.stack([r[0] for r in reps])
    ref = tuple(np.concatenate([r[1][k] for r in reps]) for k in (0, 1, 2)) + (None,) \
        + tuple(np.concatenate([r[1][k] for r in reps]) for k in (4, 5)) + (min(r[1][6] for r in reps),)
    seeds = np.array([_sweep_seed(n, b) for b in range(B)], dtype=np.uint64)
    return ys, seeds, ref


@pytest.mark.parametrize('resampling', ['stratified', 'systematic'])
@pytest.mark.parametrize('B', [1, 3, 17])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 257, 1024, 1500, 4096, 5000])
def test_shape_sweep_against_restatement(n, B, resampling):
    trans, init = P.sweep_model()
    ys, seeds, ref = _sweep_case(n, B, resampling)
    res = bootstrap_filter(trans, P.gauss_pdf, ys, init, seeds, n, RESAMPLERS[resampling], return_summaries=True)
    assert res.samples.shape == (B, SWEEP_T, n) and res.means.shape == (B, SWEEP_T) and res.cfs is None
    _assert_result_close(res, ref, n, f'n={n} B={B} {resampling}')


@pytest.mark.parametrize('resampling', ['stratified', 'systematic'])
def test_twenty_thousand_particles_cross_workgroups(resampling):
    n, B, T = 20000, 2, 6
    trans, init = P.sweep_model()
    ys, seeds, ref = _sweep_case(n, B, resampling, T)
    res = bootstrap_filter(trans, P.gauss_pdf, ys, init, seeds, n, RESAMPLERS[resampling], return_summaries=True)
    _assert_result_close(res, ref, n, f'n={n} B={B} {resampling}')


# ---- models
def _benes_case(zs, n=1000, T=20, B=3, seed0=1):
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
    trans = gaussian_transition(drift, dispersion, dt, 'tme-3')
    ys = np.random.default_rng(3).random((B, T)) < 0.5
    seeds = np.arange(seed0, seed0 + B, dtype=np.uint64)
    ref = P.particle_filter_ref(lambda b: trans, lambda b: pmf, ys, lambda b: ic, seeds, n, 'stratified', zs=zs)
    return trans, pmf, ys, ic, seeds, ref


@pytest.mark.parametrize('grid', ['uniform', 'uneven'])
def test_benes_bernoulli_tme3_with_characteristic_function(grid):
    n = 1000
    zs = np.linspace(-2., 2., 64)
    if grid == 'uneven':
        zs = np.sort(np.sign(zs) * zs ** 2)
        assert np.ptp(np.diff(zs)) > 0.01
    trans, pmf, ys, ic, seeds, ref = _benes_case(zs)
    res = bootstrap_filter(trans, pmf, ys, ic, seeds, n, zs=zs, return_summaries=True)
    assert res.cfs.shape == (3, 20, 64) and res.cfs.dtype == np.complex128
    _assert_result_close(res, ref, n, f'benes-bernoulli {grid} zs')
    # the reference's call shape: one replicate, positional arguments, (samples, nell)
    samples, nell = bootstrap_filter(trans, pmf, ys[0], ic, int(seeds[0]), n, stratified)
    assert samples.shape == (20, n) and np.array_equal(samples, res.samples[0]) and nell == res.nell[0]


@pytest.mark.parametrize('nz', [300, 600, 2100])
def test_characteristic_function_rotation_paths(nz):
    """nz > 256 puts 2, 4 or 8 frequencies on a thread, which rotates between them on a uniform grid; 2100 needs two frequency
    chunks with a ragged end, and n = 4200 a second, ragged particle segment."""
    n, T, B = 4200, 2, 2
    zs = np.linspace(-2., 2., nz)
    trans, pmf, ys, ic, seeds, ref = _benes_case(zs, n, T, B)
    res = bootstrap_filter(trans, pmf, ys, ic, seeds, n, zs=zs, return_samples=False, return_summaries=True)
    _assert_result_close(res, ref, n, f'cf nz={nz}')
    uneven = zs.copy()
    uneven[nz // 2] += 1e-3                          # not uniform any more: true sincos everywhere
    res2 = bootstrap_filter(trans, pmf, ys, ic, seeds, n, zs=uneven, return_samples=False, return_summaries=True)
    keep = np.arange(nz) != nz // 2
    worst = P.assert_close(res2.cfs[..., keep], ref[3][..., keep], 1e-11, 'cf by sincos', rtol=1.)
    print(f'nz={nz}: sincos path worst error / bound {worst:.2e}')


def test_well_poisson_per_replicate_parameters_explicit_initial_samples():
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.well_poisson(3.)
    n, T, B = 512, 20, 4
    theta1, theta2 = np.array([1., 2., 3., 4.]), np.array([0.5, 1., 1.5, 2.5])
    ys = np.random.default_rng(4).poisson(1., size=(B, T))
    init = ic.sampler(np.random.default_rng(5), B * n).reshape(B, n)
    seeds = np.array([1, 2, 3, 4], dtype=np.uint64)
    ref = P.particle_filter_ref(lambda b: gaussian_transition(lambda x: drift(x, theta1[b]), dispersion, dt, 'euler'),
                                lambda b: (lambda y, x: pmf(y, x, theta2[b])), ys, lambda b: init[b], seeds, n, 'systematic')
    trans = gaussian_transition(lambda x: drift(x, theta1), dispersion, dt, 'euler')
    res = bootstrap_filter(trans, lambda y, x: pmf(y, x, theta2), ys, init, seeds, n, systematic, return_summaries=True)
    _assert_result_close(res, ref, n, 'well-poisson')
    assert np.abs(res.nell[0] - res.nell[3]) > 1e-3       # the parameters reached their replicates
    shared = bootstrap_filter(trans, lambda y, x: pmf(y, x, theta2), ys, init[1], seeds, n, systematic, return_summaries=True)
    assert np.array_equal(shared.samples[1], res.samples[1])      # (n,) initial particles serve every replicate


# ---- invariances
def test_outputs_are_reproducible_and_consistent():
    n, B = 1500, 3
    trans, init = P.sweep_model()
    ys, seeds, _ = _sweep_case(n, B, 'stratified')
    zs = np.linspace(-3., 3., 48)
    args = (trans, P.gauss_pdf, ys, init, seeds, n, stratified)
    full = bootstrap_filter(*args, zs=zs, return_summaries=True)
    again = bootstrap_filter(*args, zs=zs, return_summaries=True)
    for a, b in zip(full, again):
        assert np.array_equal(a, b), 'two identical calls differ'
    for b in range(B):
        one = bootstrap_filter(trans, P.gauss_pdf, ys[b], init, int(seeds[b]), n, stratified, zs=zs,
                               return_summaries=True)
        for a, o in zip(full, one):
            assert np.array_equal(a[b], o), f'replicate {b} differs between the batch and a call of its own'
    lean = bootstrap_filter(*args, zs=zs, return_samples=False, return_summaries=True)
    assert lean.samples is None
    for a, b in zip(full[1:], lean[1:]):
        assert np.array_equal(a, b), 'summaries depend on return_samples'
    by_int = bootstrap_filter(trans, P.gauss_pdf, ys, init, int(seeds[0]), n, stratified)      # seeds k, k + 1, ...
    assert np.array_equal(by_int[0], full.samples) and np.array_equal(by_int[1], full.nell)
    means = full.samples.mean(axis=-1)
    variances = ((full.samples - means[..., None]) ** 2).mean(axis=-1)
    cfs = np.exp(1j * zs[None, None, :, None] * full.samples[:, :, None, :]).mean(axis=-1)
    scale = np.abs(means) + np.sqrt(variances)
    P.assert_close(full.means, means, scale, 'means from samples')
    P.assert_close(full.variances, variances, scale, 'variances from samples')
    P.assert_close(full.cfs, cfs, 1e-11, 'cf from samples', rtol=1.)


def test_nan_poisons_one_replicate_only():
    n, B = 1500, 3
    trans, init = P.sweep_model()
    ys, seeds, _ = _sweep_case(n, B, 'stratified')
    zs = np.linspace(-1., 1., 8)
    clean = bootstrap_filter(trans, P.gauss_pdf, ys, init, seeds, n, zs=zs, return_summaries=True)
    bad = ys.copy()
    bad[1, 4] = 1e6           # every weight underflows to zero
    res = bootstrap_filter(trans, P.gauss_pdf, bad, init, seeds, n, zs=zs, return_summaries=True)
    assert list(res.first_nan) == [-1, 4, -1] and list(clean.first_nan) == [-1, -1, -1]
    for name in ('samples', 'means', 'variances', 'cfs'):
        out, ref = getattr(res, name), getattr(clean, name)
        assert np.isnan(out[1, 4:]).all() and np.array_equal(out[1, :4], ref[1, :4]), name
    assert np.isnan(res.nell[1])
    for a, b in zip(res, clean):
        assert np.array_equal(a[[0, 2]], b[[0, 2]]), 'a neighbour of the poisoned replicate changed'
    assert np.isfinite(res.samples[[0, 2]]).all() and np.isfinite(res.nell[[0, 2]]).all()


# ---- error codes of the C entry
def test_argument_errors_are_codes_with_messages():
    L = _lib.lib()
    trans, _ = P.sweep_model()
    n, T, B = 8, 3, 2
    model, keep = build_model_struct(trans.tables, _trace_likelihood(P.gauss_pdf), B)
    operator = _lib.MfsModel1d.from_buffer_copy(model)
    operator.trans_kind = _lib.TRANS['operator']
    good = dict(model=model, n=n, T=T, B=B, res=0, seeds=np.array([1, 2], dtype=np.uint64), n_mix=1, cumw=np.ones(1),
                mean=np.zeros(1), var=np.ones(1), init=None, ys=np.zeros((B, T)), nz=0, zs=None, cfs=None,
                means=np.empty((B, T)), nell=np.empty(B))

    def call(**kw):
        a = dict(good, **kw)
        variances, fn = np.empty((B, T)), np.empty(B, dtype=np.int32)
        rc = L.mfs_particle_filter_1d(C.byref(a['model']), a['n'], a['T'], a['B'], a['res'], _lib.ptr(a['seeds']), a['n_mix'],
                                      _lib.ptr(a['cumw']), _lib.ptr(a['mean']), _lib.ptr(a['var']), _lib.ptr(a['init']), 0,
                                      _lib.ptr(a['ys']), a['nz'], _lib.ptr(a['zs']), None, _lib.ptr(a['means']),
                                      _lib.ptr(variances), _lib.ptr(a['cfs']), _lib.ptr(a['nell']), _lib.ptr(fn), 0, None)
        return rc, L.mfs_last_error().decode(), a['nell'], fn

    einval = [dict(n=0), dict(T=0), dict(B=0), dict(res=2), dict(res=-1), dict(model=operator), dict(n_mix=-1), dict(n_mix=9),
              dict(n_mix=0), dict(var=np.zeros(1)), dict(var=np.array([np.nan])), dict(nz=4), dict(nz=4, zs=np.zeros(4)),
              dict(nz=4, cfs=np.empty((B, T, 4), dtype=np.complex128)), dict(seeds=None), dict(ys=None), dict(means=None),
              dict(nell=None), dict(cumw=None)]
    for kw in einval:
        rc, msg, _, _ = call(**kw)
        assert rc == -1 and 'mfs_particle_filter_1d' in msg, (kw, rc, msg)
    rc, msg, _, _ = call(n=(1 << 20) + 1)
    assert rc == -2 and str(1 << 20) in msg
    assert L.mfs_pf_draws(1, 0, 0, 0, 4, None, None, 0) == -1
    rc, msg, nell, fn = call()      # and the library still works
    assert rc == 0 and np.isfinite(nell).all() and list(fn) == [-1, -1]
    rc, msg, nell, fn = call(n_mix=0, init=np.linspace(-1., 1., n))
    assert rc == 0 and np.isfinite(nell).all()
    del keep


# ---- analytic pin on the device: independent of the restatement
@pytest.mark.parametrize('n', [10000, 100000])
def test_kalman_pin_on_the_device(n):
    _, _, ys, _ = R.kalman_setting()
    trans = gaussian_transition(R.ou_drift, R.ou_dispersion, R.OU_DT, 'tme-3')
    init = GaussianSum1D.new([0.], [R.OU_SIGMA ** 2], [1.])
    B = 4
    true_m, true_v, true_nell = R.kalman(ys)
    for resampling in (stratified, systematic):
        res = bootstrap_filter(trans, P.gauss_pdf, np.tile(ys, (B, 1)), init, 11, n, resampling, return_samples=False,
                               return_summaries=True)
        print(f'n={n} {resampling.name}: max |mean err| {np.abs(res.means - true_m).max():.3e}, max |nell err| '
              f'{np.abs(res.nell - true_nell).max():.3e}, max |variance err| {np.abs(res.variances - true_v).max():.3e}')
        npt.assert_allclose(res.means, np.tile(true_m, (B, 1)), atol=2e-1)
        assert np.all(np.abs(res.nell - true_nell) <= 0.3)
        assert list(res.first_nan) == [-1] * B
        assert len({float(v) for v in res.nell}) == B          # four seeds, four different runs
