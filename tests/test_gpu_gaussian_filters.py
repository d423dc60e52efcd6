"""The Gaussian filters on the device (mfs_gaussian_filter_1d / _nd) against the NumPy restatement of the same equations
(tests/gaussian_filters_ref.py), and against the exact Kalman filter.

Tolerance, device against restatement: that of the particle-filter suite on the same tables and likelihood functions --
|delta| <= 1e-9 (|mean| + sd) on means and covariance entries, with (mean, sd) the restatement's of that replicate and step, and
rtol 1e-9 on the running nells.  "Both NaN" counts as agreement; first_nan must be equal.  Every parity case first asserts, on
the restatement alone, that it is well conditioned: no NaN, eigenvalue ratio Pp / Pf <= 16 (the cancellation in
P = Pp - K K^T S) and S >= 1e-3; a seed that fails is replaced, never skipped.

Replicate b of a case has its own measurements and initial law whatever B is, so its restatement is computed once and shared.
"""
import ctypes as C
import functools
import math

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats
from mfs_amd.classical_filters_smoothers import (SigmaPoints, ekf, gaussian_transition, gaussian_transition_nd,
                                                 measurement_moments, sgp_filter)
from mfs_amd.multi_dims import ss_models as ss_models_nd
from mfs_amd.one_dim import ss_models
from mfs_amd.one_dim.filtering import build_model_struct
from mfs_amd.one_dim.moments import _trace_sde
from mfs_amd.sym import Poly
from mfs_amd.classical_filters_smoothers.smc import GaussianTransition
from mfs_amd.tme_poly import normal_tables, tme_tables
from tests import brute_force_ref as R
from tests import gaussian_filters_ref as G

pytestmark = pytest.mark.gpu


# ---- models: name -> (d, dt, transition descriptor, measurement descriptor)
@functools.lru_cache(maxsize=None)
def _model(name):
    if name == 'ou':
        F, Sigma = math.exp(-R.OU_DT / R.OU_ELL), R.OU_SIGMA ** 2 * (1 - math.exp(-2 * R.OU_DT / R.OU_ELL))
        trans = GaussianTransition(normal_tables(Poly(np.array([0., F]), 'x'), Poly(np.array([Sigma]), 'x'), 'ou_exact'))
        return 1, R.OU_DT, trans, measurement_moments(lambda y, x: stats.norm_pdf(y, x, math.sqrt(R.OU_R)))
    if name == 'benes':
        dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
        return 1, dt, gaussian_transition(drift, dispersion, dt, 'tme-3'), measurement_moments(pmf)
    if name.startswith('well'):
        _, method, p1, p2 = name.split(':')
        p1, p2 = float(p1), float(p2)
        dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.well_poisson(p1)
        return 1, dt, gaussian_transition(lambda x: drift(x, p1), dispersion, dt, method), \
            measurement_moments(lambda y, x: pmf(y, x, p2))
    if name.startswith('prey'):
        _, method = name.split(':')
        dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models_nd.prey_predator(np.zeros((1, 2), dtype=int))
        return 2, dt, gaussian_transition_nd(drift, dispersion, 2, dt, method), measurement_moments(pmf)
    raise ValueError(name)


def _seed(name, b):
    return [sum(name.encode()), b]


def _data(name, b, T):
    """Measurements and initial law of replicate b: its own whatever the batch."""
    rng = np.random.default_rng(_seed(name, b))
    if name == 'ou':
        return R.ou_data(T, rng), np.array([0.05 * (b % 3 - 1)]), np.array([[R.OU_SIGMA ** 2 * (1. + 0.25 * (b % 2))]])
    if name == 'benes':
        return (rng.random(T) < 0.5).astype(np.float64), np.array([0.1 * (b % 3)]), np.array([[0.3 * (1. + 0.1 * (b % 4))]])
    if name.startswith('well'):
        return rng.poisson(1., T).astype(np.float64), np.array([0.1 * (b % 3 - 1)]), np.array([[0.3 * (1. + 0.1 * (b % 4))]])
    c = 2e-4 * (b % 3)
    return (rng.random(T) < 0.5).astype(np.float64), np.array([1. + 0.01 * (b % 2), 1.]), np.array([[1.5e-3, c], [c, 2e-3]])


def _rule(d, rule):
    return None if rule == 'ekf' else SigmaPoints.cubature(d) if rule == 'cub' else SigmaPoints.gauss_hermite(d, rule)


@functools.lru_cache(maxsize=None)
def _replicate(name, rule, b, T):
    d, dt, trans, meas = _model(name)
    ys, m0, v0 = _data(name, b, T)
    ref = G.gaussian_filter_ref(trans.tables, meas, G.EKF if rule == 'ekf' else G.SIGMA_POINT, _rule(d, rule), m0, v0, ys)
    return ys, m0, v0, ref


def _device(name, rule, ys, m0, v0, **kw):
    d, dt, trans, meas = _model(name)
    if rule == 'ekf':
        return ekf(trans, meas, m0, v0, dt, ys, return_first_nan=True, **kw)
    return sgp_filter(trans, meas, _rule(d, rule), m0, v0, dt, ys, return_first_nan=True, **kw)


def _batch(name, rule, B, T):
    reps = [_replicate(name, rule, b, T) for b in range(B)]
    return (np.stack([r[0] for r in reps]), np.stack([r[1] for r in reps]), np.stack([r[2] for r in reps]),
            [r[3] for r in reps])


def _check_parity(name, rule, B, T):
    d = _model(name)[0]
    ys, m0, v0, refs = _batch(name, rule, B, T)
    what = f'{name} {rule} B={B}'
    for b, ref in enumerate(refs):
        G.assert_well_conditioned(ref, f'{what} replicate {b}')
    means, covs, nells, first_nan = _device(name, rule, ys, m0, v0)
    assert means.shape == (B, T, d) and covs.shape == (B, T, d, d) and nells.shape == (B, T) and first_nan.shape == (B,)
    G.assert_filter_close(means, covs, nells, np.stack([r.means for r in refs]), np.stack([r.covs for r in refs]),
                          np.stack([r.nells for r in refs]), what)
    npt.assert_array_equal(first_nan, [r.first_nan for r in refs])
    npt.assert_array_equal(covs, np.swapaxes(covs, -1, -2))


# ---- 1. exactness on the linear-Gaussian model
@pytest.mark.parametrize('rule', [2, 3, 11, 32, 'ekf'])
def test_ou_gaussian_equals_the_kalman_filter(rule):
    T, B = 50, 3
    ys = np.stack([_data('ou', b, T)[0] for b in range(B)])
    m0, v0 = 0., R.OU_SIGMA ** 2
    means, covs, nells, first_nan = _device('ou', rule, ys, [m0], [[v0]])
    true = [R.kalman(ys[b], mean0=m0, var0=v0) for b in range(B)]
    tm, tv = np.stack([t[0] for t in true]), np.stack([t[1] for t in true])
    worst_m = G.assert_close(means[..., 0], tm, np.abs(tm) + np.sqrt(tv), f'OU {rule} means')
    worst_v = G.assert_close(covs[..., 0, 0], tv, np.abs(tm) + np.sqrt(tv), f'OU {rule} variances')
    tn = np.array([t[2] for t in true])
    worst_n = G.assert_close(nells[:, -1], tn, np.abs(tn), f'OU {rule} nell')
    print(f'OU {rule}: worst error / bound against the Kalman filter: means {worst_m:.2e}, variances {worst_v:.2e}, nell {worst_n:.2e}')
    assert np.all(first_nan == -1)
    _check_parity('ou', rule, B, T)      # and the per-replicate initial laws against the restatement


# ---- 2. shape sweep, 1-D: group widths 1 .. 64, the strided path (> 64 points) and the edges; partial groups, several blocks
@pytest.mark.parametrize('B', [1, 3, 5, 67])
@pytest.mark.parametrize('n_points', [1, 2, 3, 11, 16, 17, 32, 33, 63, 64, 65, 128, 256])
def test_shape_sweep_benes_bernoulli(n_points, B):
    _check_parity('benes', n_points, B, 40)


@pytest.mark.parametrize('B', [1, 3, 5, 67])
@pytest.mark.parametrize('n_points', [1, 2, 3, 11, 16, 17, 32, 33])
@pytest.mark.parametrize('method', ['tme-2', 'euler'])
def test_shape_sweep_well_poisson(method, n_points, B):
    _check_parity(f'well:{method}:3:3', n_points, B, 40)


def test_cubature_1d():
    _check_parity('benes', 'cub', 5, 40)


# ---- 3. EKF, 1-D
@pytest.mark.parametrize('B', [1, 67])
@pytest.mark.parametrize('method', ['tme-2', 'euler'])
def test_ekf_well_poisson(method, B):
    _check_parity(f'well:{method}:3:3', 'ekf', B, 100)


def test_ekf_benes_bernoulli_does_not_update_where_the_jacobian_vanishes():
    # replicate 0 starts at m = 0, where q'(x) = 3 x^2 / 5 = 0: H = 0, the gain is zero and the mean stays at 0
    _check_parity('benes', 'ekf', 5, 100)
    ys, m0, v0, ref = _replicate('benes', 'ekf', 0, 100)
    means, covs, nells, _ = _device('benes', 'ekf', ys, m0, v0)
    assert np.all(means == 0.) and np.all(np.diff(covs[:, 0, 0]) > 0.) and np.all(np.isfinite(nells))


# ---- 4. d = 2
@pytest.mark.parametrize('B', [1, 3, 9])
@pytest.mark.parametrize('rule', [1, 2, 3, 8, 11, 16, 'ekf'])
@pytest.mark.parametrize('method', ['euler', 'tme-2'])
def test_prey_predator(method, rule, B):
    _check_parity(f'prey:{method}', rule, B, 60)


def test_cubature_2d():
    _check_parity('prey:euler', 'cub', 3, 60)


# ---- 5. per-replicate parameters
@pytest.mark.parametrize('rule', [11, 'ekf'])
@pytest.mark.parametrize('method', ['tme-2', 'euler'])
def test_per_replicate_parameters(method, rule):
    p1, p2 = np.array([0.5, 3., 6., 2.]), np.array([1., 3., 6., 4.])
    B, T = 4, 40
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.well_poisson(3.)
    trans = gaussian_transition(lambda x: drift(x, p1), dispersion, dt, method)
    meas = measurement_moments(lambda y, x: pmf(y, x, p2))
    names = [f'well:{method}:{p1[b]}:{p2[b]}' for b in range(B)]
    reps = [_replicate(names[b], rule, b, T) for b in range(B)]
    for b, r in enumerate(reps):
        G.assert_well_conditioned(r[3], f'{names[b]} {rule}')
    ys, m0, v0 = (np.stack([r[k] for r in reps]) for k in range(3))
    if rule == 'ekf':
        means, covs, nells, first_nan = ekf(trans, meas, m0, v0, dt, ys, return_first_nan=True)
    else:
        means, covs, nells, first_nan = sgp_filter(trans, meas, _rule(1, rule), m0, v0, dt, ys, return_first_nan=True)
    G.assert_filter_close(means, covs, nells, np.stack([r[3].means for r in reps]), np.stack([r[3].covs for r in reps]),
                          np.stack([r[3].nells for r in reps]), f'well-Poisson {method} {rule} parameter batch')
    assert np.all(first_nan == -1)
    assert len({float(v) for v in nells[:, -1]}) == B      # four parameter points, four likelihoods


# ---- 6. reproducibility
@pytest.mark.parametrize('name, rule', [('benes', 11), ('benes', 65), ('benes', 'ekf'), ('well:tme-2:3:3', 3),
                                        ('prey:euler', 3), ('prey:tme-2', 11), ('prey:euler', 'ekf')])
def test_replicate_is_bit_equal_alone_and_in_a_batch(name, rule):
    B, T = 67, 20
    ys, m0, v0, _ = _batch(name, rule, B, T)
    first = _device(name, rule, ys, m0, v0)
    again = _device(name, rule, ys, m0, v0)
    for a, c in zip(first, again):
        assert np.array_equal(a, c, equal_nan=True), 'two runs differ'
    for b in (0, 5, 66):
        alone = _device(name, rule, ys[b], m0[b], v0[b])
        for a, c in zip(alone, first):
            assert np.array_equal(a, c[b]), f'replicate {b} alone differs from the batch'
        small = _device(name, rule, ys[b:b + 1], m0[b:b + 1], v0[b:b + 1])
        assert np.array_equal(small[0][0], first[0][b])


# ---- 7. the NaN rule
@pytest.mark.parametrize('name, rule', [('benes', 11), ('benes', 128), ('prey:euler', 3)])
def test_nan_rule_poisons_one_replicate_only(name, rule):
    B, T = 5, 20
    d = _model(name)[0]
    ys, m0, v0, _ = _batch(name, rule, B, T)
    clean = _device(name, rule, ys, m0, v0)
    bad = v0.copy()
    bad[2] = [[-1.]] if d == 1 else [[1e-3, 2e-3], [2e-3, 1e-3]]      # negative variance; indefinite covariance
    means, covs, nells, first_nan = _device(name, rule, ys, m0, bad)
    assert np.isnan(means[2]).all() and np.isnan(covs[2]).all() and np.isnan(nells[2]).all()
    npt.assert_array_equal(first_nan, [-1, -1, 0, -1, -1])
    for b in (0, 1, 3, 4):
        for got, want in zip((means, covs, nells), clean):
            assert np.array_equal(got[b], want[b]), f'replicate {b} changed'
    # and it is the restatement's rule
    ref = G.gaussian_filter_ref(_model(name)[2].tables, _model(name)[3], G.SIGMA_POINT, _rule(d, rule), m0[2], bad[2], ys[2])
    assert ref.first_nan == 0


def test_zero_initial_variance_is_legal():
    ys, m0, _, _ = _replicate('benes', 3, 1, 20)
    v0 = np.zeros((1, 1))
    ref = G.gaussian_filter_ref(_model('benes')[2].tables, _model('benes')[3], G.SIGMA_POINT, _rule(1, 3), m0, v0, ys)
    G.assert_well_conditioned(ref, 'benes from a point mass')
    means, covs, nells, first_nan = _device('benes', 3, ys, m0, v0)
    G.assert_filter_close(means, covs, nells, ref.means, ref.covs, ref.nells, 'benes from a point mass')
    assert first_nan == -1


# ---- 8. error codes of the C entry point
def test_error_codes():
    L = _lib.lib()
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
    lik = measurement_moments(pmf).spec(1)
    s = SigmaPoints.gauss_hermite(1, 3)
    xi, w = np.ascontiguousarray(s.xi), np.ascontiguousarray(s.w)
    T, B = 4, 1
    ys, m0, v0 = np.zeros((B, T)), np.zeros(1), np.ones(1)
    out = [np.empty((B, T)) for _ in range(3)]
    fn = np.empty(B, dtype=np.int32)

    def call(model, method, n_points):
        return L.mfs_gaussian_filter_1d(C.byref(model), method, n_points, _lib.ptr(xi), _lib.ptr(w), T, B, _lib.ptr(m0),
                                        _lib.ptr(v0), 0, _lib.ptr(ys), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                        _lib.ptr(fn), 0, None)

    a, b = _trace_sde(drift, dispersion)
    operator, keep_op = build_model_struct(tme_tables(a, b, dt, 3, gaussian=False), lik, B)
    gaussian, keep = build_model_struct(tme_tables(a, b, dt, 3, gaussian=True), lik, B)
    assert call(operator, 0, 3) == -1 and b'MFS_TRANS_GAUSSIAN' in L.mfs_last_error()       # MFS_EINVAL
    assert call(gaussian, 0, 0) == -2 and call(gaussian, 0, 257) == -2                      # MFS_EUNSUPPORTED
    assert call(gaussian, 2, 3) == -1                                                       # unknown method
    assert call(gaussian, 0, 3) == 0 and np.all(np.isfinite(out[2])) and fn[0] == -1
    del keep_op, keep
