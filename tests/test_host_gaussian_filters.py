"""CPU-only checks of the Gaussian filters: the sigma-point rules of mfs_amd.classical_filters_smoothers.quadratures, the NumPy
restatement of the two filters (tests/gaussian_filters_ref.py) pinned to the exact Kalman filter and to central differences,
the descriptors, and the Python layer's argument handling (nothing here calls the device)."""
import math

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats, sym
from mfs_amd.classical_filters_smoothers import (SigmaPoints, ekf, gaussian_transition, gaussian_transition_nd,
                                                 measurement_moments, sgp_filter)
from mfs_amd.classical_filters_smoothers import gfs
from mfs_amd.classical_filters_smoothers.smc import GaussianTransition
from mfs_amd.multi_dims import ss_models as ss_models_nd
from mfs_amd.one_dim import ss_models
from mfs_amd.one_dim.moments import _trace_sde
from mfs_amd.sym import Poly
from mfs_amd.tme_poly import normal_tables, tme_tables
from tests import brute_force_ref as R
from tests import gaussian_filters_ref as G


# ---- the rules
def _normal_moment(k):
    return 0. if k % 2 else float(math.prod(range(k - 1, 0, -2)))


@pytest.mark.parametrize('order', range(1, 33))
def test_gauss_hermite_1d_integrates_degree_below_twice_the_order(order):
    s = SigmaPoints.gauss_hermite(1, order)
    assert s.d == 1 and s.n_points == order and s.w.shape == (order,) and s.xi.shape == (order, 1) and s.wc is None
    assert abs(s.w.sum() - 1.) <= 1e-14 and np.all(s.w > 0.)
    for k in range(2 * order):
        got, size = s.w @ s.xi[:, 0] ** k, s.w @ np.abs(s.xi[:, 0]) ** k
        assert abs(got - _normal_moment(k)) <= 1e-12 * size, f'order {order}, degree {k}: {got} vs {_normal_moment(k)}'


@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_gauss_hermite_2d_is_the_tensor_product(order):
    s = SigmaPoints.gauss_hermite(2, order)
    one = SigmaPoints.gauss_hermite(1, order)
    assert s.n_points == order ** 2 and s.xi.shape == (order ** 2, 2) and abs(s.w.sum() - 1.) <= 1e-14
    # the reference's point order: the last dimension varies fastest
    npt.assert_array_equal(s.xi[:order, 1], one.xi[:, 0])
    npt.assert_array_equal(s.xi[::order, 0], one.xi[:, 0])
    for a in range(2 * order):
        for b in range(2 * order):
            got = s.w @ (s.xi[:, 0] ** a * s.xi[:, 1] ** b)
            size = s.w @ (np.abs(s.xi[:, 0]) ** a * np.abs(s.xi[:, 1]) ** b)
            assert abs(got - _normal_moment(a) * _normal_moment(b)) <= 1e-12 * size


def test_high_order_rule_stays_accurate():
    # np.roots of the order-256 Hermite polynomial does not: the eigenvalue construction does
    s = SigmaPoints.gauss_hermite(1, 256)
    for k in range(12):
        assert abs(s.w @ s.xi[:, 0] ** k - _normal_moment(k)) <= 1e-12 * (s.w @ np.abs(s.xi[:, 0]) ** k)
    assert 31. < np.abs(s.xi).max() < 31.2


def test_cubature_points_and_unscented():
    for d in (1, 2, 3):
        s = SigmaPoints.cubature(d)
        assert s.n_points == 2 * d and s.xi.shape == (2 * d, d)
        npt.assert_allclose(s.w, 1. / (2 * d))
        npt.assert_allclose(s.xi, math.sqrt(d) * np.concatenate([np.eye(d), -np.eye(d)]))
        npt.assert_allclose(s.expectation(np.einsum('ni,nj->nij', s.xi, s.xi)), np.eye(d), atol=1e-15)
    with pytest.raises(NotImplementedError):
        SigmaPoints.unscented(2, 1., 2., 0.)


def test_sigma_point_methods():
    s = SigmaPoints.gauss_hermite(2, 3)
    m, chol = np.array([1., -2.]), np.array([[2., 0.], [0.5, 0.3]])
    chi = s.gen_sigma_points(m, chol)
    assert chi.shape == (9, 2)
    npt.assert_allclose(s.expectation(chi), m, atol=1e-14)
    npt.assert_allclose(s.expectation(np.einsum('ni,nj->nij', chi - m, chi - m)), chol @ chol.T, atol=1e-14)


# ---- the models
def _ou():
    F, Sigma = math.exp(-R.OU_DT / R.OU_ELL), R.OU_SIGMA ** 2 * (1 - math.exp(-2 * R.OU_DT / R.OU_ELL))
    tables = normal_tables(Poly(np.array([0., F]), 'x'), Poly(np.array([Sigma]), 'x'), 'ou_exact')
    return tables, measurement_moments(lambda y, x: stats.norm_pdf(y, x, math.sqrt(R.OU_R)))


def _benes(method='tme-3'):
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
    return dt, gaussian_transition(drift, dispersion, dt, method), measurement_moments(pmf)


def _well(p1=3., p2=3., method='tme-2'):
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.well_poisson(p1)
    return dt, gaussian_transition(lambda x: drift(x, p1), dispersion, dt, method), \
        measurement_moments(lambda y, x: pmf(y, x, p2))


def _prey(method='euler'):
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models_nd.prey_predator(np.zeros((1, 2), dtype=int))
    return dt, gaussian_transition_nd(drift, dispersion, 2, dt, method), measurement_moments(pmf)


# ---- the restatement
@pytest.mark.parametrize('rule', [2, 3, 11, 'ekf'])
def test_restatement_matches_kalman(rule):
    tables, meas = _ou()
    ys = R.ou_data(100, np.random.default_rng(0))
    true_m, true_v, true_nell = R.kalman(ys)
    sgps = None if rule == 'ekf' else SigmaPoints.gauss_hermite(1, rule)
    ref = G.gaussian_filter_ref(tables, meas, G.EKF if rule == 'ekf' else G.SIGMA_POINT, sgps, [0.], [[R.OU_SIGMA ** 2]], ys)
    G.assert_well_conditioned(ref, f'OU {rule}')
    npt.assert_allclose(ref.means[:, 0], true_m, rtol=0., atol=1e-12)
    npt.assert_allclose(ref.covs[:, 0, 0], true_v, rtol=0., atol=1e-12)
    assert abs(ref.nells[-1] - true_nell) <= 1e-11 * abs(true_nell) and ref.first_nan == -1


def test_restatement_jacobians_against_central_differences():
    # a central difference of step 1e-6 carries rounding of about u |f| / eps = 1e-10 for |f| of order one, and a truncation
    # error of eps^2 f''' / 6 ~ 1e-12: atol 1e-9
    eps = 1e-6
    for trans in (_benes()[1], _well()[1], _well(method='euler')[1]):
        for x in (-1.3, 0.2, 0.9):
            num = (trans.tables.cond_mean(x + eps) - trans.tables.cond_mean(x - eps)) / (2 * eps)
            npt.assert_allclose(G.transition_jacobian(trans.tables, np.array([x]))[0, 0], num, rtol=1e-8, atol=1e-9)
    for method in ('euler', 'tme-2'):
        tables = _prey(method)[1].tables
        x = np.array([1.1, 0.8])
        J = G.transition_jacobian(tables, x)
        for j in range(2):
            e = np.zeros(2)
            e[j] = eps
            num = (G.transition(tables, x + e)[0] - G.transition(tables, x - e)[0]) / (2 * eps)
            npt.assert_allclose(J[:, j], num, rtol=1e-8, atol=1e-9)
    for meas, d in ((_benes()[2], 1), (_well()[2], 1), (_ou()[1], 1), (_prey()[2], 2)):
        lik = meas.spec(d)
        for x in (-1.1, 0.3, 1.4):
            num = (G.measurement(lik, x + eps)[0] - G.measurement(lik, x - eps)[0]) / (2 * eps)
            npt.assert_allclose(G.measurement(lik, x)[2], num, rtol=1e-8, atol=1e-9)


def test_restatement_nan_rule():
    dt, trans, meas = _benes()
    ys = (np.random.default_rng(5).random(6) < 0.5).astype(np.float64)
    ref = G.gaussian_filter_ref(trans.tables, meas, G.SIGMA_POINT, SigmaPoints.gauss_hermite(1, 3), [0.], [[-1.]], ys)
    assert ref.first_nan == 0 and ref.any_nan and np.isnan(ref.means).all() and np.isnan(ref.nells).all()
    ref = G.gaussian_filter_ref(trans.tables, meas, G.SIGMA_POINT, SigmaPoints.gauss_hermite(1, 3), [0.], [[0.]], ys)
    assert ref.first_nan == -1 and not ref.any_nan       # a point mass is legal
    dt, trans, meas = _prey()
    ref = G.gaussian_filter_ref(trans.tables, meas, G.SIGMA_POINT, SigmaPoints.gauss_hermite(2, 3), [1., 1.],
                                [[1e-3, 2e-3], [2e-3, 1e-3]], ys)
    assert ref.first_nan == 0 and np.isnan(ref.covs).all()


def test_logistic_moments_survive_large_arguments():
    lik = _benes()[2].spec(1)
    h, var, dh = G.measurement(lik, np.array([-30., 30.]))      # q(x) = x^3 / 5 = -+5400
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(var)) and np.all(np.isfinite(dh))
    npt.assert_array_equal(h, [0., 1.])


# ---- descriptors
def test_descriptor_kinds():
    dt, trans, meas = _benes()
    assert isinstance(trans, GaussianTransition) and trans.dt == dt and trans.tables.kind == 'gaussian'
    assert GaussianTransition(trans.tables).dt is None       # the particle filter's one-field form stays valid
    assert meas.spec(1).kind == 'bernoulli_logistic'
    assert _well()[2].spec(1).kind == 'poisson_softplus' and _ou()[1].spec(1).kind == 'gaussian'
    dt, trans, meas = _prey('tme-2')
    assert isinstance(trans, gfs.GaussianTransitionND) and trans.dt == dt and trans.tables.d == 2
    lik = meas.spec(2)
    assert lik.kind == 'bernoulli_logistic' and lik.component == 0
    npt.assert_allclose(np.asarray(lik.params), [-1., 0., 0., 1.])
    one = gaussian_transition_nd(lambda x: -x, lambda x: np.array([[1.]]), 1, 0.1, 'euler')
    assert isinstance(one, GaussianTransition) and one.dt == 0.1
    npt.assert_allclose(one.tables.cond_mean(2.), 1.8)
    for bad in ('rk4', 'tme-x', 3):
        with pytest.raises(ValueError, match='method must be'):
            gaussian_transition_nd(lambda x: -x, lambda x: np.eye(2), 2, 0.1, bad)


def test_abi_constants_and_symbols():
    assert _lib.GF_METHOD == {'sigma_point': 0, 'ekf': 1} and _lib.GF_MAX_POINTS == 256
    assert 'mfs_gaussian_filter_1d' in _lib.DECLARED_SYMBOLS and 'mfs_gaussian_filter_nd' in _lib.DECLARED_SYMBOLS


# ---- argument handling: every refusal comes before the library is loaded
@pytest.fixture
def no_library(monkeypatch):
    def refuse(*_a, **_k):
        raise AssertionError('the library was loaded before the arguments were validated')
    monkeypatch.setattr(_lib, 'lib', refuse)
    monkeypatch.setattr(_lib, 'pinned_empty', refuse)


def test_validation_errors(no_library):
    dt, trans, meas = _benes()
    dt2, trans2, meas2 = _prey()
    gh, gh2 = SigmaPoints.gauss_hermite(1, 3), SigmaPoints.gauss_hermite(2, 3)
    ys = np.zeros(5)
    with pytest.raises(ValueError, match='differs from the step'):
        sgp_filter(trans, meas, gh, [0.], [[1.]], 2 * dt, ys)
    with pytest.raises(ValueError, match='differs from the step'):
        ekf(trans2, meas2, [1., 1.], np.eye(2), 2 * dt2, ys)
    with pytest.raises(ValueError, match='gaussian_transition'):
        sgp_filter(lambda x, dt: (x, 1.), meas, gh, [0.], [[1.]], dt, ys)
    with pytest.raises(ValueError, match='measurement_moments'):
        ekf(trans, lambda x: (x, 1.), [0.], [[1.]], dt, ys)
    with pytest.raises(ValueError, match='callable'):
        measurement_moments(3.)
    a, b = _trace_sde(lambda x: sym.tanh(x), lambda _: 1.)
    with pytest.raises(ValueError, match='Normal closure'):
        ekf(GaussianTransition(tme_tables(a, b, dt, 2, gaussian=False)), meas, [0.], [[1.]], dt, ys)
    with pytest.raises(ValueError, match='SigmaPoints'):
        sgp_filter(trans, meas, (gh.xi, gh.w), [0.], [[1.]], dt, ys)
    with pytest.raises(ValueError, match='2-dimensional'):
        sgp_filter(trans, meas, gh2, [0.], [[1.]], dt, ys)
    with pytest.raises(ValueError, match='1-dimensional'):
        sgp_filter(trans2, meas2, gh, [1., 1.], np.eye(2), dt2, ys)
    with pytest.raises(ValueError, match='1 .. 256 points'):
        sgp_filter(trans, meas, SigmaPoints.gauss_hermite(1, 257), [0.], [[1.]], dt, ys)
    with pytest.raises(ValueError, match='1 .. 256 points'):
        sgp_filter(trans2, meas2, SigmaPoints.gauss_hermite(2, 17), [1., 1.], np.eye(2), dt2, ys)
    with pytest.raises(NotImplementedError, match='one likelihood factor'):
        ekf(trans2, measurement_moments(lambda y, x: math.prod(stats.norm_pdf(y, x, 1.5))), [1., 1.], np.eye(2), dt2,
            np.zeros((5, 2)))
    with pytest.raises(NotImplementedError, match='one state component'):
        ekf(trans2, measurement_moments(lambda y, x: stats.norm_pdf(y, sym.arctan2(x[1], x[0]), 0.1)), [1., 1.], np.eye(2),
            dt2, ys)
    dt3 = 0.01
    with pytest.raises(NotImplementedError, match='d = 3'):
        ekf(gaussian_transition_nd(lambda x: -x, lambda x: np.eye(3), 3, dt3, 'euler'), meas2, np.ones(3), np.eye(3), dt3, ys)
    for bad_m0, bad_v0 in (([0., 0.], [[1.]]), ([0.], np.eye(2)), (np.zeros(4), [[1.]])):
        with pytest.raises(ValueError, match='must have shape'):
            sgp_filter(trans, meas, gh, bad_m0, bad_v0, dt, ys)
    with pytest.raises(ValueError, match='leading replicate axis'):
        sgp_filter(trans, meas, gh, [[0.]], [[1.]], dt, np.zeros(3))     # (B, 1) initial means, ys (T,)
    with pytest.raises(ValueError, match='ys must have shape'):
        ekf(trans, meas, [0.], [[1.]], dt, np.zeros((2, 3, 4, 1)))
    with pytest.raises(ValueError, match='ys must have shape'):
        ekf(trans, meas, [0.], [[1.]], dt, np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match='at least one'):
        ekf(trans, meas, [0.], [[1.]], dt, np.zeros((0,)))


def test_per_replicate_parameters_need_a_batch_axis(no_library):
    p1, p2 = np.array([0.5, 3., 6.]), np.array([1., 3., 6.])
    dt, trans, meas = _well(p1, p2)
    gh = SigmaPoints.gauss_hermite(1, 3)
    with pytest.raises(ValueError, match='leading replicate axis'):
        sgp_filter(trans, meas, gh, [0.], [[1.]], dt, np.zeros(5))
    with pytest.raises(ValueError, match='leading replicate axis'):
        ekf(trans, _well()[2], [0.], [[1.]], dt, np.zeros(5))
    with pytest.raises(ValueError, match='batch'):
        ekf(trans, meas, [0.], [[1.]], dt, np.zeros((4, 5)))      # three parameter points, four replicates


def test_ys_shape_rules():
    for shape, want, squeeze in (((7,), (1, 7), True), ((7, 1), (1, 7), True), ((3, 7), (3, 7), False),
                                 ((3, 7, 1), (3, 7), False), ((1, 7), (1, 7), False)):
        ys = np.arange(np.prod(shape), dtype=np.int64).reshape(shape)
        out, sq = gfs._split_ys(ys)
        assert out.shape == want and sq is squeeze and out.dtype == np.float64 and out.flags['C_CONTIGUOUS']
        npt.assert_array_equal(out.reshape(-1), np.arange(np.prod(shape)))


def test_initial_shape_rules():
    m, v, batched = gfs._initial(0.5, 2., 1, 4, False)
    assert m.shape == (1,) and v.shape == (1, 1) and not batched
    m, v, batched = gfs._initial(np.arange(4.), 2., 1, 4, False)
    assert m.shape == (4, 1) and v.shape == (4, 1, 1) and batched and np.all(v == 2.)
    m, v, batched = gfs._initial([1., 2.], np.arange(12.).reshape(3, 2, 2), 2, 3, False)
    assert m.shape == (3, 2) and v.shape == (3, 2, 2) and batched and np.all(m == [1., 2.])
    m, v, batched = gfs._initial([[1.], [2.]], [[[3.]], [[4.]]], 1, 2, False)
    assert batched and m[1, 0] == 2. and v[1, 0, 0] == 4.
