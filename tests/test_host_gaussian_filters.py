"""CPU-only checks of the Gaussian filters: the sigma-point rules of mfs_amd.classical_filters_smoothers.quadratures, the NumPy
restatement of the two filters (tests/gaussian_filters_ref.py) pinned to the exact Kalman filter and to central differences,
the descriptors, and the Python layer's argument handling (nothing here calls the device)."""
import math
import os

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
from tests import gaussian_filters_exact as X
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


# =====================================================================================================================
# the 50-digit arbiter (tests/gaussian_filters_exact.py) and its fixture (tests/golden/gaussian_filters_exact.npz)
# =====================================================================================================================
AGREE = 1e-40


@pytest.fixture(scope='module')
def frozen():
    with np.load(os.path.join(os.path.dirname(__file__), 'golden', X.FIXTURE)) as npz:
        return {k: npz[k] for k in npz.files}


def _linear_case(component):
    rng = np.random.default_rng([7, component])
    model = X.Model(2, X.linear_table2(), 'gaussian', X.LINEAR_LIK, 'x', 0., component)
    return model, np.array([0.3, -0.2]), np.array([[0.4, -0.05], [0.1, 0.3]]), 0.6 * rng.standard_normal(12)


# ---- B.1 the arbiter against the matrix Kalman filter, d = 2, full F and Q, either component measured
@pytest.mark.parametrize('component', [0, 1])
def test_arbiter_equals_the_matrix_kalman_filter(component):
    model, m0, P0, ys = _linear_case(component)
    H = np.zeros(2)
    H[component] = X.LINEAR_LIK[0]
    sym_P0 = np.array([[P0[0, 0], P0[1, 0]], [P0[1, 0], P0[1, 1]]])
    true = X.kalman_mp(X.LINEAR_F, X.LINEAR_C, X.LINEAR_Q, H, X.LINEAR_LIK[1], X.LINEAR_LIK[2], m0, sym_P0, ys)
    assert X.LINEAR_F[0, 1] != 0. and X.LINEAR_F[1, 0] != 0. and X.LINEAR_F[0, 1] != X.LINEAR_F[1, 0] and X.LINEAR_Q[0, 1] != 0.
    for order in (2, 3):
        xi, w = X.gauss_hermite_mp(2, order)
        assert X.trace_distance(X.sigma_point_mp(model, xi, w, m0, P0, ys), true) <= AGREE, f'GH-{order}'
    assert X.trace_distance(X.ekf_mp(model, m0, P0, ys), true) <= AGREE
    # and it is not blind: the other component, or the upper triangle of P0, is another filter
    other = X.ekf_mp(model._replace(component=1 - component), m0, P0, ys)
    assert X.trace_distance(other, true) > 1e-3
    assert X.trace_distance(X.ekf_mp(model, m0, P0.T, ys), true) > 1e-3


# ---- B.2 the closed form against the restated sigma-point filter at a sufficient order, and not below it
def _adf_models():
    one = X.case('adf1/gh4')
    two = X.case('adf2/gh4')
    c2 = two.model.coef      # S_01 not constant; mu cubic in either variable and in both together
    assert np.count_nonzero(c2[3]) > 1 and np.all(c2[:2, 3, 0] != 0.) and np.all(c2[:2, 0, 3] != 0.) and np.all(c2[:2, 1, 2] != 0.)
    assert one.model.coef[0, 3] != 0. and one.model.coef[1, 2] != 0.
    return one, two


@pytest.mark.parametrize('which', [0, 1])
def test_closed_form_adf_equals_a_sufficient_rule_and_no_lesser_one(which):
    case = _adf_models()[which]
    d = case.model.d
    m0, P0 = case.initial(0)
    ys = case.ys[0][:8]
    closed = X.adf_closed_form(case.model, m0, P0, ys)
    # degree max(2 deg mu, deg S) = 6 in a standard variable: order n integrates 2 n - 1
    for order in (4, 6):
        xi, w = X.gauss_hermite_mp(d, order)
        assert X.trace_distance(X.sigma_point_mp(case.model, xi, w, m0, P0, ys), closed) <= AGREE, f'order {order}'
    xi, w = X.gauss_hermite_mp(d, 3)
    gap = X.trace_distance(X.sigma_point_mp(case.model, xi, w, m0, P0, ys), closed)
    assert gap > 1e-7, f'order 3 integrates degree 5 only, yet differs from the closed form by {float(gap):.3g}'


# ---- B.3 the restatement against the arbiter on every frozen case
def _spread(name, got, exact):
    return G.assert_filter_close(got['means'], got['covs'], got['nells'], exact['means'], exact['covs'], exact['nells'], name)


def test_restatement_against_the_arbiter(frozen):
    stored_spread = {'means': 0., 'covs': 0., 'nells': 0.}
    for case in X.cases():
        case, exact, ref = X.thaw(frozen, case)
        runs = [X.restatement_of(case, r) for r in range(case.R)]
        if case.guarded:
            for r, run in enumerate(runs):
                G.assert_well_conditioned(run, f'{case.name} replicate {r}')
        now = {q: np.stack([getattr(run, q) for run in runs]) for q in ('means', 'covs', 'nells')}
        npt.assert_array_equal([run.first_nan for run in runs], exact['first_nan'], err_msg=case.name)
        _spread(f'{case.name} (restatement now)', now, exact)
        npt.assert_array_equal(ref['first_nan'], exact['first_nan'], err_msg=case.name)
        worst = _spread(f'{case.name} (restatement stored)', ref, exact)
        for q, v in worst.items():
            stored_spread[q] = max(stored_spread[q], v)
    print('REF_SPREAD measured: ' + ', '.join(f'{q} {v:.3e}' for q, v in stored_spread.items()))
    # the recorded value is the measured one: not smaller, and not padded
    for q, v in stored_spread.items():
        assert v <= X.REF_SPREAD[q] <= 1.05 * v, f'REF_SPREAD[{q!r}] = {X.REF_SPREAD[q]:.4e}, measured {v:.4e}'


def test_the_fixture_covers_the_case_list(frozen):
    names = {k.split(':')[0] for k in frozen}
    assert names == {c.name for c in X.cases()}
    for c in X.cases():
        assert c.ys.shape[1] <= 24 and c.R <= 5
        if c.guarded and (c.arbiter or c.method) == X.SIGMA_POINT:
            assert c.n_points <= 64, f'{c.name}: mpmath runs at most 64 points outside the saturation cases'


# ---- B.4 the fixture is what the generator writes
@pytest.mark.parametrize('name', X.FRESHNESS_CASES)
def test_fixture_is_fresh(frozen, name):
    fresh = X.freeze(X.case(name))
    for key, value in fresh.items():
        got = frozen[key]
        assert got.dtype == np.asarray(value).dtype and got.shape == np.shape(value), key
        assert np.array_equal(got, value, equal_nan=True), f'{key} differs from a fresh run of the generator'


# ---- the rule on measurements that are not finite, in the arbiter and in the restatement
@pytest.mark.parametrize('bad', [math.nan, math.inf, -math.inf])
@pytest.mark.parametrize('name', ['lanes1/n3', 'edges1/deg0/ekf', 'lanes2/n4', 'matrix2/gaussian/c1/ekf/D7'])
def test_non_finite_measurement_poisons_from_that_step(name, bad):
    case = X.case(name)
    ys = case.ys[:, :6].copy()
    ys[1, 3] = bad
    case = case._replace(ys=ys)
    for run in (X.arbiter_of, X.restatement_of):
        clean, hit = run(case, 0), run(case, 1)
        assert clean.first_nan == -1 and np.all(np.isfinite(clean.nells))
        assert hit.first_nan == 3
        assert np.all(np.isfinite(hit.means[:3])) and np.all(np.isfinite(hit.covs[:3])) and np.all(np.isfinite(hit.nells[:3]))
        assert np.isnan(hit.means[3:]).all() and np.isnan(hit.covs[3:]).all() and np.isnan(hit.nells[3:]).all()


def test_point_masses_at_d2_in_the_arbiter(frozen):
    # diag(v, 0): a zero second pivot, legal.  diag(0, v) and 0: the first pivot divides by zero, poisoned at step 0
    _, exact, ref = X.thaw(frozen, X.case('pointmass2/sigma_point'))
    npt.assert_array_equal(exact['first_nan'], [-1, 0, 0])
    npt.assert_array_equal(ref['first_nan'], [-1, 0, 0])
    _, exact, _ = X.thaw(frozen, X.case('pointmass2/ekf'))          # the EKF takes no Cholesky factor
    npt.assert_array_equal(exact['first_nan'], [-1, -1, -1])


def test_saturation_cases_reach_the_tails(frozen):
    case, exact, _ = X.thaw(frozen, X.case('saturation/bernoulli_logistic/sigma_point'))
    sd = np.sqrt(exact['covs'][..., 0, 0]).min()
    assert np.abs(case.xi).max() > 31. and case.model.lik[3] * (sd * 31.) ** 3 > 1000.
    assert np.all(np.isfinite(exact['nells'])) and np.all(exact['first_nan'] == -1)
    case, exact, _ = X.thaw(frozen, X.case('saturation/poisson_softplus/sigma_point'))
    assert case.model.lik[0] * np.sqrt(exact['covs'][..., 0, 0]).min() * 31. > 100. and np.all(np.isfinite(exact['nells']))


# ---- the frozen cases can see the defects they are there for (the restatement carries the defect; the arbiter is the stored one)
def _restatement_misses(frozen, name, defect):
    case, exact, _ = X.thaw(frozen, X.case(name))
    case = defect(case)
    runs = [X.restatement_of(case, r) for r in range(case.R)]
    now = {q: np.stack([getattr(run, q) for run in runs]) for q in ('means', 'covs', 'nells')}
    with pytest.raises(AssertionError):
        _spread(f'{name} with the defect', now, exact)


def test_a_dropped_tail_point_shows_only_where_it_has_weight(frozen):
    def drop(case):
        w = case.w.copy()
        w[64] = 0.      # lane 0 of a 64-lane group takes points 0 and 64
        return case._replace(w=w)
    _restatement_misses(frozen, 'adf1/gh65-centre-last', drop)
    _restatement_misses(frozen, 'adf2/gh9-centre-last', drop)
    case, exact, _ = X.thaw(frozen, X.case('adf1/gh65'))      # the outermost node of 65 weighs 1e-28: no fp64 test sees it go
    assert case.w[64] < 1e-25
    runs = [X.restatement_of(drop(case), r) for r in range(case.R)]
    _spread('adf1/gh65 without its last point', {q: np.stack([getattr(run, q) for run in runs]) for q in ('means', 'covs', 'nells')}, exact)


@pytest.mark.parametrize('method', [X.SIGMA_POINT, X.EKF])
def test_the_upper_triangle_of_p0_shows_if_read(frozen, method):
    _restatement_misses(frozen, f'matrix2/asymmetric/{method}', lambda case: case._replace(P0=np.swapaxes(case.P0, -1, -2).copy()))
