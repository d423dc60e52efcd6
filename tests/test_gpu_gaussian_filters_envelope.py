"""The Gaussian filters on the device over their whole envelope, against arbiters that owe nothing to fp64 summation order
(tests/gaussian_filters_exact.py, frozen in tests/golden/gaussian_filters_exact.npz): the step of include/mfs_hip.h in 50-digit
arithmetic, a closed-form assumed-density filter that uses no quadrature rule, and the matrix Kalman filter.

Two bars, device against arbiter, per case and quantity:
  hard    |delta| <= 1e-9 (|mean| + sd) on means and covariance entries ((mean, sd) the arbiter's), rtol 1e-9 on the running
          nells, equal first_nan, "both NaN" agreeing -- the numbers of tests/test_gpu_gaussian_filters.py;
  sharp   the same error <= 8 x REF_SPREAD, REF_SPREAD the largest error of the fp64 NumPy restatement against the arbiter over
          all cases, measured on the CPU (tests/test_host_gaussian_filters.py), about 2e-15 (|mean| + sd).  The 8 covers what
          the restatement does not share with the device: a butterfly sum over up to 64 lanes, ocml's exp / tanh / log1p / log
          at a few ulp where libm is <= 1, and multiply-adds contracted to FMAs -- each O(u) per term, like the restatement's
          own error.
The conditioning guard (no NaN, eigenvalue ratio Pp / Pf <= 16, S >= 1e-3) is asserted on the restatement alone, for every case,
by the host test; the saturation and point-mass cases are exempt from the guard, not from the bars.

The fixture holds R = 3 (or 5, or 2) replicates per case; a batch of B takes replicate b % R, with its own table row where the
tables are per replicate.  Every call goes through the C entry with guard words around every output buffer.

Which case launches which build (gf_filter_1d / gf_filter_2d <L, EKF>), each held to the arbiter:
    d = 1  L = 1 lanes1/n1, edges1/batched/n1/*   L = 2 lanes1/n2      L = 4 lanes1/n3, adf1/gh4     L = 8 lanes1/n5, n7, adf1/gh5, gh8
           L = 16 lanes1/n11, adf1/gh12          L = 32 lanes1/n17, n25   L = 64 lanes1/n33, n64, adf1/gh33, gh65, saturation/*
           EKF edges1/*/ekf, saturation/*/ekf
    d = 2  L = 1 lanes2/n1      L = 2 lanes2/n2 (two points)      L = 4 lanes2/n4, kalman cubature / GH-2
           L = 8 lanes2/n5, n7 (a partial last round)            L = 16 lanes2/n9, n16, matrix2/*, adf2/gh4
           L = 32 lanes2/n17, n25, adf2/gh5                      L = 64 lanes2/n64, adf2/gh8, adf2/gh9-centre-last (81 points)
           EKF matrix2/*/ekf, pointmass2/ekf
What each would catch: `on0 ? q01 : q11` swapped in the EKF -- matrix2/*/c1/ekf and the Kalman test on component 1 (C1 and S read
q01 for q11); P0[2] read as P0[1] -- matrix2/asymmetric/* (the upper entry is 99); one lane's tail point dropped at n = 65 --
adf1/gh65-centre-last (the tail point is the centre node, weight 0.15; in adf1/gh65 it is the outermost node, weight 1e-28, which
no fp64 test can see); the finite(y) term removed -- test_first_nan_contract.
"""
import ctypes as C
import functools
import os
import types

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib
from mfs_amd.classical_filters_smoothers import SigmaPoints, sgp_filter
from mfs_amd.classical_filters_smoothers.gfs import GaussianTransitionND, MeasurementMoments
from mfs_amd.classical_filters_smoothers.smc import GaussianTransition
from mfs_amd.multi_dims import filtering as _fnd
from mfs_amd.one_dim.filtering import fill_model_struct
from tests import gaussian_filters_exact as X
from tests import gaussian_filters_ref as G

pytestmark = pytest.mark.gpu

GUARD = 16                 # guard words on either side of every output buffer
SENTINEL = -12345.678      # no filter output


@pytest.fixture(scope='module')
def frozen():
    with np.load(os.path.join(os.path.dirname(__file__), 'golden', X.FIXTURE)) as npz:
        return {k: npz[k] for k in npz.files}


# ---- the call
def _tile(a, nd, B):
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a if a.ndim == nd else a[np.arange(B) % a.shape[0]])


def _struct(model, B):
    """mfs_model_1d / mfs_model_nd straight from the arrays -> (struct, keep-alive)."""
    if model.d == 1:
        coef, lik = _tile(model.coef, 2, B), _tile(model.lik, 1, B)
        tables = types.SimpleNamespace(kind='gaussian', umap=model.umap, n_terms=0, mean_x_coef=float(model.cx))
        return fill_model_struct(tables, types.SimpleNamespace(kind=model.kind), coef.shape[-1] - 1, coef, lik, coef.ndim == 3,
                                 lik.ndim == 2)
    lik = np.asarray(model.lik, dtype=np.float64)
    padded = np.zeros(lik.shape[:-1] + (_lib.MAX_LIK,))
    padded[..., :lik.shape[-1]] = lik
    padded = _tile(padded, 1, B)
    m = _lib.MfsModelNd()
    m.d, m.trans_kind, m.n_terms, m.extent, m.n_factors, m.ny = 2, _lib.ND_TRANS_GAUSSIAN, 5, model.coef.shape[-1], 1, 1
    m.fac_kind[0], m.fac_component[0], m.fac_ycol[0], m.fac_n_par[0] = _lib.LIK[model.kind], int(model.component), 0, lik.shape[-1]
    m.coef_batched, m.lik_batched = 0, int(padded.ndim == 2)
    return _fnd._attach(m, coef=np.asarray(model.coef, dtype=np.float64), lik=padded)


class _Guarded:
    """An output buffer between guard words; `ptr` is NULL when the caller does not pass it."""

    def __init__(self, shape, dtype, passed):
        self.n = int(np.prod(shape))
        self.fill = np.array(SENTINEL).astype(dtype)
        self.buf = np.full(self.n + 2 * GUARD, self.fill, dtype=dtype)
        self.payload = self.buf[GUARD:GUARD + self.n]
        self.shape, self.passed = shape, passed

    @property
    def ptr(self):
        return _lib.ptr(self.payload) if self.passed else None

    def result(self, what):
        assert np.all(self.buf[:GUARD] == self.fill) and np.all(self.buf[GUARD + self.n:] == self.fill), f'{what}: guard words written'
        if not self.passed:
            assert np.all(self.payload == self.fill), f'{what}: written although NULL was passed'
            return None
        return self.payload.reshape(self.shape).copy()


def _device(case, B, means=True, covs=True, first_nan=True, ys=None):
    """(means, covs, nells, first_nan) of the C entry on replicates b % R of the case; None for an output not passed."""
    model, d, T = case.model, case.model.d, case.ys.shape[1]
    idx = np.arange(B) % case.R
    ys = np.ascontiguousarray(case.ys[idx] if ys is None else ys)
    batched = case.m0.ndim == 2
    m0 = np.ascontiguousarray(case.m0[idx] if batched else case.m0)
    P0 = np.ascontiguousarray(case.P0[idx] if batched else case.P0)
    sp = case.method == X.SIGMA_POINT
    xi, w = (np.ascontiguousarray(case.xi), np.ascontiguousarray(case.w)) if sp else (None, None)
    struct, keep = _struct(model, B)
    out = (_Guarded((B, T, d), np.float64, means), _Guarded((B, T, d, d), np.float64, covs), _Guarded((B, T), np.float64, True),
           _Guarded((B,), np.int32, first_nan))
    L = _lib.lib()
    entry = L.mfs_gaussian_filter_1d if d == 1 else L.mfs_gaussian_filter_nd
    rc = entry(C.byref(struct), _lib.GF_METHOD['sigma_point' if sp else 'ekf'], case.n_points, _lib.ptr(xi), _lib.ptr(w), T, B,
               _lib.ptr(m0), _lib.ptr(P0), int(batched), _lib.ptr(ys), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr, 0, None)
    assert rc == 0, L.mfs_last_error()
    del keep
    return tuple(o.result(f'{case.name} B={B} output {k}') for k, o in enumerate(out))


def _hold(what, got, exact, idx):
    """Both bars on (means, covs, nells, first_nan) against the arbiter's replicates idx."""
    means, covs, nells, first_nan = got
    worst = G.assert_filter_close(means, covs, nells, exact['means'][idx], exact['covs'][idx], exact['nells'][idx], what)
    npt.assert_array_equal(first_nan, exact['first_nan'][idx], err_msg=what)
    npt.assert_array_equal(covs, np.swapaxes(covs, -1, -2))
    sharp = {q: v / (X.SHARP_FACTOR * X.REF_SPREAD[q]) for q, v in worst.items()}
    print(f'{what}: worst error / sharp bound ' + ', '.join(f'{q} {v:.2e}' for q, v in sharp.items()))
    for q, v in sharp.items():
        assert v <= 1., (f'{what}: {q} are {worst[q]:.3g} x 1e-9 from the arbiter, more than {X.SHARP_FACTOR:g} x the restatement\'s '
                         f'own {X.REF_SPREAD[q]:.3g}')
    return worst


def _check(frozen, name, B):
    case, exact, _ = X.thaw(frozen, X.case(name))
    idx = np.arange(B) % case.R
    return case, _hold(f'{name} B={B}', _device(case, B), exact, idx)


def _lanes(n):
    L = 1
    while L < n and L < 64:
        L *= 2
    return L


def _names(prefix):
    return [c.name for c in X.cases() if c.name.startswith(prefix)]


# ---- C.1 truth at d = 2: the matrix Kalman filter
@functools.lru_cache(maxsize=None)
def _kalman_truth(component):
    case = X.case_2d(f'kalman2/c{component}', 2, 'gaussian', component, X.EKF, table=X.linear_table2(), asymmetric=True)
    H = np.zeros(2)
    H[component] = X.LINEAR_LIK[0]
    runs = []
    for r in range(case.R):
        P0 = case.P0[r].copy()
        P0[0, 1] = P0[1, 0]
        runs.append(X.kalman_mp(X.LINEAR_F, X.LINEAR_C, X.LINEAR_Q, H, X.LINEAR_LIK[1], X.LINEAR_LIK[2], case.m0[r], P0, case.ys[r]))
    exact = {q: np.stack([getattr(run, q) for run in runs]) for q in ('means', 'covs', 'nells')}
    exact['first_nan'] = np.full(case.R, -1, dtype=np.int32)
    return case, exact


@pytest.mark.parametrize('component', [0, 1])
@pytest.mark.parametrize('rule', [2, 3, 5, 8, 'cub', 'ekf'])
def test_linear_model_equals_the_matrix_kalman_filter(rule, component):
    case, exact = _kalman_truth(component)
    assert np.array_equal(case.model.lik, X.LINEAR_LIK)
    if rule != 'ekf':
        xi, w = X._cub(2) if rule == 'cub' else X._gh(2, rule)
        case = case._replace(method=X.SIGMA_POINT, xi=xi, w=w)
    _hold(f'linear d = 2, component {component}, rule {rule}', _device(case, 3), exact, np.arange(3))


# ---- C.2 the closed-form ADF, through the Python layer: tables built directly, every sufficient rule
class _Spec(MeasurementMoments):
    """A measurement descriptor whose factor is given, not traced."""

    def spec(self, d):
        return self.pdf


@pytest.mark.parametrize('name', _names('adf1/') + _names('adf2/'))
def test_closed_form_adf(frozen, name):
    case, exact, _ = X.thaw(frozen, X.case(name))
    tables, factor = X.host_tables(case.model)
    trans = GaussianTransition(tables) if case.model.d == 1 else GaussianTransitionND(tables, None)
    rule = SigmaPoints(case.model.d, case.n_points, case.w, None, case.xi)
    got = sgp_filter(trans, _Spec(factor), rule, case.m0, case.P0, 1., case.ys, return_first_nan=True)
    _hold(f'{name} (sgp_filter)', got, exact, np.arange(case.R))
    _hold(f'{name} (C entry)', _device(case, case.R), exact, np.arange(case.R))


def test_closed_form_adf_rules_share_one_truth(frozen):
    for prefix in ('adf1/', 'adf2/'):
        exacts = [X.thaw(frozen, X.case(n))[1] for n in _names(prefix)]
        assert len(exacts) >= 4
        for e in exacts[1:]:
            for q in ('means', 'covs', 'nells'):
                npt.assert_array_equal(e[q], exacts[0][q])


# ---- C.3 every lane group at both dimensions: one full block, and one replicate in a second block whose other groups are dead
@pytest.mark.parametrize('second_block', [False, True])
@pytest.mark.parametrize('name', _names('lanes1/') + _names('lanes2/'))
def test_every_lane_group(frozen, name, second_block):
    L = _lanes(X.case(name).n_points)
    _check(frozen, name, 64 // L + 1 if second_block else 1)


def test_lane_groups_are_all_there():
    for prefix in ('lanes1/', 'lanes2/'):
        assert {_lanes(X.case(n).n_points) for n in _names(prefix)} == {1, 2, 4, 8, 16, 32, 64}
    assert [X.case(n).n_points for n in ('lanes2/n2', 'lanes2/n5', 'lanes2/n7', 'lanes2/n17', 'lanes2/n25')] == [2, 5, 7, 17, 25]


# ---- C.4 the d = 2 model matrix
@pytest.mark.parametrize('name', _names('matrix2/'))
def test_model_matrix_2d(frozen, name):
    case = X.case(name)
    if 'likbatched' in name:
        assert case.R == 5 and case.model.lik.shape == (5, 4) and len({tuple(row) for row in case.model.lik}) == 5
    if 'sharedinit' in name:
        assert case.m0.shape == (2,) and case.P0.shape == (2, 2) and case.R == 3
    if 'asymmetric' in name:
        assert np.all(case.P0[:, 0, 1] == 99.) and np.all(np.abs(case.P0[:, 1, 0]) < 1.)
    _check(frozen, name, 67 if name == 'matrix2/likbatched/ekf' else case.R)


def test_model_matrix_2d_is_complete():
    seen = {(c.model.kind, c.model.component, c.method) for c in X.cases() if c.name.startswith('matrix2/')}
    assert seen >= {(k, c, m) for k in X.KINDS for c in (0, 1) for m in (X.SIGMA_POINT, X.EKF)}
    for method in (X.SIGMA_POINT, X.EKF):
        extents = {c.model.coef.shape[-1] for c in X.cases() if c.name.startswith('matrix2/') and c.method == method}
        assert extents >= {1, 2, 3, 5, 7}
    for c in X.cases():      # a truncated Horner loop shows: no zero in the top row and column of any block
        if c.name.startswith('matrix2/') and c.model.coef.shape[-1] > 1:
            assert np.all(c.model.coef[:, -1, :] != 0.) and np.all(c.model.coef[:, :, -1] != 0.)


# ---- C.5 the d = 1 table edges
@pytest.mark.parametrize('name', _names('edges1/'))
def test_table_edges_1d(frozen, name):
    case = X.case(name)
    if '/deg15/' in name:
        assert case.model.coef.shape == (2, 16) and np.all(case.model.coef[:, -1] != 0.)
    if '/deg0/' in name:
        assert case.model.coef.shape == (2, 1)
    if '/nlik' in name:
        assert case.model.lik.shape == (3, int(name.split('/nlik')[1][0]))
    _check(frozen, name, 67 if '/batched/' in name else case.R)


# ---- C.6 optional outputs
@pytest.mark.parametrize('name', ['lanes1/n5', 'edges1/nlik4/ekf', 'lanes2/n9', 'matrix2/gaussian/c1/ekf/D7'])
def test_optional_outputs(frozen, name):
    case = X.thaw(frozen, X.case(name))[0]
    full = _device(case, 3)
    for means, covs, first_nan in ((False, True, True), (True, False, True), (False, False, True), (True, True, False),
                                   (False, False, False)):
        got = _device(case, 3, means=means, covs=covs, first_nan=first_nan)      # asserts the guard words and the NULL buffers
        for k, (g, f) in enumerate(zip(got, full)):
            assert g is None or np.array_equal(g, f), f'{name}: output {k} changed with means={means} covs={covs} first_nan={first_nan}'
        assert got[2] is not None and (got[0] is None) == (not means) and (got[1] is None) == (not covs)


# ---- C.7 saturation, C.8 point masses: outside the conditioning guard, inside both bars
@pytest.mark.parametrize('name', _names('saturation/'))
def test_saturation(frozen, name):
    case, exact, _ = X.thaw(frozen, X.case(name))
    got = _device(case, case.R)
    assert all(np.all(np.isfinite(a)) for a in got[:3]) and np.all(got[3] == -1)
    _hold(name, got, exact, np.arange(case.R))


def test_saturated_logistic_moments_are_zero_not_nan(frozen):
    # an EKF whose mean sits at |q| = |x|^3 / 5 = 5400: p (1 - p) = 0 and p (1 - p) q' = 0 exactly, so H = 0 and S = 0 -- which is
    # the NaN rule's business (S must be > 0), at step 0, and not a NaN born in the measurement moments; the arbiter agrees
    case = X.thaw(frozen, X.case('saturation/bernoulli_logistic/ekf'))[0]
    case = case._replace(m0=np.array([[30.], [-30.]]), ys=case.ys[:, :3])
    got = _device(case, 2)
    exact = [X.arbiter_of(case, r) for r in range(2)]
    npt.assert_array_equal(got[3], [0, 0])
    npt.assert_array_equal([e.first_nan for e in exact], [0, 0])
    assert all(np.isnan(a).all() for a in got[:3])


@pytest.mark.parametrize('name', _names('pointmass2/'))
def test_point_masses_2d(frozen, name):
    case, exact, _ = X.thaw(frozen, X.case(name))
    assert np.array_equal(np.diagonal(case.P0, axis1=-2, axis2=-1) > 0., [[True, False], [False, True], [False, False]])
    got = _device(case, 3)
    _hold(name, got, exact, np.arange(3))
    # diag(v, 0), a zero second pivot, is legal; a zero first pivot divides by zero and poisons step 0 of the sigma-point filter
    npt.assert_array_equal(got[3], [-1, 0, 0] if case.method == X.SIGMA_POINT else [-1, -1, -1])


# ---- C.9 the first_nan contract: a measurement that is not finite
@pytest.mark.parametrize('bad', [np.nan, np.inf])
@pytest.mark.parametrize('name', ['lanes1/n5', 'edges1/gaussian-nonlinear/ekf', 'lanes2/n9', 'matrix2/gaussian/c1/ekf/D7',
                                  'matrix2/bernoulli_logistic/c0/ekf/D3'])
def test_first_nan_contract(frozen, name, bad):
    case = X.thaw(frozen, X.case(name))[0]
    B, t0 = 5, 7
    ys = np.ascontiguousarray(case.ys[np.arange(B) % case.R])
    clean = _device(case, B, ys=ys)
    assert np.all(clean[3] == -1)
    ys[2, t0] = bad
    means, covs, nells, first_nan = got = _device(case, B, ys=ys)
    T = ys.shape[1]
    finite = np.isfinite(means).all(axis=-1) & np.isfinite(covs).all(axis=(-1, -2)) & np.isfinite(nells)      # (B, T)
    first_bad = np.where(finite.all(axis=1), -1, np.argmin(finite, axis=1))
    npt.assert_array_equal(first_nan, first_bad, err_msg='first_nan is not the first step with a non-finite output')
    npt.assert_array_equal(first_nan, [-1, -1, t0, -1, -1])
    assert np.isnan(means[2, t0:]).all() and np.isnan(covs[2, t0:]).all() and np.isnan(nells[2, t0:]).all(), \
        'not every output is NaN from the poisoned step on'
    for b in range(B):
        upto = t0 if b == 2 else T
        for g, c in zip(got[:3], clean[:3]):
            assert np.array_equal(g[b, :upto], c[b, :upto]), f'replicate {b} differs from the clean run'


# ---- C.10 error codes of mfs_gaussian_filter_nd
def test_error_codes_nd(frozen):
    L = _lib.lib()
    case = X.thaw(frozen, X.case('lanes2/n9'))[0]
    T, B = 4, 1
    xi, w = np.ascontiguousarray(case.xi), np.ascontiguousarray(case.w)
    ys, m0, P0 = np.zeros((B, T)), np.zeros(2), np.eye(2)
    out = [np.empty((B, T, 2)), np.empty((B, T, 2, 2)), np.empty((B, T))]
    fn = np.empty(B, dtype=np.int32)
    EINVAL, EUNSUPPORTED = -1, -2

    def call(edit=None, method=0, n_points=9, T=T, B=B, ys=ys, nells=out[2]):
        model, keep = _struct(case.model, 1)
        if edit:
            edit(model)
        rc = L.mfs_gaussian_filter_nd(C.byref(model), method, n_points, _lib.ptr(xi), _lib.ptr(w), T, B, _lib.ptr(m0), _lib.ptr(P0),
                                      0, _lib.ptr(ys), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(nells), _lib.ptr(fn), 0, None)
        assert rc == 0 or b'mfs_gaussian_filter_nd' in L.mfs_last_error(), L.mfs_last_error()
        return rc

    def setter(**fields):
        def edit(model):
            for k, v in fields.items():
                if isinstance(v, tuple):
                    getattr(model, k)[v[0]] = v[1]
                else:
                    setattr(model, k, v)
        return edit

    for what, edit in (('d = 3', setter(d=3)), ('two factors', setter(n_factors=2)), ('ny = 2', setter(ny=2)),
                       ('a bearing factor', setter(fac_kind=(0, _lib.LIK['bearing_gaussian']))),
                       ('a factor of both components', setter(fac_component=(0, 2))), ('coef_batched', setter(coef_batched=1))):
        assert call(edit) == EUNSUPPORTED, what
    for what, edit in (('extent 0', setter(extent=0)), ('extent 8', setter(extent=8)),
                       ('an operator table', setter(trans_kind=_lib.ND_TRANS_OPERATOR))):
        assert call(edit) == EINVAL, what
    assert call(n_points=0) == EUNSUPPORTED and call(n_points=257) == EUNSUPPORTED
    assert call(ys=None) == EINVAL and call(nells=None) == EINVAL and call(T=0) == EINVAL and call(B=0) == EINVAL
    assert call(method=2) == EINVAL
    assert call() == 0 and np.all(np.isfinite(out[2])) and fn[0] == -1      # the library is still usable
