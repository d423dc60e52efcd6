"""Host side of the d = 3 N-D path: Stein recursion, dense tables, the kappa order, refusals and the C struct (no GPU)."""
import ctypes as C
import math
import os
import re

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats, sym
from mfs_amd.multi_dims import filtering, moments
from mfs_amd.multi_dims.multi_indices import generate_graded_lexico_multi_indices, gram_and_hankel_indices_graded_lexico
from mfs_amd.tme_poly_nd import stein_moments_3d
from oracle import multi_dims as omd, tme_sympy
from tests.nd3_models import LV_DT, MODELS
from tests.nd_support import host_disp, host_drift

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mfs_hip.h')


LORENZ, LV = MODELS['lorenz'], MODELS['lv']
_lorenz, _disp = host_drift(LORENZ), host_disp(LORENZ)      # the forms the host traces


def test_stein_recursion_matches_kan():
    rng = np.random.default_rng(3)
    mi = generate_graded_lexico_multi_indices(3, 7)
    for _ in range(4):
        m = rng.normal(size=3)
        A = rng.normal(size=(3, 3))
        S = A @ A.T + 0.1 * np.eye(3)
        got = stein_moments_3d(list(m), S.tolist(), mi)
        want = np.array([omd.raw_moments_mvn_kan(m, S, n) for n in mi])
        npt.assert_allclose(got, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize('order', ['euler', 2])
def test_normal_closure_cond_moments_match_oracle(order):
    rng = np.random.default_rng(5)
    mi = generate_graded_lexico_multi_indices(3, 5)
    dt = 0.01
    if order == 'euler':
        fns = moments.sde_cond_moments_euler_maruyama(_lorenz, _disp, dt, mi)
    else:
        fns = moments.sde_cond_moments_tme_normal(_lorenz, _disp, dt, order, mi)
    _, ocms, omean = tme_sympy.sde_cond_moments_normal_nd(LORENZ.drift, LORENZ.disp, 3, dt, order, mi)
    x = rng.normal(scale=0.5, size=(6, 3))
    c = rng.normal(scale=0.3, size=3)
    idx = np.arange(mi.shape[0])
    want = ocms(x, idx, c)
    got = fns[1](x, idx, c)
    npt.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    npt.assert_allclose(fns[3](x), omean(x), rtol=1e-12)


@pytest.mark.parametrize('order', ['euler', 2, 3])
def test_lotka_volterra_normal_closures_match_kan(order):
    """The host closures that tests/nd3_models.py hands the oracle for the Normal families, on the model with a
    state-dependent dispersion (3-species Lotka--Volterra) and at TME order 3: against the oracle's per-node Kan moments."""
    rng = np.random.default_rng(6)
    mi = generate_graded_lexico_multi_indices(3, 7)
    drift, disp = host_drift(LV), host_disp(LV)
    if order == 'euler':
        fns = moments.sde_cond_moments_euler_maruyama(drift, disp, LV_DT, mi)
    else:
        fns = moments.sde_cond_moments_tme_normal(drift, disp, LV_DT, order, mi)
    _, ocms, omean = tme_sympy.sde_cond_moments_normal_nd(LV.drift, LV.disp, 3, LV_DT, order, mi)
    x = 1. + rng.normal(scale=0.3, size=(6, 3))
    c = 1. + rng.normal(scale=0.1, size=3)
    idx = np.arange(mi.shape[0])
    want = ocms(x, idx, c)
    npt.assert_allclose(fns[1](x, idx, c), want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    npt.assert_allclose(fns[3](x), omean(x), rtol=1e-12)
    scale = np.array([0.2, 0.3, 0.25])
    npt.assert_allclose(fns[2](x, idx, c, scale), want / np.prod(scale ** mi, axis=-1), rtol=1e-9,
                        atol=1e-12 * np.abs(want / np.prod(scale ** mi, axis=-1)).max())


def test_operator_dense_table_matches_sympy():
    """The d = 3 operator rows, evaluated at random points through the kernel's row order, against the oracle's SymPy TME."""
    rng = np.random.default_rng(7)
    mi = generate_graded_lexico_multi_indices(3, 5)
    dt = 0.01
    fns = moments.sde_cond_moments_tme(_lorenz, _disp, dt, 2, d=3)
    tables = fns[0].tables
    m, (coef, _) = filtering._model_struct3(tables, filtering._trace_likelihood(_gauss_pdf, 3))
    assert coef.shape[0] == _lib.ND3_ROWS and m.n_terms == _lib.ND3_TERMS
    D = coef.shape[1]
    x = rng.normal(scale=0.5, size=(5, 3))
    c = rng.normal(scale=0.3, size=3)

    def poly(blk, pts):
        out = np.zeros(pts.shape[0])
        for a in range(D):
            for b in range(D):
                for e in range(D):
                    out += blk[a, b, e] * pts[:, 0] ** a * pts[:, 1] ** b * pts[:, 2] ** e
        return out

    Q = [poly(coef[r], x) for r in range(_lib.ND3_TERMS)]
    dx = x - c
    got = np.zeros((x.shape[0], mi.shape[0]))
    for zi, n in enumerate(mi):
        v = np.prod(dx ** n, axis=-1)
        for r, kap in enumerate(_lib.ND3_KAPPAS):
            if all(k <= nn for k, nn in zip(kap, n)):
                ff = math.prod(math.perm(int(nn), int(k)) for nn, k in zip(n, kap))
                v = v + Q[r] * ff * np.prod(dx ** (n - np.asarray(kap)), axis=-1)
        got[:, zi] = v
    _, ocms, omean, omv = tme_sympy.sde_cond_moments_tme_nd(LORENZ.drift, LORENZ.disp, 3, dt, 2, mi)
    want = ocms(x, mi, c)
    npt.assert_allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    # variance rows (scaled mode)
    var = np.stack([poly(coef[_lib.ND3_TERMS + k], x) for k in range(3)], axis=-1)
    npt.assert_allclose(var, omv(x)[1], rtol=1e-10, atol=1e-14)
    # the host's own evaluation agrees too
    npt.assert_allclose(fns[1](x, mi, c), want, rtol=1e-9, atol=1e-12 * np.abs(want).max())


def test_kappa_order_is_the_graded_lex_table():
    assert _lib.ND3_KAPPAS == [tuple(int(v) for v in k) for k in generate_graded_lexico_multi_indices(3, 4, 1)]
    assert len(_lib.ND3_KAPPAS) == _lib.ND3_TERMS == _lib.ND3_ROWS - 3


def _header_value(name):
    txt = open(_HEADER).read()
    return int(re.search(rf'#define {name} (\d+)', txt).group(1))


def test_nd3_struct_and_constants_match_header():
    assert C.sizeof(_lib.MfsModelNd3) == (5 + 4 * 3 + 2) * 4 + 4 + 2 * 8
    assert _lib.MfsModelNd3.coef.offset == 80
    assert (_header_value('MFS_ND3_MIN_N'), _header_value('MFS_ND3_MAX_N')) == (_lib.ND3_MIN_N, _lib.ND3_MAX_N)
    assert (_header_value('MFS_ND3_TERMS'), _header_value('MFS_ND3_ROWS'), _header_value('MFS_ND3_GAUSS_TERMS')) == \
           (_lib.ND3_TERMS, _lib.ND3_ROWS, _lib.ND3_GAUSS_TERMS)
    assert (_header_value('MFS_ND3_MAX_EXTENT'), _header_value('MFS_ND3_MAX_FACTORS')) == \
           (_lib.ND3_MAX_EXTENT, _lib.ND3_MAX_FACTORS)
    names = [n for n, _, _ in _lib._SIGNATURES]
    for n in ('mfs_filter_nd3', 'mfs_plan_nd3_create', 'mfs_plan_nd3_run', 'mfs_plan_nd3_destroy', 'mfs_plan_nd3_geometry'):
        assert n in names and n in _lib.DECLARED_SYMBOLS


def _gauss_pdf(y, x):
    return stats.norm_pdf(y, x[0], 0.5)


def _setup(N, tme_order=2):
    mi = generate_graded_lexico_multi_indices(3, 2 * N - 1)
    inds = gram_and_hankel_indices_graded_lexico(N, 3)
    fns = moments.sde_cond_moments_tme(_lorenz, _disp, 0.01, tme_order, d=3)
    m0 = np.array([omd.raw_moments_mvn_kan(np.zeros(3), 0.1 * np.eye(3), n) for n in mi])
    return mi, inds, fns, m0


def test_refusals():
    ys = np.zeros((2, 4))
    # N outside 2..4 at d = 3
    mi, inds, fns, m0 = _setup(5)
    with pytest.raises(sym.NotDeviceDescribable):
        filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], _gauss_pdf, ys, (mi, inds), m0, np.zeros(3))
    # operator tables beyond TME order 2
    mi, inds, fns, m0 = _setup(2, tme_order=3)
    with pytest.raises(sym.NotDeviceDescribable):
        filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], _gauss_pdf, ys, (mi, inds), m0, np.zeros(3))
    # d >= 4
    mi4 = generate_graded_lexico_multi_indices(4, 3)
    inds4 = gram_and_hankel_indices_graded_lexico(2, 4)
    fns4 = moments.sde_cond_moments_tme(lambda x: -x, lambda x: np.eye(4).astype(object), 0.01, 1, d=4)
    with pytest.raises(sym.NotDeviceDescribable):
        filtering.moment_filter_nd_cms((fns4[1], 'multi-index'), fns4[3], _gauss_pdf, ys, (mi4, inds4),
                                       np.zeros(mi4.shape[0]), np.zeros(4))
    # a likelihood of several components (the bearing kind)
    mi, inds, fns, m0 = _setup(2)

    def bearing(y, x):
        return stats.norm_pdf(y, sym.arctan2(x[1], x[0]), 0.1)

    with pytest.raises(sym.NotDeviceDescribable):
        filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], bearing, ys, (mi, inds), m0, np.zeros(3))
    # coefficient extent beyond MFS_ND3_MAX_EXTENT (a degree-6 drift)
    fns6 = moments.sde_cond_moments_tme(lambda x: -x ** 6, _disp, 0.01, 1, d=3)
    with pytest.raises(sym.NotDeviceDescribable):
        filtering.moment_filter_nd_cms((fns6[1], 'multi-index'), fns6[3], _gauss_pdf, ys, (mi, inds), m0, np.zeros(3))
