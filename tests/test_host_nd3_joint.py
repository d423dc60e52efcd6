"""Host side of the d = 3 joint likelihood factors: tracing of each link and kind to the mfs_joint_nd3 descriptor, the
refusals of the tracer and of the C ABI, and the traces that must not change (bearing at d = 2, single-component factors)."""
import ctypes as C
import os
import re

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats, sym
from mfs_amd.multi_dims import filtering, moments
from mfs_amd.multi_dims.multi_indices import generate_graded_lexico_multi_indices, gram_and_hankel_indices_graded_lexico

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mfs_hip.h')
S = np.array([-5., -5., -2.])


def _trace(fn, d=3):
    return filtering._trace_likelihood(fn, d)


def _block(entries, E):
    """[E][E][E] block from {(a, b, c): coefficient of x0^a x1^b x2^c}."""
    out = np.zeros((E, E, E))
    for idx, v in entries.items():
        out[idx] = v
    return out


def test_product_traces_to_a_poly_link():
    (f,) = _trace(lambda y, x: stats.norm_pdf(y, x[0] * x[1], 0.5))
    assert isinstance(f, sym.JointLikelihoodSpec) and (f.kind, f.link, f.ycol) == ('gaussian', 'poly', 0)
    npt.assert_array_equal(f.coef[0], _block({(1, 1, 0): 1.}, 2))
    npt.assert_array_equal(f.coef[1], np.zeros((2, 2, 2)))
    npt.assert_allclose(f.params, [0.25])


def test_axes_of_the_coefficient_block_are_x0_x1_x2():
    (f,) = _trace(lambda y, x: stats.norm_pdf(y, 2. * x[0] ** 2 * x[2] + 3. * x[1] - 7. * x[2] + 1., 1.))
    npt.assert_array_equal(f.coef[0], _block({(2, 0, 1): 2., (0, 1, 0): 3., (0, 0, 1): -7., (0, 0, 0): 1.}, 3))


def test_range_azimuth_elevation_trace_to_the_three_links():
    def pdf(y, x):
        dx, dy, dz = x[0] - S[0], x[1] - S[1], x[2] - S[2]
        g = dx * dx + dy * dy
        return (stats.norm_pdf(y[0], sym.sqrt(g + dz * dz), 0.5) * stats.norm_pdf(y[1], sym.arctan2(dy, dx), 0.1)
                * stats.norm_pdf(y[2], sym.arctan2(dz, sym.sqrt(g)), 0.2))
    r, az, el = _trace(pdf)
    assert [(f.kind, f.link, f.ycol) for f in (r, az, el)] == [('gaussian', 'sqrt', 0), ('gaussian', 'atan2', 1),
                                                               ('gaussian', 'atan2_sqrt', 2)]
    ground = {(0, 0, 0): 50., (1, 0, 0): 10., (0, 1, 0): 10., (2, 0, 0): 1., (0, 2, 0): 1.}
    npt.assert_array_equal(r.coef[0], _block({**ground, (0, 0, 0): 54., (0, 0, 1): 4., (0, 0, 2): 1.}, 3))
    npt.assert_array_equal(az.coef[0], _block({(0, 0, 0): 5., (0, 1, 0): 1.}, 2))     # p = x1 - s1
    npt.assert_array_equal(az.coef[1], _block({(0, 0, 0): 5., (1, 0, 0): 1.}, 2))     # q = x0 - s0
    npt.assert_array_equal(el.coef[0], _block({(0, 0, 0): 2., (0, 0, 1): 1.}, 3))
    npt.assert_array_equal(el.coef[1], _block(ground, 3))
    npt.assert_allclose([r.params[0], az.params[0], el.params[0]], [0.25, 0.01, 0.04])
    joint, keep = filtering._joint_struct3([r, az, el])
    assert (joint.n_joint, joint.extent, joint.batched) == (3, 3, 0)
    assert list(joint.kind) == [2, 2, 2] and list(joint.link) == [1, 2, 3] and list(joint.ycol) == [0, 1, 2]
    assert keep[0].shape == (3, 2, 3, 3, 3)
    npt.assert_array_equal(keep[0][1, 0, :2, :2, :2], az.coef[0])     # the smaller block sits in the corner of the common extent


def test_poisson_and_bernoulli_kinds():
    (f,) = _trace(lambda y, x: stats.poisson_pmf(y, sym.log(1. + sym.exp(x[0] + x[1] + x[2]))))
    assert (f.kind, f.link) == ('poisson_softplus', 'poly')
    npt.assert_array_equal(f.coef[0], _block({(1, 0, 0): 1., (0, 1, 0): 1., (0, 0, 1): 1.}, 2))
    (f,) = _trace(lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-(2. * x[0] * x[1] - x[2] ** 2 + 0.5)))))
    assert (f.kind, f.link) == ('bernoulli_logistic', 'poly')
    npt.assert_array_equal(f.coef[0], _block({(1, 1, 0): 2., (0, 0, 2): -1., (0, 0, 0): 0.5}, 3))
    # a link under the logistic: 1 / (1 + exp(-sqrt(p)))
    (f,) = _trace(lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-sym.sqrt(x[0] * x[0] + x[1] * x[1])))))
    assert (f.kind, f.link) == ('bernoulli_logistic', 'sqrt')


def test_mixed_product_keeps_single_component_factors_single():
    fs = _trace(lambda y, x: stats.norm_pdf(y[1], x[2], 0.5) * stats.norm_pdf(y[0], x[0] * x[1], 0.5))
    assert type(fs[0]) is sym.LikelihoodSpec and (fs[0].kind, int(fs[0].component), fs[0].ycol) == ('gaussian', 2, 1)
    assert isinstance(fs[1], sym.JointLikelihoodSpec) and fs[1].ycol == 0


def test_existing_traces_are_unchanged():
    (b,) = _trace(lambda y, x: stats.norm_pdf(y, sym.arctan2(x[1], x[0]), 0.1), d=2)
    assert type(b) is sym.LikelihoodSpec and b.kind == 'bearing_gaussian' and b.component == 2
    for d in (1, 2, 3):
        (g,) = _trace(lambda y, x: stats.norm_pdf(y, 2. * (x if d == 1 else x[d - 1]) + 1., 0.5), d=d)
        assert type(g) is sym.LikelihoodSpec and g.kind == 'gaussian' and int(g.component) == d - 1
        npt.assert_allclose(g.params, [2., 1., 0.25])
    (p,) = _trace(lambda y, x: stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-x[1] ** 3 + 1.))), d=3)
    assert type(p) is sym.LikelihoodSpec and int(p.component) == 1
    npt.assert_allclose(p.params, [-1., 0., 0., 1.])
    # vector form: one factor per component
    fs = _trace(lambda y, x: np.prod(stats.norm_pdf(y, x, 0.5)), d=3)
    assert [int(f.component) for f in fs] == [0, 1, 2] and all(type(f) is sym.LikelihoodSpec for f in fs)


def test_tracer_refusals_name_the_limit():
    with pytest.raises(sym.NotDeviceDescribable, match='degree 4 exceeds'):
        _trace(lambda y, x: stats.norm_pdf(y, x[0] ** 4 * x[1], 0.5))
    with pytest.raises(sym.NotDeviceDescribable, match='cannot enter further arithmetic'):
        _trace(lambda y, x: stats.norm_pdf(y, sym.sqrt(sym.sqrt(x[0] * x[1]) + sym.sqrt(x[1] * x[2])), 0.5))
    with pytest.raises(sym.NotDeviceDescribable, match='arctan2 of this composition'):
        _trace(lambda y, x: stats.norm_pdf(y, sym.arctan2(sym.sqrt(x[0] * x[1]), x[2]), 0.5))
    with pytest.raises(sym.NotDeviceDescribable, match='batch_likelihoods'):
        _trace(lambda y, x: stats.norm_pdf(y, x[0] * x[1], np.array([0.5, 0.6])))
    with pytest.raises(sym.NotDeviceDescribable, match='at most 3'):
        _trace(lambda y, x: np.prod([stats.norm_pdf(y[k], x[0] * x[1] + k, 0.5) for k in range(4)]))
    # d = 2: products of components and arctan2 of polynomials stay refused, and say where they do run
    with pytest.raises(sym.NotDeviceDescribable, match='d = 3 only'):
        _trace(lambda y, x: stats.norm_pdf(y, x[0] * x[1], 0.5), d=2)
    with pytest.raises(sym.NotDeviceDescribable, match='d = 3 only'):
        _trace(lambda y, x: stats.norm_pdf(y, sym.arctan2(x[1] + 1., x[0]), 0.5), d=2)
    with pytest.raises(sym.NotDeviceDescribable, match='sqrt'):
        _trace(lambda y, x: stats.norm_pdf(y, sym.sqrt(x[0]), 0.5), d=2)


def test_batch_likelihoods_stacks_joint_and_single_factors():
    fn = stats.batch_likelihoods([lambda y, x, k=k: stats.norm_pdf(y[1], x[0] * x[1] + k, 0.5 + k)
                                  * stats.norm_pdf(y[0], x[2], 1. + k) for k in range(3)])
    j, s = _trace(fn)
    assert j.coef.shape == (3, 2, 2, 2, 2) and j.params.shape == (3, 1) and s.params.shape == (3, 3)
    npt.assert_array_equal(j.coef[:, 0, 0, 0, 0], [0., 1., 2.])
    npt.assert_allclose(j.params[:, 0], [0.25, 2.25, 6.25])
    joint, _ = filtering._joint_struct3([j], 3)
    assert joint.batched == 1
    with pytest.raises(ValueError, match='batch'):
        filtering._joint_struct3([j], 4)
    with pytest.raises(sym.NotDeviceDescribable, match='same factors'):
        _trace(stats.batch_likelihoods([lambda y, x: stats.norm_pdf(y, x[0] * x[1], 0.5),
                                        lambda y, x: stats.norm_pdf(y, sym.sqrt(x[0] * x[1]), 0.5)]))


def test_struct_and_constants_match_header():
    txt = open(_HEADER).read()
    val = lambda name: int(re.search(rf'#define {name} (\d+)', txt).group(1))   # noqa: E731
    assert (val('MFS_ND3_MAX_JOINT'), val('MFS_ND3_JOINT_MAX_EXTENT'), val('MFS_ND3_JOINT_MAX_NY')) == \
           (_lib.ND3_MAX_JOINT, _lib.ND3_JOINT_MAX_EXTENT, _lib.ND3_JOINT_MAX_NY)
    assert _lib.ND3_JOINT_MAX_EXTENT == sym.JOINT_MAX_EXTENT
    for name, code in _lib.ND3_LINK.items():
        assert val('MFS_ND3_LINK_' + name.upper()) == code == sym.JointLikelihoodSpec.LINKS[name]
    assert C.sizeof(_lib.MfsJointNd3) == (3 + 3 * 3) * 4 + 2 * 8 and _lib.MfsJointNd3.coef.offset == 48


# ---- C ABI refusals: validation happens before any device call, so these run without a GPU ----
def _abi_setup(link=0, kind=2, extent=2, ycol=0, n_joint=1, ny=1, n_factors=0):
    N = 2
    mi = np.ascontiguousarray(generate_graded_lexico_multi_indices(3, 2 * N - 1), dtype=np.int32)
    inds = np.ascontiguousarray(gram_and_hankel_indices_graded_lexico(N, 3), dtype=np.int32)
    fns = moments.sde_cond_moments_tme(lambda x: -x, lambda x: np.eye(3).astype(object), 0.01, 1, d=3)
    model, keep = filtering._model_struct3(fns[1].tables, [], 1, ny=ny)
    model.n_factors = n_factors
    coef, par = np.zeros((3, 2, 4, 4, 4)), np.ones(3)
    j = _lib.MfsJointNd3()
    j.n_joint, j.extent, j.batched = n_joint, extent, 0
    j.kind[0], j.link[0], j.ycol[0] = kind, link, ycol
    j.coef, j.par = coef.ctypes.data_as(_lib.c_double_p), par.ctypes.data_as(_lib.c_double_p)
    return N, mi, inds, model, j, (keep, coef, par)


@pytest.mark.parametrize('kw,code,msg', [
    (dict(link=4), -1, b'unknown link'), (dict(link=-1), -1, b'unknown link'),
    (dict(kind=3), -1, b'kind 3'), (dict(extent=5), -2, b'extent 5'), (dict(extent=0), -2, b'extent 0'),
    (dict(ycol=1), -1, b'measurement column 1'), (dict(ycol=2, ny=2), -1, b'measurement column 2'),
    (dict(n_joint=4), -1, b'n_joint 4'), (dict(n_joint=0), -1, b'n_joint 0'), (dict(ny=7), -1, b'ny 7'),
    (dict(n_factors=4), -1, b'n_factors 4'),
])
def test_abi_refuses_bad_joint_descriptors(kw, code, msg):
    N, mi, inds, model, j, keep = _abi_setup(**kw)
    L = _lib.lib()
    plan = C.c_void_p()
    rc = L.mfs_plan_nd3_create_joint(C.byref(plan), C.byref(model), C.byref(j), 1, N, 4, 1, mi.shape[0], _lib.ptr(mi),
                                     _lib.ptr(inds), 0, 0)
    assert rc == code and msg in L.mfs_last_error() and not plan.value
    del keep


def test_abi_refuses_a_null_joint_and_keeps_the_plain_entry_point_strict():
    N, mi, inds, model, j, keep = _abi_setup()
    L = _lib.lib()
    plan = C.c_void_p()
    assert L.mfs_plan_nd3_create_joint(C.byref(plan), C.byref(model), None, 1, N, 4, 1, mi.shape[0], _lib.ptr(mi),
                                       _lib.ptr(inds), 0, 0) == -1 and b'joint is NULL' in L.mfs_last_error()
    assert L.mfs_filter_nd3_joint(C.byref(model), None, 1, N, 4, 1, mi.shape[0], _lib.ptr(mi), _lib.ptr(inds), None, 0, None,
                                  None, None, 0, None, None, None, None, None, 0, None) == -1
    # without joint factors a model still needs 1..3 single-component factors
    assert L.mfs_plan_nd3_create(C.byref(plan), C.byref(model), 1, N, 4, 1, mi.shape[0], _lib.ptr(mi), _lib.ptr(inds), 0,
                                 0) == -1 and b'n_factors 0' in L.mfs_last_error()
    del keep
