"""The d = 3 moment filters (filternd3_kernel) across the envelope the ABI promises: N = 2..4 in raw, central and scaled
modes, with and without `stable`; operator TME-1 / TME-2 tables and the TME-normal-2 / -3 and Euler closures; a
state-dependent dispersion (3-species Lotka--Volterra, diag(sigma_k x_k)) whose coefficient blocks fill all three bytes of
`ext` up to extent 5; every non-joint likelihood kind, on every component, read from out-of-order y-columns, two factors on
one component; per-replicate likelihood parameters, tables and initial states; NaN measurements; empty shapes; reversal of
the state components; and the long-horizon fixture tests/golden/filter_nd3.npz (tests/golden/make_nd3_golden.py).

Oracles: oracle/multi_dims.py with the SymPy TME tables of oracle/tme_sympy.py for the operator families; for the Normal
closures the host's vectorised Stein closure, which tests/test_host_nd3.py pins to the oracle's per-node Kan moments (one
case here runs the Kan closure itself).  The bar is that of tests/test_gpu_nd3.py: 1e-6 relative on NLL, means, scales and
moments, with the natural-magnitude floor.  Where a test uses another bound, it says where the bound comes from."""
import math
import os

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import stats, sym
from mfs_amd.multi_dims import filtering, moments
from mfs_amd.multi_dims.moments import marginalise_moments
from mfs_amd.one_dim import filtering as f1, moments as m1
from oracle import models as om, multi_dims as omd, one_dim as o1, tme_sympy
from tests.nd3_models import (C0, DT, LV_A, LV_C0, LV_DT, LV_M0, LV_SD, LV_SIG, M0, MODELS, family, lorenz_disp, lorenz_drift,
                              lv_model, lv_path, lv_pdf, lv_ys)
from tests.nd_support import (KIND_NAMES, MODES, MOMENTS_OF, RTOL, assert_state, compare, factor_pdfs, first_bad, host_disp,
                              host_drift, initial, moment_err, run_device, run_oracle, same_bits, stack_initial, tables)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'filter_nd3.npz')


# ---------------------------------------------------------------------------------------------------------------------
# the rule reproduces its input moments
# ---------------------------------------------------------------------------------------------------------------------
_L = np.array([[0.5, 0., 0.], [0.2, 0.15, 0.], [-0.1, 0.05, 0.3]])
RULE_MEAN = np.array([0.4, -0.7, 1.1])
RULE_COV = _L @ _L.T                    # correlated, anisotropic (sd 0.5, 0.25, 0.32)


def _oracle_rule_err(mode, st, mi, inds, stable):
    """The oracle's own reproduction error on the same input: one oracle.multi_dims.moment_quadrature_nd rule integrating
    the monomials of the table in the mode's coordinates (max _moment_err)."""
    key = MOMENTS_OF[mode]
    if mode == 'raw':
        w, x = omd.moment_quadrature_nd(st['rms'], inds, ldl=stable)
        u = x
    elif mode == 'central':
        w, x = omd.moment_quadrature_nd(st['cms'], inds, st['mean'], ldl=stable)
        u = x - st['mean']
    else:
        w, x = omd.moment_quadrature_nd(st['scms'], inds, st['mean'], st['scale'], ldl=stable)
        u = (x - st['mean']) / st['scale']
    rep = np.einsum('i,ij->j', w, np.prod(u[:, None, :] ** mi[None, :, :], axis=-1))
    return float(moment_err(rep[None], st[key][None], mi).max())


@pytest.mark.parametrize('stable', [False, True])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N', [2, 3, 4])
def test_rule_reproduces_its_input_moments(N, mode, stable):
    """Every predict and every update is "build the rule, integrate the monomials": an identity transition
    (cond_moments_linear_gaussian(I, Q)) and a likelihood that does not depend on the state (a Gaussian factor with l0 = 0).

    raw / central: Q = 0, so the moments must stay those of the start at every step and the NLL is sum_t -log N(y_t; 0.3, 1).
    scaled: the reference's prediction takes the scale from E[var(X' | x)] (mfs/multi_dims/filtering.py:181-190), which
    Q = 0 makes 0; Q = q C0 instead, so the law after step t is N(m0, (1 + q (t + 1)) C0) exactly: the scaled moments
    and the means stay constant, the scales grow by sqrt(1 + q (t + 1)).

    Bound: the oracle's own error for one rule on the same input (_oracle_rule_err), times the 2 T rules of the run (their
    errors add at most linearly), times 10 for the device's eigensolver (cyclic Jacobi) against LAPACK's."""
    T, B = 20, 2
    mi, inds = tables(3, N)
    st = initial(mi, RULE_MEAN, RULE_COV)
    q = 0.05 if mode == 'scaled' else 0.
    fns = moments.cond_moments_linear_gaussian(np.eye(3), q * RULE_COV, mi)
    ys = np.random.default_rng(N).normal(size=(B, T))
    got = run_device(mode, fns, 'index', lambda y, x: stats.norm_pdf(y, 0. * x[2] + 0.3, 1.), ys, mi, inds, st, stable)
    e1 = _oracle_rule_err(mode, st, mi, inds, stable)
    bound = 10 * 2 * T * max(e1, np.finfo(float).eps)
    key = MOMENTS_OF[mode]
    want = {'m': np.broadcast_to(st[key], (T, mi.shape[0]))}
    if mode != 'raw':
        want['mean'] = np.broadcast_to(st['mean'], (T, 3))
    if mode == 'scaled':
        want['scale'] = st['scale'] * np.sqrt(1. + q * np.arange(1, T + 1))[:, None]
    nell = np.sum(0.5 * (ys - 0.3) ** 2 + 0.5 * math.log(2 * math.pi), axis=1)
    assert np.all(got['fn'] == -1)
    print(f'N={N} {mode} stable={stable}: oracle one-rule error {e1:.2e}, device after {2 * T} rules '
          f'{max(moment_err(got["m"][b], want["m"], mi).max() for b in range(B)):.2e}, bound {bound:.2e}')
    for b in range(B):
        assert_state(got, b, want, mi, T, bound, f'N={N} {mode} stable={stable}')
        assert abs(got['nell'][b] - nell[b]) <= bound * abs(nell[b])


# ---------------------------------------------------------------------------------------------------------------------
# independent components reduce to three 1-D filters
# ---------------------------------------------------------------------------------------------------------------------
def test_independent_components_reduce_to_three_1d_filters():
    """Diagonal linear drift, diagonal dispersion, a product start and one Gaussian factor per component, factor k reading
    y-column k (reference tests/test_filtering.py:244-302 at d = 3).  The identity holds only up to the truncation of the
    tensor rule (and of TME-2 on products), so the device's d = 3 vs 1-D gap is bounded by the oracle's own d = 3 vs 1-D
    gap plus the parity bar on each side (2e-6); the device's d = 3 run is also held to the d = 3 oracle at 1e-6."""
    N, T, dt = 3, 15, 0.1
    a, bdisp, sd = np.array([-1.0, -0.6, -1.5]), np.array([0.3, 0.5, 0.4]), np.array([0.5, 0.8, 0.6])
    m0, v0 = np.array([0.2, -0.4, 0.6]), np.array([0.2, 0.1, 0.3])
    mi, inds = tables(3, N)
    st = initial(mi, m0, np.diag(v0))
    ys = np.array([0.3, -0.2, 0.5]) + np.random.default_rng(17).normal(size=(T, 3)) * 0.7

    def drift(x):
        return [float(a[k]) * x[k] for k in range(3)]

    def disp(x):
        return [[float(bdisp[i]) if i == j else 0. for j in range(3)] for i in range(3)]

    def pdf(y, x):
        return stats.norm_pdf(y[0], x[0], sd[0]) * stats.norm_pdf(y[1], x[1], sd[1]) * stats.norm_pdf(y[2], x[2], sd[2])

    def opdf(y, x):
        return float(np.prod(om.norm_pdf(y, x, sd)))

    fns = moments.sde_cond_moments_tme(lambda x: np.array(drift(x), dtype=object), lambda x: np.array(disp(x), dtype=object),
                                       dt, 2, d=3)
    got = run_device('central', fns, 'multi-index', pdf, ys[None], mi, inds, st)
    _, ocms, omean, _ = tme_sympy.sde_cond_moments_tme_nd(drift, disp, 3, dt, 2, mi)
    ref = omd.moment_filter_nd_cms((ocms, 'multi-index'), omean, opdf, ys, (mi, inds), st['cms'], m0)
    assert compare(got, 0, {'m': ref[0], 'mean': ref[1], 'nell': ref[2]}, mi, inds, 'independent d = 3') == T
    mi1 = np.arange(2 * N)[:, None]
    nell_dev, nell_ora = 0., 0.
    for k in range(3):
        cms0 = np.array([m1.central_moment_of_normal(v0[k], p) for p in range(2 * N)])
        f1d = m1.sde_cond_moments_tme(lambda x, k=k: float(a[k]) * x, lambda _, k=k: float(bdisp[k]), dt, 2)
        c1, me1, n1 = f1.moment_filter_cms(f1d[1], f1d[3], lambda y, x, k=k: stats.norm_pdf(y, x, sd[k]), cms0, m0[k],
                                           ys[:, k])
        of = tme_sympy.sde_cond_moments_tme_1d(lambda x, k=k: float(a[k]) * x, lambda x, k=k: float(bdisp[k]), dt, 2, 2 * N)
        oc1, ome1, on1 = o1.moment_filter_cms(of[1], of[3], lambda y, x, k=k: om.norm_pdf(y, x, sd[k]), cms0, m0[k], ys[:, k])
        gap_ora = moment_err(marginalise_moments(ref[0], 3, N, k), oc1, mi1).max()
        gap_dev = moment_err(marginalise_moments(got['m'][0], 3, N, k), c1, mi1).max()
        assert gap_dev <= gap_ora + 2 * RTOL, f'component {k}: moments {gap_dev:.3e} vs the oracle gap {gap_ora:.3e}'
        floor = 1e-2 * np.sqrt(oc1[:, 2])
        gap_ora = (np.abs(ref[1][:, k] - ome1) / np.maximum(np.abs(ome1), floor)).max()
        gap_dev = (np.abs(got['mean'][0, :, k] - me1) / np.maximum(np.abs(ome1), floor)).max()
        assert gap_dev <= gap_ora + 2 * RTOL, f'component {k}: means {gap_dev:.3e} vs the oracle gap {gap_ora:.3e}'
        nell_dev, nell_ora = nell_dev + n1, nell_ora + on1
    gap_ora = abs(ref[2] - nell_ora) / abs(nell_ora)
    assert abs(got['nell'][0] - nell_dev) / abs(nell_ora) <= gap_ora + 2 * RTOL


# ---------------------------------------------------------------------------------------------------------------------
# models and paths against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _extents(coef):
    """(ea, eb, ec) of every coefficient block, as mfs_plan_nd3_create packs them into ext."""
    out = []
    for blk in coef:
        nz = np.nonzero(blk)
        out.append(tuple(int(v.max()) + 1 if v.size else 0 for v in nz))
    return out


@pytest.mark.parametrize('fam,min_extent', [('tme_2', 5), ('tme_normal_3', 4)])
def test_lotka_volterra_tables_fill_every_extent_byte(fam, min_extent):
    """What the Lotka--Volterra tests run through the kernel: coefficient blocks of extent >= 5 (TME-2) / 4 (TME-normal-3)
    that are not constant in any of the three variables, so that every byte of ext = ea | eb << 8 | ec << 16 matters."""
    fns, _, _ = family('lv', fam, 3)
    model, keep = filtering._model_struct3(fns[0].tables, filtering._trace_likelihood(lv_pdf, 3))
    assert model.extent >= min_extent
    ext = np.array(_extents(keep[0]))
    assert ext.max() >= min_extent
    assert all(np.any(ext[:, k] >= 3) for k in range(3))


LV_CASES = ([(2, fam, mode, False, 8) for fam in ('tme_1', 'tme_2', 'tme_normal_2', 'tme_normal_3') for mode in MODES] +
            [(3, 'tme_1', 'raw', False, 4), (3, 'tme_2', 'central', False, 4), (3, 'tme_2', 'scaled', False, 4),
             (3, 'tme_normal_2', 'scaled', False, 4), (3, 'tme_normal_3', 'central', False, 4),
             (3, 'tme_normal_3', 'raw', False, 4),
             (4, 'tme_2', 'central', False, 2), (4, 'tme_1', 'scaled', False, 2), (4, 'tme_2', 'raw', False, 2),
             (4, 'tme_normal_3', 'central', False, 2),
             # stable = True (the LDL^T completion) at N = 2 and N = 4, raw and scaled
             (2, 'tme_2', 'raw', True, 8), (2, 'tme_2', 'scaled', True, 8), (4, 'tme_2', 'raw', True, 2),
             (4, 'tme_normal_2', 'scaled', True, 2)])


@pytest.mark.parametrize('N,fam,mode,stable,T', LV_CASES)
def test_lotka_volterra_against_the_oracle(N, fam, mode, stable, T):
    """The 3-species Lotka--Volterra model (state-dependent dispersion), a Gaussian factor on x_0 and a Poisson-softplus
    factor on x_2; replicate 1 of a batch of 2 against the oracle.  Raw mode at N = 4 may meet a numerically singular Gram
    matrix: compare() then applies the one-sided poisoning criterion instead of skipping."""
    mi, inds = tables(3, N)
    m = MODELS['lv']
    fns, sig, ofns = family('lv', fam, N)
    st = initial(mi, m.mean0, m.cov0)
    ys = m.ys(2, T, 100 + N)
    got = run_device(mode, fns, sig, m.pdf, ys, mi, inds, st, stable)
    ref = run_oracle(mode, ofns, sig, m.opdf, ys[1], mi, inds, st, stable, completed=True)
    upto = compare(got, 1, ref, mi, inds, f'lv N={N} {fam} {mode} stable={stable}')
    assert upto == T or (mode == 'raw' and N == 4)


@pytest.mark.parametrize('N,T,mode,kan', [(2, 8, 'central', True), (3, 4, 'scaled', False), (3, 4, 'raw', False)])
def test_lorenz_tme_normal_3(N, T, mode, kan):
    """Lorenz-63 with the TME-normal-3 closure; at N = 2 against the oracle's own per-node Kan closure
    (oracle/tme_sympy.py sde_cond_moments_normal_nd)."""
    mi, inds = tables(3, N)
    m = MODELS['lorenz']
    fns, sig, ofns = family('lorenz', 'tme_normal_3', N)
    if kan:
        orms, ocms, omean = tme_sympy.sde_cond_moments_normal_nd(lorenz_drift, lorenz_disp, 3, DT, 3, mi)
        ofns = (orms, ocms, None, omean, None)
    st = initial(mi, m.mean0, m.cov0)
    ys = m.ys(2, T, 50 + N)
    got = run_device(mode, fns, sig, m.pdf, ys, mi, inds, st)
    ref = run_oracle(mode, ofns, sig, m.opdf, ys[1], mi, inds, st, completed=True)
    assert compare(got, 1, ref, mi, inds, f'lorenz N={N} tme_normal_3 {mode}') == T


def factor_ys(spec, B, T, seed):
    """Measurements of the factors of `spec` along Lotka--Volterra paths, (B, T, ny)."""
    xs, rng = lv_path(B, T, seed)
    ys = np.zeros((B, T, max(c for _, _, c, _ in spec) + 1))
    for kind, j, c, p in spec:
        x = xs[..., j]
        if kind == 'gaussian':
            ys[..., c] = x + p * rng.standard_normal((B, T))
        elif kind == 'poisson':
            ys[..., c] = rng.poisson(np.log1p(np.exp(x * p)))
        else:
            ys[..., c] = rng.random((B, T)) < 1. / (1. + np.exp(-(x * p) + 1.))
    return ys


WIRING = {
    'x2_alone': [('gaussian', 2, 0, 0.3)],
    'bernoulli_x0': [('bernoulli', 0, 0, 3.0)],
    'poisson_x1_bernoulli_x2': [('poisson', 1, 0, 1.5), ('bernoulli', 2, 1, 2.0)],
    # factor 0 reads x_2 from column 1, factor 1 reads x_0 from column 0
    'out_of_order': [('gaussian', 2, 1, 0.3), ('poisson', 0, 0, 2.0)],
    # two factors on x_1 (columns 2 and 0) and a third, on x_0, between them
    'two_on_x1': [('gaussian', 1, 2, 0.3), ('bernoulli', 0, 1, 2.0), ('gaussian', 1, 0, 0.5)],
}


@pytest.mark.parametrize('case', list(WIRING))
def test_likelihood_wiring(case):
    """Each factor of the product reads its own component and y-column (fac_comp / fac_ycol), whatever the order of the
    factors, the components and the columns: Lotka--Volterra, TME-2, N = 3, central, against the oracle."""
    spec = WIRING[case]
    N, T = 3, 6
    mi, inds = tables(3, N)
    m = MODELS['lv']
    fns, sig, ofns = family('lv', 'tme_2', N)
    pdf, opdf = factor_pdfs(spec)
    assert [(f.kind, f.component, f.ycol) for f in filtering._trace_likelihood(pdf, 3)] == \
        [(KIND_NAMES[kind], j, c) for kind, j, c, _ in spec]
    st = initial(mi, m.mean0, m.cov0)
    ys = factor_ys(spec, 2, T, 7)
    got = run_device('central', fns, sig, pdf, ys, mi, inds, st)
    ref = run_oracle('central', ofns, sig, opdf, ys[0], mi, inds, st, completed=True)
    assert compare(got, 0, ref, mi, inds, case) == T


def test_per_replicate_likelihood_parameters_are_bit_identical_to_single_runs():
    """lik_batched: a Gaussian factor with a per-replicate sd and a Bernoulli factor with a per-replicate offset."""
    N, T, B = 2, 10, 3
    mi, inds = tables(3, N)
    m = MODELS['lv']
    fns, sig, _ = family('lv', 'tme_2', N)
    sds, offs = np.array([0.15, 0.3, 0.6]), np.array([0.5, 1.0, 2.0])

    def pdf_of(sd, c):
        return lambda y, x: stats.norm_pdf(y[0], x[0], sd) * stats.bernoulli_pmf(y[1], 1. / (1. + sym.exp(-(x[1] * 2.) + c)))

    model, _ = filtering._model_struct3(fns[0].tables, filtering._trace_likelihood(pdf_of(sds, offs), 3), B)
    assert model.lik_batched == 1
    st = initial(mi, m.mean0, m.cov0)
    ys = factor_ys([('gaussian', 0, 0, 0.3), ('bernoulli', 1, 1, 2.0)], B, T, 5)
    for mode in ('central', 'scaled'):
        got = run_device(mode, fns, sig, pdf_of(sds, offs), ys, mi, inds, st)
        assert np.all(got['fn'] == -1) and len(set(got['nell'].tolist())) == B
        for b in range(B):
            one = run_device(mode, fns, sig, pdf_of(float(sds[b]), float(offs[b])), ys[b:b + 1], mi, inds, st)
            same_bits({k: v[b:b + 1] for k, v in got.items()}, one)


def test_per_replicate_tables_and_initial_states_are_bit_identical_to_single_runs():
    """Per-replicate transition tables (batch_closures over the dispersion sigma) and per-replicate m0 / mean0 / scale0:
    each replicate has the bits of its own single-replicate run."""
    N, T, B = 2, 10, 3
    mi, inds = tables(3, N)
    per = [moments.sde_cond_moments_tme(host_drift(mdl), host_disp(mdl), LV_DT, 2, d=3)
           for mdl in (lv_model(sig=LV_SIG * f) for f in (0.5, 1.0, 2.0))]
    bfns = moments.batch_closures(per)
    ys = lv_ys(B, T, 9)
    st = initial(mi, LV_M0, LV_C0)
    for mode in MODES:
        got = run_device(mode, bfns, 'multi-index', lv_pdf, ys, mi, inds, st)
        assert np.all(got['fn'] == -1) and len(set(got['nell'].tolist())) == B
        for b in range(B):
            one = run_device(mode, per[b], 'multi-index', lv_pdf, ys[b:b + 1], mi, inds, st)
            same_bits({k: v[b:b + 1] for k, v in got.items()}, one)
    fns, sig, _ = family('lv', 'tme_2', N)
    shifts = np.array([[0., 0., 0.], [0.1, -0.05, 0.02], [-0.1, 0.1, 0.]])
    states = [initial(mi, LV_M0 + shifts[b], LV_C0 * f) for b, f in enumerate((1., 1.5, 0.7))]
    for mode in MODES:
        got = run_device(mode, fns, sig, lv_pdf, ys, mi, inds, stack_initial(states))
        assert np.all(got['fn'] == -1) and len(set(got['nell'].tolist())) == B
        for b in range(B):
            one = run_device(mode, fns, sig, lv_pdf, ys[b:b + 1], mi, inds, states[b])
            same_bits({k: v[b:b + 1] for k, v in got.items()}, one)


@pytest.mark.parametrize('mode', MODES)
def test_nan_measurement_poisons_its_replicate_from_that_step(mode):
    N, T, B, t_nan = 2, 12, 3, 7
    mi, inds = tables(3, N)
    fns, sig, _ = family('lv', 'tme_2', N)
    st = initial(mi, LV_M0, LV_C0)
    ys = lv_ys(B, T, 21)
    clean = run_device(mode, fns, sig, lv_pdf, ys, mi, inds, st)
    assert np.all(clean['fn'] == -1)
    ys[1, t_nan, 0] = np.nan
    got = run_device(mode, fns, sig, lv_pdf, ys, mi, inds, st)
    assert list(got['fn']) == [-1, t_nan, -1]
    assert np.isnan(got['nell'][1])
    for k in ('m', 'mean', 'scale'):
        if k in got:
            assert np.all(np.isnan(got[k][1, t_nan:])), k
            npt.assert_array_equal(got[k][1, :t_nan], clean[k][1, :t_nan], err_msg=k)
            npt.assert_array_equal(got[k][[0, 2]], clean[k][[0, 2]], err_msg=k)
    npt.assert_array_equal(got['nell'][[0, 2]], clean['nell'][[0, 2]])


@pytest.mark.parametrize('mode', MODES)
def test_empty_batch_and_zero_steps(mode):
    """B = 0 gives empty outputs, T = 0 the initial state's shapes, a zero NLL and no poisoning."""
    N = 2
    mi, inds = tables(3, N)
    z = mi.shape[0]
    fns, sig, _ = family('lv', 'tme_2', N)
    st = initial(mi, LV_M0, LV_C0)
    ys = lv_ys(3, 5, 1)
    r = run_device(mode, fns, sig, lv_pdf, ys[:0], mi, inds, st)
    assert r['m'].shape == (0, 5, z) and r['nell'].shape == (0,) and r['fn'].shape == (0,)
    assert all(r[k].shape == (0, 5, 3) for k in ('mean', 'scale') if k in r)
    r = run_device(mode, fns, sig, lv_pdf, ys[:, :0], mi, inds, st)
    assert r['m'].shape == (3, 0, z)
    assert all(r[k].shape == (3, 0, 3) for k in ('mean', 'scale') if k in r)
    npt.assert_array_equal(r['nell'], np.zeros(3))
    npt.assert_array_equal(r['fn'], -np.ones(3))


# ---------------------------------------------------------------------------------------------------------------------
# long horizon against the frozen oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_long_horizon_golden_fixture():
    """tests/golden/filter_nd3.npz: Lorenz-63 and Lotka--Volterra with operator TME-2 tables, N = 3 at T = 200 and N = 4 at
    T = 50, central and scaled.  1e-6 at every step where both sides are finite, the same NaN pattern otherwise.  Lorenz-63 with
    the (non-closure) TME-2 tables loses a positive-definite Gram matrix in the oracle at step 15 (N = 3) / 9 (N = 4) of this
    record: the device must poison at that same step; the Lotka--Volterra runs stay finite over the whole horizon."""
    g = np.load(GOLDEN)
    for name, want in (('lv_A', LV_A), ('lv_sig', LV_SIG), ('lv_m0', LV_M0), ('lv_c0', LV_C0), ('lorenz_m0', M0),
                       ('lorenz_c0', C0)):
        npt.assert_array_equal(g[name], want, err_msg=name)
    assert float(g['lv_dt']) == LV_DT and float(g['lv_sd']) == LV_SD and float(g['lorenz_dt']) == DT
    for model in ('lorenz', 'lv'):
        m = MODELS[model]
        fns = moments.sde_cond_moments_tme(host_drift(m), host_disp(m), m.dt, 2, d=3)
        for N, T in ((3, 200), (4, 50)):
            mi, inds = tables(3, N)
            st = initial(mi, m.mean0, m.cov0)
            ys = g[f'{model}_ys'][None, :T]
            for mode in ('central', 'scaled'):
                key = f'{model}_N{N}_{mode}'
                ref = {'m': g[f'{key}_moments'], 'mean': g[f'{key}_means'], 'nell': float(g[f'{key}_nell'])}
                if mode == 'scaled':
                    ref['scale'] = g[f'{key}_scales']
                assert ref['m'].shape == (T, mi.shape[0])
                got = run_device(mode, fns, 'multi-index', m.pdf, ys, mi, inds, st)
                f_ora = first_bad(ref)
                assert int(got['fn'][0]) == f_ora, f'{key}: first NaN {got["fn"][0]} vs {f_ora}'
                assert_state(got, 0, ref, mi, T if f_ora < 0 else f_ora, RTOL, key)
                if f_ora < 0:
                    assert abs(got['nell'][0] - ref['nell']) <= RTOL * abs(ref['nell']), key
                else:
                    assert np.all(np.isnan(got['m'][0, f_ora:])) and np.isnan(got['nell'][0]), key


# ---------------------------------------------------------------------------------------------------------------------
# coordinate reversal
# ---------------------------------------------------------------------------------------------------------------------
REV = np.array([2, 1, 0])


@pytest.mark.parametrize('fam', ['tme_2', 'tme_normal_2'])
@pytest.mark.parametrize('mode', MODES)
def test_reversing_the_components_reverses_the_outputs(fam, mode):
    """Lotka--Volterra with x' = (x_2, x_1, x_0): A' = A[p][:, p], sigma' = sigma[p], the start, mean0 / scale0 and the
    factors' components permuted to match.  The outputs must be the permuted outputs.

    Why the reversal: the tensor rule's weights chain the components 0 - 1 - 2 (W = v0[0] <v0, v1> <v1, v2> v2[0],
    mfs/multi_dims/quadratures.py:165-170), and the K_k of the permuted law are orthogonally similar to the originals with
    the constant basis function fixed; the reversed chain therefore gives the same nodes and weights in exact arithmetic,
    where any other permutation changes the weights, and the integrals of non-polynomial likelihoods with them.  Both runs
    are the device's, summed in different orders: 1e-10, or where larger the rounding that the Gram matrix of the start can
    amplify over the 2 T rules of a run, 2 T cond(G0) eps (raw moments about the origin: cond(G0) = 2e5)."""
    N, T, B = 3, 10, 2
    p = REV
    mi, inds = tables(3, N)
    spec = [('gaussian', 0, 0, 0.2), ('poisson', 2, 1, 1.0), ('bernoulli', 1, 2, 2.0)]
    spec_p = [(kind, int(np.where(p == j)[0][0]), c, q) for kind, j, c, q in spec]
    ys = factor_ys(spec, B, T, 13)
    out = []
    for A, sig, m0, c0, sp in ((LV_A, LV_SIG, LV_M0, LV_C0, spec),
                               (LV_A[p][:, p], LV_SIG[p], LV_M0[p], LV_C0[p][:, p], spec_p)):
        mdl = lv_model(A, sig)
        if fam == 'tme_2':
            fns, sig_ = moments.sde_cond_moments_tme(host_drift(mdl), host_disp(mdl), LV_DT, 2, d=3), 'multi-index'
        else:
            fns, sig_ = moments.sde_cond_moments_tme_normal(host_drift(mdl), host_disp(mdl), LV_DT, 2, mi), 'index'
        out.append(run_device(mode, fns, sig_, factor_pdfs(sp)[0], ys, mi, inds, initial(mi, m0, c0)))
    # moment j of x' is the moment n of x with n[p] = n'_j
    idx = []
    for row in mi:
        n = np.zeros(3, dtype=int)
        n[p] = row
        idx.append(int(np.where((mi == n).all(axis=1))[0][0]))
    ref, got = out
    assert np.all(ref['fn'] == -1) and np.all(got['fn'] == -1)
    st = initial(mi, LV_M0, LV_C0)
    g0 = st[MOMENTS_OF[mode]][inds[0]]
    bound = max(1e-10, 2 * T * np.linalg.cond(g0) * np.finfo(float).eps)
    err = max(moment_err(got['m'][b], ref['m'][b][:, idx], mi).max() for b in range(B))
    print(f'{fam} {mode}: moments of the reversed run off by {err:.1e}, bound {bound:.1e}')
    for b in range(B):
        want = {'m': ref['m'][b][:, idx]}
        for k in ('mean', 'scale'):
            if k in ref:
                want[k] = ref[k][b][:, p]
        assert_state(got, b, want, mi, T, bound, f'{fam} {mode}')
        assert abs(got['nell'][b] - ref['nell'][b]) <= bound * abs(ref['nell'][b])
