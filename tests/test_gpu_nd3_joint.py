"""Joint likelihood factors at d = 3 (filternd3_joint_kernel): factors kind(y; u(x)) with u = p, sqrt(p), atan2(p, q) or
atan2(p, sqrt(q)) of trivariate polynomials, against the oracle's N-D filters, whose measurement density is any Python
callable of (y, x).

Bar: that of tests/test_gpu_nd3.py and tests/test_gpu_nd3_envelope.py (`compare` of tests/nd_support.py: 1e-6 relative on
NLL, means, scales and moments with the natural-magnitude floor; under stable=True the comparison stops at the first LDL^T
completion).

Inputs were chosen so that the ORACLE ALONE stays finite: every (case, N, family, mode, stable) combination of
`PARITY` was run through oracle/multi_dims.py alone on the CPU, with the data of this file; none of the 50 poisons.  The
horizons are T = 16 / 10 / 3 at N = 2 / 3 / 4 for the Lorenz cases: with this file's data the N = 2 operator filters of the
oracle poison at step 28 (product), 21 (range-azimuth-elevation) and 27 (mixed) of 30, so T = 16 stays well clear of them;
range-azimuth-elevation at N = 3 runs T = 8.  The Lotka--Volterra cases run T = 20 / 8 / 3 (Poisson counts of
softplus(x0 + x1 + x2) ~ 3; Bernoulli draws of a degree-2 logit).  Each headline test asserts that the oracle run is finite, so
a comparison of NaN patterns cannot pass for a comparison of numbers.
"""
import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import stats, sym
from mfs_amd.multi_dims import filtering, moments, ss_models
from oracle import models as om
from tests.nd3_models import C0, LV_C0, LV_M0, M0, family, lorenz_path, lv_path
from tests.nd_support import MODES, compare, first_bad, initial, moment_err, run_device, run_oracle, same_bits, tables
from tests.plan_api import run_plan_nd

pytestmark = pytest.mark.gpu

SENSOR = np.array([-5., -5., -2.])
PROD_SD, RANGE_SD, ANGLE_SD = 0.5, 0.5, 0.1


# ---- the measurement models: device callable (traced), oracle callable (numbers), data ----
def rae_of(x, s):
    """Noise-free (range, azimuth, elevation) of the position(s) x (..., 3) from the sensor s."""
    d = np.asarray(x) - s
    ground = d[..., 0] ** 2 + d[..., 1] ** 2
    return np.stack([np.sqrt(ground + d[..., 2] ** 2), np.arctan2(d[..., 1], d[..., 0]), np.arctan2(d[..., 2], np.sqrt(ground))],
                    axis=-1)


def product_pdf(sd=PROD_SD):
    return lambda y, x: stats.norm_pdf(y, x[0] * x[1], sd)


def product_opdf(sd=PROD_SD):
    return lambda y, x: float(om.norm_pdf(y, x[0] * x[1], sd))


def product_ys(B, T, seed, sd=PROD_SD):
    xs, rng = lorenz_path(B, T, seed)
    return xs[..., 0] * xs[..., 1] + sd * rng.standard_normal((B, T))


def rae_pdf(s=SENSOR, range_sd=RANGE_SD, angle_sd=ANGLE_SD):
    def pdf(y, x):
        dx, dy, dz = x[0] - s[0], x[1] - s[1], x[2] - s[2]
        ground = dx * dx + dy * dy
        return (stats.norm_pdf(y[0], sym.sqrt(ground + dz * dz), range_sd) * stats.norm_pdf(y[1], sym.arctan2(dy, dx), angle_sd)
                * stats.norm_pdf(y[2], sym.arctan2(dz, sym.sqrt(ground)), angle_sd))
    return pdf


def rae_opdf(s=SENSOR, range_sd=RANGE_SD, angle_sd=ANGLE_SD):
    def opdf(y, x):
        r, az, el = rae_of(np.asarray(x, dtype=float), s)
        return float(om.norm_pdf(y[0], r, range_sd) * om.norm_pdf(y[1], az, angle_sd) * om.norm_pdf(y[2], el, angle_sd))
    return opdf


def rae_ys(B, T, seed, s=SENSOR, range_sd=RANGE_SD, angle_sd=ANGLE_SD):
    xs, rng = lorenz_path(B, T, seed)
    return rae_of(xs, s) + np.array([range_sd, angle_sd, angle_sd]) * rng.standard_normal((B, T, 3))


def _softplus(v):
    return sym.log(1. + sym.exp(v))


def lv_poisson_pdf(y, x):
    return stats.poisson_pmf(y, _softplus(x[0] + x[1] + x[2]))


def lv_poisson_opdf(y, x):
    return float(om.poisson_pmf(y, np.log1p(np.exp(x[0] + x[1] + x[2]))))


def lv_poisson_ys(B, T, seed):
    xs, rng = lv_path(B, T, seed)
    return rng.poisson(np.log1p(np.exp(xs.sum(axis=-1)))).astype(np.float64)


def _bern_poly(x):
    """Degree 2, mixing all three components."""
    return 2. * x[0] * x[1] - x[2] ** 2 + 0.5 * x[1] - 1.


def lv_bernoulli_pdf(y, x):
    return stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-_bern_poly(x))))


def lv_bernoulli_opdf(y, x):
    return float(om.bernoulli_pmf(y, 1. / (1. + np.exp(-_bern_poly(x)))))


def lv_bernoulli_ys(B, T, seed):
    xs, rng = lv_path(B, T, seed)
    p = 1. / (1. + np.exp(-_bern_poly(np.moveaxis(xs, -1, 0))))
    return (rng.random((B, T)) < p).astype(np.float64)


MIX_SD = 0.5


def mixed_pdf(y, x):
    """A single-component factor on x2 reading column 1, times a joint factor reading column 0."""
    return stats.norm_pdf(y[1], x[2], MIX_SD) * stats.norm_pdf(y[0], x[0] * x[1], PROD_SD)


def mixed_opdf(y, x):
    return float(om.norm_pdf(y[1], x[2], MIX_SD) * om.norm_pdf(y[0], x[0] * x[1], PROD_SD))


def mixed_ys(B, T, seed):
    xs, rng = lorenz_path(B, T, seed)
    return np.stack([xs[..., 0] * xs[..., 1] + PROD_SD * rng.standard_normal((B, T)),
                     xs[..., 2] + MIX_SD * rng.standard_normal((B, T))], axis=-1)


# case -> (dynamics of nd3_models.MODELS, device pdf, oracle pdf, data, mean0, cov0, {N: T})
CASES = {
    'product': ('lorenz', product_pdf(), product_opdf(), product_ys, M0, C0, {2: 16, 3: 10, 4: 3}),
    'rae': ('lorenz', rae_pdf(), rae_opdf(), rae_ys, M0, C0, {2: 16, 3: 8, 4: 3}),
    'lv_poisson': ('lv', lv_poisson_pdf, lv_poisson_opdf, lv_poisson_ys, LV_M0, LV_C0, {2: 20, 3: 8, 4: 3}),
    'lv_bernoulli': ('lv', lv_bernoulli_pdf, lv_bernoulli_opdf, lv_bernoulli_ys, LV_M0, LV_C0, {2: 20, 3: 8, 4: 3}),
    'mixed': ('lorenz', mixed_pdf, mixed_opdf, mixed_ys, M0, C0, {2: 16, 3: 10, 4: 3}),
}
NORMAL = {'lorenz': 'euler', 'lv': 'tme_normal_2'}
# (N, family, mode, stable): raw / central / scaled with TME-2 and one Normal closure at N = 2, 3; central and one scaled,
# stable run at N = 4
RUNS = ([(N, 'tme_2', mode, False) for N in (2, 3) for mode in MODES] + [(N, 'normal', 'central', False) for N in (2, 3)]
        + [(4, 'tme_2', 'central', False), (4, 'tme_2', 'scaled', True)])
PARITY = [(case,) + run for case in CASES for run in RUNS]


def setup(case, N, fam):
    model, pdf, opdf, ys_of, mean0, cov0, horizon = CASES[case]
    mi, inds = tables(3, N)
    fns, sig, ofns = family(model, NORMAL[model] if fam == 'normal' else fam, N)
    return pdf, opdf, ys_of, horizon[N], mi, inds, fns, sig, ofns, initial(mi, mean0, cov0)


@pytest.mark.parametrize('case,N,fam,mode,stable', PARITY)
def test_joint_factors_match_the_oracle(case, N, fam, mode, stable):
    pdf, opdf, ys_of, T, mi, inds, fns, sig, ofns, st = setup(case, N, fam)
    ys = ys_of(2, T, 100 + N)
    got = run_device(mode, fns, sig, pdf, ys, mi, inds, st, stable)
    ref = run_oracle(mode, ofns, sig, opdf, ys[0], mi, inds, st, stable, completed=True)
    tag = f'{case} N={N} {fam} {mode} stable={stable}'
    assert first_bad(ref) < 0 and np.isfinite(ref['nell']), f'{tag}: the oracle alone poisons; not a test input'
    assert got['fn'][0] == -1, f'{tag}: the device poisons at step {got["fn"][0]}, the oracle does not'
    upto = compare(got, 0, ref, mi, inds, tag)
    assert upto == T or (stable and upto >= 1), f'{tag}: only {upto} of {T} steps compared'


# ---------------------------------------------------------------------------------------------------------------------
# consistency with the single-component path
# ---------------------------------------------------------------------------------------------------------------------
def _rows(r, idx):
    return {k: v[idx] for k, v in r.items()}


def _joint_of(kind, k):
    """The same law as the single-component factor, with its argument forced through the joint path: the polynomial gets a
    product of two other components with coefficient zero, which makes it trivariate to the tracer."""
    def pdf(y, x):
        zero = 0. * x[(k + 1) % 3] * x[(k + 2) % 3]
        if kind == 'gaussian':
            return stats.norm_pdf(y, 0.8 * x[k] + 0.3 + zero, 0.4)
        if kind == 'bernoulli':
            return stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-(0.5 * x[k] ** 3 - x[k] + 0.2 + zero))))
        return stats.poisson_pmf(y, _softplus(1.5 * x[k] + zero))
    return pdf


def _single_of(kind, k):
    def pdf(y, x):
        if kind == 'gaussian':
            return stats.norm_pdf(y, 0.8 * x[k] + 0.3, 0.4)
        if kind == 'bernoulli':
            return stats.bernoulli_pmf(y, 1. / (1. + sym.exp(-(0.5 * x[k] ** 3 - x[k] + 0.2))))
        return stats.poisson_pmf(y, _softplus(1.5 * x[k]))
    return pdf


def _oracle_of(kind, k):
    def opdf(y, x):
        if kind == 'gaussian':
            return float(om.norm_pdf(y, 0.8 * x[k] + 0.3, 0.4))
        if kind == 'bernoulli':
            return float(om.bernoulli_pmf(y, 1. / (1. + np.exp(-(0.5 * x[k] ** 3 - x[k] + 0.2)))))
        return float(om.poisson_pmf(y, np.log1p(np.exp(1.5 * x[k]))))
    return opdf


def _gap(a, b, mi):
    """Largest relative gap between two single-replicate runs over NLL, means, scales and moments (moments as `moment_err`)."""
    g = float(abs(a['nell'] - b['nell']) / abs(b['nell']))
    g = max(g, float(np.nanmax(moment_err(a['m'], b['m'], mi))))
    for k in ('mean', 'scale'):
        if k in a and k in b:
            g = max(g, float(np.max(np.abs(a[k] - b[k]) / np.maximum(np.abs(b[k]), 1e-300))))
    return g


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('kind,k', [('gaussian', 0), ('bernoulli', 1), ('poisson', 2)])
def test_joint_poly_of_one_component_agrees_with_the_single_component_factor(kind, k, mode):
    """A joint POLY factor whose polynomial reads one component only against today's single-component factor of the same
    law.  Both sum the same node values with the factor multiplied in at a different place, so no bound is fixed: each run
    meets the oracle bar on its own (`compare`), and the gap between the two device runs does not exceed the larger of
    their gaps to the oracle.  Measured on MI355X (N = 3, T = 8, Lotka--Volterra TME-2, the nine cases): the gap between the two
    device runs is exactly 0 in every case -- the joint path multiplies 1 * 1 * 1 by the factor where the table path multiplies
    the factor by 1 * 1, and both evaluate the argument by the same fused Horner steps -- while each run is 2e-13 .. 9e-12 from
    the oracle (the test prints the three figures of each case)."""
    N, T = 3, 8
    mi, inds = tables(3, N)
    fns, sig, ofns = family('lv', 'tme_2', N)
    st = initial(mi, LV_M0, LV_C0)
    xs, rng = lv_path(2, T, 7 + k)
    if kind == 'gaussian':
        ys = 0.8 * xs[..., k] + 0.3 + 0.4 * rng.standard_normal((2, T))
    elif kind == 'bernoulli':
        ys = (rng.random((2, T)) < 1. / (1. + np.exp(-(0.5 * xs[..., k] ** 3 - xs[..., k] + 0.2)))).astype(np.float64)
    else:
        ys = rng.poisson(np.log1p(np.exp(1.5 * xs[..., k]))).astype(np.float64)
    traced = filtering._trace_likelihood(_joint_of(kind, k), 3)
    assert isinstance(traced[0], sym.JointLikelihoodSpec) and traced[0].link == 'poly'
    assert not isinstance(filtering._trace_likelihood(_single_of(kind, k), 3)[0], sym.JointLikelihoodSpec)
    joint = run_device(mode, fns, sig, _joint_of(kind, k), ys, mi, inds, st)
    single = run_device(mode, fns, sig, _single_of(kind, k), ys, mi, inds, st)
    ref = run_oracle(mode, ofns, sig, _oracle_of(kind, k), ys[0], mi, inds, st, completed=True)
    assert first_bad(ref) < 0
    assert compare(joint, 0, ref, mi, inds, 'joint') == T and compare(single, 0, ref, mi, inds, 'single') == T
    j0, s0 = _rows(joint, 0), _rows(single, 0)
    g_js, g_jo, g_so = _gap(j0, s0, mi), _gap(j0, ref, mi), _gap(s0, ref, mi)
    print(f'consistency {kind} x[{k}] {mode}: joint-single {g_js:.3e}, joint-oracle {g_jo:.3e}, single-oracle {g_so:.3e}')
    assert g_js <= max(g_jo, g_so)


# ---------------------------------------------------------------------------------------------------------------------
# batch properties, bit-exact
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_batch_position_and_poisoned_neighbours_do_not_change_a_replicate(mode):
    N, T, B = 2, 12, 4
    mi, inds = tables(3, N)
    fns, sig, _ = family('lorenz', 'tme_2', N)
    st = initial(mi, M0, C0)
    ys = rae_ys(B, T, 5)
    clean = run_device(mode, fns, sig, rae_pdf(), ys, mi, inds, st)
    assert np.all(clean['fn'] == -1) and len(set(clean['nell'].tolist())) == B
    perm = np.array([2, 0, 3, 1])
    moved = run_device(mode, fns, sig, rae_pdf(), ys[perm], mi, inds, st)
    same_bits(moved, _rows(clean, perm))
    # a NaN measurement in a joint factor's column (the elevation) poisons that replicate from that step, and no other
    t_nan = 5
    bad = ys.copy()
    bad[1, t_nan, 2] = np.nan
    got = run_device(mode, fns, sig, rae_pdf(), bad, mi, inds, st)
    assert list(got['fn']) == [-1, t_nan, -1, -1] and np.isnan(got['nell'][1])
    for k in ('m', 'mean', 'scale'):
        if k in got:
            assert np.all(np.isnan(got[k][1, t_nan:])), k
            npt.assert_array_equal(got[k][1, :t_nan], clean[k][1, :t_nan], err_msg=k)
    same_bits(_rows(got, [0, 2, 3]), _rows(clean, [0, 2, 3]))


@pytest.mark.parametrize('mode', MODES)
def test_per_replicate_sensors_and_noise_equal_separate_runs(mode):
    """mfs_joint_nd3.batched: sensor positions (coefficient blocks) and noise levels (par) per replicate, stacked with
    stats.batch_likelihoods, together with a per-replicate single-component factor."""
    N, T, B = 2, 10, 3
    mi, inds = tables(3, N)
    fns, sig, _ = family('lorenz', 'tme_2', N)
    st = initial(mi, M0, C0)
    sensors = np.array([[-5., -5., -2.], [-4., -6., -3.], [6., -5., -1.5]])
    rsd, asd = np.array([0.5, 0.8, 0.3]), np.array([0.1, 0.15, 0.2])
    ys = np.stack([rae_ys(1, T, 40 + b, sensors[b], rsd[b], asd[b])[0] for b in range(B)])

    def member(b):
        return rae_pdf(sensors[b], float(rsd[b]), float(asd[b]))
    batched = stats.batch_likelihoods([member(b) for b in range(B)])
    joint, _ = filtering._joint_struct3(filtering._trace_likelihood(batched, 3), B)
    assert joint.batched == 1 and joint.n_joint == 3
    got = run_device(mode, fns, sig, batched, ys, mi, inds, st)
    assert np.all(got['fn'] == -1) and len(set(got['nell'].tolist())) == B
    for b in range(B):
        one = run_device(mode, fns, sig, member(b), ys[b:b + 1], mi, inds, st)
        same_bits(_rows(got, slice(b, b + 1)), one)
    # a mixed model: per-replicate single-component parameters and joint parameters in one batch
    mix = stats.batch_likelihoods([lambda y, x, b=b: stats.norm_pdf(y[1], x[2], 0.4 + 0.1 * b)
                                   * stats.norm_pdf(y[0], x[0] * x[1] + 0.1 * b, 0.5 + 0.2 * b) for b in range(B)])
    ysm = mixed_ys(B, T, 8)
    gm = run_device(mode, fns, sig, mix, ysm, mi, inds, st)
    assert np.all(gm['fn'] == -1)
    for b in range(B):
        one = run_device(mode, fns, sig, lambda y, x, b=b: stats.norm_pdf(y[1], x[2], 0.4 + 0.1 * b)
                     * stats.norm_pdf(y[0], x[0] * x[1] + 0.1 * b, 0.5 + 0.2 * b), ysm[b:b + 1], mi, inds, st)
        same_bits(_rows(gm, slice(b, b + 1)), one)


@pytest.mark.parametrize('mode', MODES)
def test_empty_batch_and_zero_steps(mode):
    N = 2
    mi, inds = tables(3, N)
    z = mi.shape[0]
    fns, sig, _ = family('lorenz', 'tme_2', N)
    st = initial(mi, M0, C0)
    ys = rae_ys(3, 5, 1)
    r = run_device(mode, fns, sig, rae_pdf(), ys[:0], mi, inds, st)
    assert r['m'].shape == (0, 5, z) and r['nell'].shape == (0,) and r['fn'].shape == (0,)
    r = run_device(mode, fns, sig, rae_pdf(), ys[:, :0], mi, inds, st)
    assert r['m'].shape == (3, 0, z)
    npt.assert_array_equal(r['nell'], np.zeros(3))
    npt.assert_array_equal(r['fn'], -np.ones(3))


def test_plan_is_bit_identical_to_the_host_entry_point():
    N, T, B = 3, 6, 3
    mi, inds = tables(3, N)
    fns, sig, _ = family('lorenz', 'tme_2', N)
    st = initial(mi, M0, C0)
    ys = np.ascontiguousarray(rae_ys(B, T, 11))
    host = run_device('central', fns, sig, rae_pdf(), ys, mi, inds, st)
    factors = filtering._trace_likelihood(rae_pdf(), 3)
    model, keep = filtering._model_struct3(fns[1].tables, [], B, ny=3)
    joint, keep_joint = filtering._joint_struct3(factors, B)
    geo, (out,) = run_plan_nd(model, N, T, B, mi, inds, joint=joint, m0=st['cms'], mean0=st['mean'], ys=ys,
                              outputs=(('moments', 'means', 'nell'),))
    assert geo.threads_per_filter == 256 and geo.grid == B and 0 < geo.lds_bytes <= 160 * 1024
    npt.assert_array_equal(out.moments, host['m'])
    npt.assert_array_equal(out.means, host['mean'])
    npt.assert_array_equal(out.nell, host['nell'])
    del keep, keep_joint


def test_negative_sqrt_argument_poisons_only_its_replicate():
    """sqrt of a negative value is NaN at the node and poisons the replicate through p(y), as a non-finite posterior does."""
    N, T, B = 2, 4, 2
    mi, inds = tables(3, N)
    fns, sig, _ = family('lorenz', 'tme_2', N)
    st = initial(mi, M0, C0)
    members = [lambda y, x: stats.norm_pdf(y, sym.sqrt(x[0] * x[0] + x[1] * x[1] + 1.), 0.5),
               lambda y, x: stats.norm_pdf(y, sym.sqrt(x[0] * x[0] + x[1] * x[1] - 100.), 0.5)]
    ys = np.ones((B, T))
    got = run_device('central', fns, sig, stats.batch_likelihoods(members), ys, mi, inds, st)
    assert list(got['fn']) == [-1, 0] and np.isfinite(got['nell'][0]) and np.isnan(got['nell'][1])


def test_tracking_model_factory_runs():
    N = 2
    mi, inds = tables(3, N)
    dt, T, ts, gs, drift, dispersion, emission, pdf, simulate = ss_models.lorenz_tracking(mi)
    _, _, ys = simulate(np.random.default_rng(3))
    fns = moments.sde_cond_moments_tme(drift, dispersion, dt, 2, d=3)
    cmss, means, nell = filtering.moment_filter_nd_cms((fns[1], 'multi-index'), fns[3], pdf, ys[:20], (mi, inds), gs.cms, gs.mean)
    assert cmss.shape == (20, mi.shape[0]) and np.all(np.isfinite(means)) and np.isfinite(nell)
