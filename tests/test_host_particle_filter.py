"""CPU-only checks of the particle filter: the random stream of include/mfs_hip.h as tests/particle_filter_ref.py restates it
(Philox4x32-10 known answers, the uniform lattice), the restatement pinned to the exact Kalman filter, and the Python layer's
argument handling (nothing here calls the device)."""
import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import io
from mfs_amd.classical_filters_smoothers import (bootstrap_filter, gaussian_transition, multinomial, stratified, systematic,
                                                 ParticleFilterResult)
from mfs_amd.one_dim import ss_models
from mfs_amd.sym import NotDeviceDescribable
from mfs_amd.utils import GaussianSum1D
from tests import brute_force_ref as R
from tests import particle_filter_ref as P


# ---- the stream
@pytest.mark.parametrize('ctr, key, out', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, out):
    assert tuple(int(v) for v in P.philox4x32_10(*ctr, *key)) == out


def test_philox_is_vectorised_over_the_counter():
    i = np.arange(5)
    r = P.philox4x32_10(i, 3, 1, 0, 7, 9)
    for k in range(5):
        assert tuple(int(v[k]) for v in r) == tuple(int(v) for v in P.philox4x32_10(k, 3, 1, 0, 7, 9))


def test_uniform_is_inside_the_unit_interval_and_on_its_lattice():
    edge = np.array([0, 0xffffffff, 63, 64], dtype=np.uint64)
    u_edge = P.uniform(edge[:, None], edge[None, :])
    assert u_edge.min() == 2. ** -53 and u_edge.max() == 1. - 2. ** -53
    u, z = P.draws(12345, np.arange(100000), 7, 1, 0)
    assert np.all((u > 0.) & (u < 1.))
    k = u * 2. ** 52 - 0.5
    assert np.array_equal(k, np.floor(k)) and k.min() >= 0 and k.max() < 2. ** 52
    assert np.all(np.isfinite(z)) and abs(z.mean()) < 0.02 and abs(z.std() - 1.) < 0.02
    assert abs(u.mean() - 0.5) < 0.01


# ---- the restatement against the exact Kalman filter (the reference's own pin, tests/test_classical_filters_smoothers.py:112)
def kalman_case():
    _, _, ys, _ = R.kalman_setting()
    trans = gaussian_transition(R.ou_drift, R.ou_dispersion, R.OU_DT, 'tme-3')
    init = GaussianSum1D.new([0.], [R.OU_SIGMA ** 2], [1.])
    return ys, trans, init


@pytest.mark.parametrize('resampling', ['stratified', 'systematic'])
def test_restatement_matches_kalman(resampling):
    ys, trans, init = kalman_case()
    true_m, _, true_nell = R.kalman(ys)
    _, means, _, _, nell, first_nan, _ = P.particle_filter_ref(lambda b: trans, lambda b: P.gauss_pdf, ys[None, :],
                                                               lambda b: init, [11], 10000, resampling)
    print(f'{resampling}: max |mean err| {np.abs(means[0] - true_m).max():.3e}, |nell err| {abs(nell[0] - true_nell):.3e}')
    npt.assert_allclose(means[0], true_m, atol=2e-1)
    assert abs(nell[0] - true_nell) <= 0.3
    assert first_nan[0] == -1


def test_restatement_nan_rule_and_margin():
    ys, trans, init = kalman_case()
    ys = np.stack([ys[:8], ys[:8]])
    ys[1, 3] = 1e6
    samples, means, variances, cfs, nell, first_nan, margin = P.particle_filter_ref(
        lambda b: trans, lambda b: P.gauss_pdf, ys, lambda b: init, [1, 1], 200, 'stratified', zs=np.linspace(-1., 1., 5))
    assert list(first_nan) == [-1, 3] and np.isnan(nell[1]) and np.isfinite(nell[0])
    assert np.isnan(samples[1, 3:]).all() and np.isnan(cfs[1, 3:]).all() and np.isnan(means[1, 3:]).all()
    assert np.array_equal(samples[0, :3], samples[1, :3])          # same seed, same measurements up to the poisoned step
    assert 0. < margin < 1. / 200
    npt.assert_allclose(cfs[0, :, 2], 1.)                          # z = 0


# ---- the Python layer: argument errors come before the library is touched
def test_argument_errors():
    ys, trans, init = kalman_case()
    ok = (trans, P.gauss_pdf, ys[:5], init, 0, 100)
    with pytest.raises(NotImplementedError, match='multinomial'):
        bootstrap_filter(*ok, multinomial)
    with pytest.raises(NotImplementedError, match='sort'):
        bootstrap_filter(*ok, stratified, True)
    with pytest.raises(ValueError, match='resampling'):
        bootstrap_filter(*ok, lambda w, key: None)
    with pytest.raises(ValueError, match='gaussian_transition'):
        bootstrap_filter(lambda x, key: x, *ok[1:])
    for bad_n in (0, -3, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError, match='nsamples'):
            bootstrap_filter(*ok[:5], bad_n)
    with pytest.raises(ValueError, match='ys'):
        bootstrap_filter(trans, P.gauss_pdf, np.zeros((2, 3, 4)), init, 0, 100)
    with pytest.raises(ValueError, match='init'):
        bootstrap_filter(trans, P.gauss_pdf, ys[:5], np.zeros(99), 0, 100)
    with pytest.raises(ValueError, match='init'):
        bootstrap_filter(trans, P.gauss_pdf, ys[:5], np.zeros((2, 100)), 0, 100)
    with pytest.raises(ValueError, match='key'):
        bootstrap_filter(trans, P.gauss_pdf, np.zeros((3, 5)), init, np.arange(2, dtype=np.uint64), 100)
    with pytest.raises(ValueError, match='key'):
        bootstrap_filter(trans, P.gauss_pdf, ys[:5], init, -1, 100)
    with pytest.raises(ValueError, match='key'):
        bootstrap_filter(trans, P.gauss_pdf, ys[:5], init, np.array([0.5]), 100)
    with pytest.raises(ValueError, match='zs'):
        bootstrap_filter(*ok, zs=np.zeros((2, 2)), return_summaries=True)
    with pytest.raises(ValueError, match='return_summaries'):
        bootstrap_filter(*ok, zs=np.linspace(-1, 1, 4))
    with pytest.raises(ValueError, match='nothing to return'):
        bootstrap_filter(*ok, return_samples=False)
    with pytest.raises(ValueError, match='components'):
        bootstrap_filter(trans, P.gauss_pdf, ys[:5], GaussianSum1D.new(np.zeros(9), np.ones(9), np.full(9, 1 / 9)), 0, 100)
    with pytest.raises(ValueError, match='method'):
        gaussian_transition(R.ou_drift, R.ou_dispersion, 1e-2, 'rk4')
    # per-replicate parameters without a replicate axis, or with the wrong batch
    _, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.well_poisson(3.)
    batched = gaussian_transition(lambda x: drift(x, np.array([1., 2.])), dispersion, 1e-2, 'euler')
    with pytest.raises(ValueError, match='per-replicate'):
        bootstrap_filter(batched, lambda y, x: pmf(y, x, 1.), np.zeros(5), ic, 0, 100)
    with pytest.raises(ValueError, match='batch'):
        bootstrap_filter(batched, lambda y, x: pmf(y, x, 1.), np.zeros((3, 5)), ic, 0, 100)
    with pytest.raises(NotDeviceDescribable):
        bootstrap_filter(trans, lambda y, x: 1., ys[:5], init, 0, 100)
    assert stratified.code == 0 and systematic.code == 1 and ParticleFilterResult._fields[3] == 'cfs'


def test_gaussian_transition_tables():
    dt, _, _, _, drift, dispersion, _, _, _ = ss_models.benes_bernoulli()
    t = gaussian_transition(drift, dispersion, dt, 'tme-3').tables
    assert t.kind == 'gaussian' and t.umap == 'tanh' and t.mean_x_coef == 1.
    e = gaussian_transition(R.ou_drift, R.ou_dispersion, 1e-2, 'euler').tables
    x = np.linspace(-1., 1., 5)
    npt.assert_allclose(e.cond_mean(x), x - 1e-2 * x / R.OU_ELL, rtol=1e-15)
    npt.assert_allclose(e.cond_var(x), 2 * R.OU_SIGMA ** 2 / R.OU_ELL * 1e-2 * np.ones(5), rtol=1e-15)


def test_pf_result_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    means = rng.standard_normal(7)
    cfs = rng.standard_normal((7, 5)) + 1j * rng.standard_normal((7, 5))
    f = str(tmp_path / 'b_2_m_5_mc_0.npz')
    io.save_pf_result(f, means, cfs)
    assert sorted(np.load(f).files) == ['pf_filtering_cfs', 'pf_filtering_means']
    m2, c2 = io.load_pf_result(f)
    assert np.array_equal(m2, means) and np.array_equal(c2, cfs) and c2.dtype == np.complex128
