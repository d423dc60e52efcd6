"""CPU-only checks of the grid filter's characteristic functions: argument errors of `brute_force_filter(zs=...)` and
`characteristic_from_pdf` raise before anything touches the device; `cf_errors` is the three lines of
dardel/benes_bernoulli/compute_errs.py:103-105; the two writers of mfs_amd.io use the reference's key names; the exactly
summed restatement (tests/grid_cf_ref.py) alone meets the analytic pins the GPU tests apply; and the new C symbols carry the
header's signatures."""
import ctypes as C
import math
import os
import re

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, io, stats
from mfs_amd import one_dim
from mfs_amd.classical_filters_smoothers.brute_force import (brute_force_filter, GridFilterCFResult, GridFilterResult)
from mfs_amd.one_dim.moments import cf_errors, characteristic_from_pdf
from tests import brute_force_ref as R
from tests import grid_cf_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gauss_pdf(y, x):
    return stats.norm_pdf(y, x, math.sqrt(R.OU_R))


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the argument checks come first."""
    def boom():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'lib', boom)


def test_brute_force_filter_zs_argument_errors(no_library):
    xs = np.linspace(-3., 3., 31)
    p0 = np.exp(-xs ** 2)
    ys = np.zeros(4)
    call = lambda zs, **kw: brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, p0, xs, ys, 1e-2, zs=zs, **kw)  # noqa: E731
    for bad in (np.zeros((2, 3)), 1.5, np.zeros(0)):
        with pytest.raises(ValueError, match=r'zs must have shape \(m,\)'):
            call(bad)
    for v in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match='zs must be finite'):
            call(np.array([0., v, 1.]))
    with pytest.raises(ValueError, match='8192'):
        call(np.linspace(-2., 2., _lib.GRID_MAX_NZ + 1))
    with pytest.raises(ValueError, match='zs must be finite'):     # legal together with return_pdfs=False: the error is zs's
        call(np.array([np.nan]), return_pdfs=False)
    with pytest.raises(TypeError):                                 # keyword-only
        brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, p0, xs, ys, 1e-2, 1, 'chapman-tme-2', np.zeros(3))
    assert GridFilterResult._fields == ('pdfs', 'means', 'variances', 'nell', 'first_nan')
    assert GridFilterCFResult._fields == GridFilterResult._fields + ('cfs',)


def test_characteristic_from_pdf_argument_errors(no_library):
    xs = np.linspace(-1., 1., 9)
    ps = np.ones(9)
    with pytest.raises(ValueError, match='z must be a scalar'):
        characteristic_from_pdf(np.zeros((2, 2)), ps, xs)
    with pytest.raises(ValueError, match='z must be a scalar'):
        characteristic_from_pdf(np.zeros(0), ps, xs)
    with pytest.raises(ValueError, match='z must be finite'):
        characteristic_from_pdf(np.array([0., np.nan]), ps, xs)
    with pytest.raises(ValueError, match='8192'):
        characteristic_from_pdf(np.zeros(_lib.GRID_MAX_NZ + 1), ps, xs)
    with pytest.raises(ValueError, match='xs must have shape'):
        characteristic_from_pdf(0.5, ps, xs.reshape(3, 3))
    with pytest.raises(ValueError, match='strictly increasing'):
        characteristic_from_pdf(0.5, ps, xs[::-1])
    with pytest.raises(ValueError, match='ps must have shape'):
        characteristic_from_pdf(0.5, np.ones((2, 8)), xs)
    with pytest.raises(ValueError, match='ps must have shape'):
        characteristic_from_pdf(0.5, np.float64(1.), xs)
    with pytest.raises(ValueError, match='exceed'):
        characteristic_from_pdf(0.5, np.ones(_lib.GRID_MAX_N + 1), np.arange(_lib.GRID_MAX_N + 1.))


def test_cf_errors_is_the_reference_three_lines():
    rng = np.random.default_rng(11)
    zs = np.sort(rng.uniform(-2., 2., 17))
    a = rng.standard_normal((3, 5, 17)) + 1j * rng.standard_normal((3, 5, 17))
    b = rng.standard_normal((3, 5, 17)) + 1j * rng.standard_normal((3, 5, 17))
    l1, l2, sup = cf_errors(a, b, zs)
    npt.assert_array_equal(l1, R.trapz(np.abs(a - b), zs, axis=-1))
    npt.assert_array_equal(l2, np.sqrt(R.trapz(np.abs(a - b) ** 2, zs, axis=-1)))
    npt.assert_array_equal(sup, np.max(np.abs(a - b), axis=-1))
    assert l1.shape == l2.shape == sup.shape == (3, 5)
    l1_row, _, _ = cf_errors(a[1, 2], b[1, 2], zs)
    assert l1_row.shape == () and l1_row == l1[1, 2]
    with pytest.raises(ValueError, match='last axis'):
        cf_errors(a, b, zs[:-1])
    assert one_dim.cf_errors is cf_errors and one_dim.characteristic_from_pdf is characteristic_from_pdf


def test_io_round_trips_use_the_reference_keys(tmp_path):
    rng = np.random.default_rng(12)
    trajs, means = rng.standard_normal((4, 6)), rng.standard_normal((4, 6))
    cfs = rng.standard_normal((4, 6, 5)) + 1j * rng.standard_normal((4, 6, 5))
    f = str(tmp_path / 'b_2_m_5.npz')
    io.save_brute_force_summary(f, trajs, means, cfs)
    assert sorted(np.load(f).files) == ['true_filtering_cfs', 'true_filtering_means', 'true_trajs']   # post_processing_brute_force.py:53-55
    back = io.load_brute_force_summary(f)
    for a, b in zip(back, (trajs, means, cfs)):
        npt.assert_array_equal(a, b)
    assert back[2].dtype == np.complex128

    keys = ['true_trajs_vs_true_means_abs', 'true_trajs_vs_mf_means_abs', 'true_trajs_vs_ghf_means_abs',
            'true_trajs_vs_pf_means_abs', 'true_means_vs_mf_means_abs', 'true_means_vs_ghf_means_abs',
            'true_means_vs_pf_means_abs', 'true_cfs_vs_mf_l1', 'true_cfs_vs_mf_l2', 'true_cfs_vs_mf_sup', 'true_cfs_vs_ghf_l1',
            'true_cfs_vs_ghf_l2', 'true_cfs_vs_ghf_sup', 'true_cfs_vs_pf_l1', 'true_cfs_vs_pf_l2', 'true_cfs_vs_pf_sup']
    assert len(keys) == 16 and list(io.BENES_BERNOULLI_ERR_KEYS) == keys                            # compute_errs.py:115-128
    errs = {k: rng.random((4, 6)) for k in keys}
    g = str(tmp_path / 'errs.npz')
    io.save_benes_bernoulli_errs(g, **errs)
    data = np.load(g)
    assert sorted(data.files) == sorted(keys)
    for k in keys:
        npt.assert_array_equal(data[k], errs[k])
    with pytest.raises(ValueError, match='missing'):
        io.save_benes_bernoulli_errs(g, **{k: errs[k] for k in keys[:-1]})
    with pytest.raises(ValueError, match='unknown'):
        io.save_benes_bernoulli_errs(g, other=1., **errs)


# ---- the reference of the GPU tests' analytic pins, on its own
def test_restatement_meets_the_normal_pin():
    """Trapezoid aliasing exp(-2 pi^2 sigma^2 / h^2) with h = sigma / 16 and tails of e^-32: far below 1e-12."""
    mu, sigma, xs, ps, zs = G.normal_pin_case()
    assert np.abs(zs * sigma).max() <= 4.
    ref = G.cf_ref(ps, xs, zs)
    exact = np.exp(1j * zs * mu - 0.5 * zs ** 2 * sigma ** 2)
    print(f'restatement against exp(i z mu - z^2 sigma^2 / 2): max |err| {np.abs(ref - exact).max():.3e}')
    npt.assert_allclose(ref, exact, rtol=0, atol=1e-12)


def test_restatements_meet_the_kalman_pin_within_half_its_tolerance():
    """Filter restatement + cf restatement against exp(i z m_t - z^2 v_t / 2) on the grid of the device pin, linspace(-5, 5,
    1000): the case is kept on the device only because the reference alone stays within half the tolerance."""
    xs, init_ps, ys, S = R.kalman_setting()
    pdfs = R.brute_force_ref(R.ou_drift, R.ou_dispersion, lambda b: _gauss_pdf, init_ps, xs, ys[None, :], R.OU_DT, S,
                             'chapman-tme-3')[0][0]
    true_m, true_v, _ = R.kalman(ys)
    ref = G.cf_ref(pdfs, xs, G.KALMAN_ZS)
    exact = np.exp(1j * G.KALMAN_ZS[None, :] * true_m[:, None] - 0.5 * G.KALMAN_ZS[None, :] ** 2 * true_v[:, None])
    tol = G.kalman_cf_tolerance(G.KALMAN_ZS, true_m, true_v)
    ratio = np.abs(ref - exact) / tol
    print(f'restatements against the Kalman cf: worst |err| / tolerance {ratio.max():.3f}')
    assert ratio.max() <= 0.5


def test_new_symbols_are_exported_with_the_header_signatures():
    L = _lib.lib()
    text = open(os.path.join(ROOT, 'include', 'mfs_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    sigs = dict((s[0], s) for s in _lib._SIGNATURES)
    for name, count in (('mfs_grid_filter_1d_cf', 25), ('mfs_cf_from_pdf_1d', 9)):
        decl = re.search(r'int\s+' + name + r'\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
        params = [' '.join(p.split()) for p in decl.split(',')]
        want = [C.c_void_p if '*' in p else C.c_int for p in params]
        assert all('*' in p or p.startswith('int ') for p in params)
        assert len(params) == count
        assert sigs[name][1] is C.c_int and list(sigs[name][2]) == want
        assert list(getattr(L, name).argtypes) == want
    defs = dict(re.findall(r'^#define\s+(MFS_[A-Z0-9_]+)\s+(\d+)\b', text, flags=re.M))
    assert int(defs['MFS_GRID_MAX_NZ']) == _lib.GRID_MAX_NZ == 8192
