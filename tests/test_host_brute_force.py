"""CPU-only checks of the brute-force grid filter: the NumPy restatement (tests/brute_force_ref.py) reproduces the reference's
analytic pins against the exact Kalman filter; the host side evaluates the transition mean and standard deviation on the grid
as the closed forms say; argument errors raise; and the C symbol is exported with the header's signature."""
import ctypes as C
import math
import os
import re

import numpy as np
import numpy.testing as npt
import pytest

from mfs_amd import _lib, stats
from mfs_amd.classical_filters_smoothers.brute_force import brute_force_filter, transition_on_grid, GridFilterResult
from mfs_amd.one_dim import ss_models
from tests import brute_force_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gauss_pdf(y, x):
    return stats.norm_pdf(y, x, math.sqrt(R.OU_R))


@pytest.mark.parametrize('method, atol, rtol', [('chapman-euler', 1e-4, 1e-2), ('chapman-tme-2', 1e-7, 1e-6),
                                                ('chapman-tme-3', 1e-11, 1e-10)])
def test_restatement_against_kalman_filter(method, atol, rtol):
    """The reference's TestBruteForce.test_chapman (tests/test_classical_filters_smoothers.py:204-225) at its own tolerances."""
    xs, init_ps, ys, S = R.kalman_setting()
    pdfs, means, variances, nell, first_nan = R.brute_force_ref(R.ou_drift, R.ou_dispersion, lambda b: _gauss_pdf, init_ps, xs,
                                                                ys[None, :], R.OU_DT, S, method)
    true_m, true_v, true_nell = R.kalman(ys)
    est_m = R.trapz(pdfs[0] * xs[None, :], xs, axis=1)
    est_2nd = R.trapz(pdfs[0] * xs[None, :] ** 2, xs, axis=1)
    print(f'{method}: max |mean err| {np.abs(est_m - true_m).max():.3e}, max rel 2nd-moment err '
          f'{np.abs(est_2nd / (true_v + true_m ** 2) - 1).max():.3e}, |nell err| {abs(nell[0] - true_nell):.3e}')
    npt.assert_allclose(est_m, true_m, atol=atol, rtol=rtol)
    npt.assert_allclose(est_2nd, true_v + true_m ** 2, atol=atol, rtol=rtol)
    assert first_nan[0] == -1
    # the restatement's own summaries are these integrals
    npt.assert_allclose(means[0], est_m, rtol=1e-12, atol=1e-15)
    npt.assert_allclose(variances[0] + means[0] ** 2, est_2nd, rtol=1e-12)


def test_ou_transition_on_grid_is_the_truncated_exponential():
    xs = np.linspace(-5., 5., 101)
    S = 20
    ddt = R.OU_DT / S
    mean, sd = transition_on_grid(R.ou_drift, R.ou_dispersion, xs, R.OU_DT, S, 'chapman-tme-3')
    q2 = 2 * R.OU_SIGMA ** 2 / R.OU_ELL
    npt.assert_allclose(mean, xs * sum((-ddt / R.OU_ELL) ** r / math.factorial(r) for r in range(4)), rtol=1e-15, atol=1e-300)
    var = q2 * sum(ddt ** r * (-2 / R.OU_ELL) ** (r - 1) / math.factorial(r) for r in range(1, 4))
    npt.assert_allclose(sd ** 2, np.full_like(xs, var), rtol=1e-15)
    mean_e, sd_e = transition_on_grid(R.ou_drift, R.ou_dispersion, xs, R.OU_DT, S, 'chapman-euler')
    npt.assert_allclose(mean_e, xs * (1 - ddt / R.OU_ELL), rtol=1e-15, atol=1e-300)
    npt.assert_allclose(sd_e ** 2, np.full_like(xs, q2 * ddt), rtol=1e-15)


@pytest.mark.parametrize('method', ['chapman-tme-2', 'chapman-tme-3'])
def test_benes_transition_on_grid(method):
    """for the Benes drift the TME mean and variance stop at order 2."""
    dt, _, _, _, drift, dispersion, _, _, _ = ss_models.benes_bernoulli()
    xs = np.linspace(-4., 4., 200)
    ddt = dt / 4
    mean, sd = transition_on_grid(drift, dispersion, xs, dt, 4, method)
    npt.assert_allclose(mean, xs + np.tanh(xs) * ddt, rtol=1e-15, atol=1e-18)
    npt.assert_allclose(sd ** 2, ddt + (1 - np.tanh(xs) ** 2) * ddt ** 2, rtol=1e-15)


def test_argument_errors_raise_without_a_gpu():
    xs = np.linspace(-3., 3., 31)
    p0 = np.exp(-xs ** 2)
    ys = np.zeros(4)
    with pytest.raises(NotImplementedError, match='kolmogorov'):
        brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, p0, xs, ys, 1e-2, 2, 'kolmogorov')
    with pytest.raises(NotImplementedError):
        brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, p0, xs, ys, 1e-2, 2, 'chapman-rk4')
    _, _, _, _, drift, dispersion, _, pmf, _ = ss_models.well_poisson(3.)
    with pytest.raises(ValueError, match='per-replicate drift'):
        brute_force_filter(lambda x: drift(x, np.array([1., 2.])), dispersion, lambda y, x: pmf(y, x, 1.), p0, xs,
                           np.zeros((2, 4)), 1e-2, 2, 'chapman-euler')
    for bad in (xs[::-1], np.concatenate([xs[:5], xs[4:]])):
        with pytest.raises(ValueError, match='strictly increasing'):
            brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, np.ones(bad.shape), bad, ys, 1e-2)
    with pytest.raises(ValueError, match='init_ps'):      # 3 initial densities, 2 measurement rows
        brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, np.ones((3, 31)), xs, np.zeros((2, 4)), 1e-2)
    with pytest.raises(ValueError, match='init_ps'):      # batched initial densities, ys without a replicate axis
        brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, np.ones((3, 31)), xs, ys, 1e-2)
    with pytest.raises(ValueError, match='likelihood parameters'):
        brute_force_filter(R.ou_drift, R.ou_dispersion, lambda y, x: stats.norm_pdf(y, x, np.array([.1, .2, .3])), p0, xs,
                           np.zeros((2, 4)), 1e-2)
    with pytest.raises(ValueError, match='route'):
        brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, p0, xs, ys, 1e-2, route='fast')
    with pytest.raises(ValueError, match='nothing to return'):
        brute_force_filter(R.ou_drift, R.ou_dispersion, _gauss_pdf, p0, xs, ys, 1e-2, return_pdfs=False)
    assert GridFilterResult._fields == ('pdfs', 'means', 'variances', 'nell', 'first_nan')


def test_symbol_is_exported_with_the_header_signature():
    L = _lib.lib()
    assert hasattr(L, 'mfs_grid_filter_1d') and hasattr(L, 'mfs_grid_gemm_dev')
    text = open(os.path.join(ROOT, 'include', 'mfs_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    decl = re.search(r'int\s+mfs_grid_filter_1d\s*\((.*?)\)\s*;', text, flags=re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    want = []
    for p in params:
        if '*' in p:
            want.append(C.c_void_p)
        else:
            assert p.startswith('int '), p
            want.append(C.c_int)
    assert len(params) == 22
    sig = dict((s[0], s) for s in _lib._SIGNATURES)['mfs_grid_filter_1d']
    assert sig[1] is C.c_int and list(sig[2]) == want
    assert list(L.mfs_grid_filter_1d.argtypes) == want
    defs = dict(re.findall(r'^#define\s+(MFS_[A-Z0-9_]+)\s+(\d+)\b', text, flags=re.M))
    assert int(defs['MFS_GRID_MAX_N']) == _lib.GRID_MAX_N == 8192 and int(defs['MFS_ABI_VERSION']) == 2
