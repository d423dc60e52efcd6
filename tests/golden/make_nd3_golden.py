"""Freeze the oracle's d = 3 filters over long horizons as tests/golden/filter_nd3.npz.

The NumPy oracle (oracle/multi_dims.py with the SymPy TME tables of oracle/tme_sympy.py) takes ~0.15 s per step at N = 3 and
~1.2 s at N = 4, too slow to run inside a GPU test at these horizons.  Models: Lorenz-63 in units of 10 with a Gaussian factor
on x_0 (tests/test_gpu_nd3.py) and the 3-species Lotka--Volterra model with dispersion diag(sigma_k x_k), a Gaussian factor on
x_0 and a Poisson-softplus factor on x_2 (tests/test_gpu_nd3_envelope.py); their parameters are stored next to the outputs
and checked by the test.  Operator TME-2 tables; one seeded replicate of each; N = 3 at T = 200 and N = 4 at T = 50 (the
first 50 measurements); central and scaled modes.  Run from the repository root:

    python tests/golden/make_nd3_golden.py [--procs P]
"""
import argparse
import math
import multiprocessing as mp
import os
import sys
import time

for _v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):   # forked workers + threaded BLAS deadlock
    os.environ.setdefault(_v, '1')

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import models as om, multi_dims as omd, tme_sympy  # noqa: E402

T_LONG = 200
N_T = ((3, 200), (4, 50))
MODES = ('central', 'scaled')

# Lorenz-63 in units of 10 (x = X / 10), dispersion 0.1 I, y = x_0 + N(0, 0.5^2)
LORENZ_DT, LORENZ_SD = 0.01, 0.5
LORENZ_M0, LORENZ_C0 = np.array([0.1, 0.1, 2.4]), np.diag([0.01, 0.01, 0.01])
# Lotka--Volterra: dx_i = x_i (r_i - sum_j A_ij x_j) dt + sigma_i x_i dW_i with r = A 1
LV_A = np.array([[0.8, 0.3, 0.1], [0.2, 0.6, 0.1], [0.4, 0.2, 0.9]])
LV_SIG = np.array([0.1, 0.15, 0.2])
LV_DT, LV_SD = 0.05, 0.2
LV_M0 = np.array([1.0, 0.9, 1.1])
LV_C0 = np.array([[0.02, 0.005, 0.], [0.005, 0.03, -0.004], [0., -0.004, 0.025]])


def lorenz_drift(x):
    return [10. * (x[1] - x[0]), x[0] * (28. - 10. * x[2]) - x[1], 10. * x[0] * x[1] - 8. / 3. * x[2]]


def lorenz_disp(x):
    return [[0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]]


def lv_drift(x):
    r = LV_A.sum(axis=1)
    return [x[i] * (float(r[i]) - sum(float(LV_A[i, j]) * x[j] for j in range(3))) for i in range(3)]


def lv_disp(x):
    return [[float(LV_SIG[i]) * x[i] if i == j else 0. for j in range(3)] for i in range(3)]


def lorenz_opdf(y, x):
    return float(om.norm_pdf(y, x[0], LORENZ_SD))


def lv_opdf(y, x):
    return float(om.norm_pdf(y[0], x[0], LV_SD) * om.poisson_pmf(y[1], np.log1p(np.exp(x[2]))))


def lorenz_ys(T, seed):
    """Euler--Maruyama on 10 sub-steps per dt from a perturbed start; y = x_0 + noise."""
    rng = np.random.default_rng(seed)
    x = LORENZ_M0 + 0.1 * rng.standard_normal(3)
    h = LORENZ_DT / 10
    ys = np.empty(T)
    for t in range(T):
        for _ in range(10):
            a = np.array(lorenz_drift(x))
            x = x + a * h + 0.1 * math.sqrt(h) * rng.standard_normal(3)
        ys[t] = x[0] + LORENZ_SD * rng.standard_normal()
    return ys


def lv_ys(T, seed):
    """Euler--Maruyama on 10 sub-steps per dt; columns x_0 + noise and Poisson(softplus(x_2)) counts."""
    rng = np.random.default_rng(seed)
    r = LV_A.sum(axis=1)
    x = LV_M0 + 0.1 * rng.standard_normal(3)
    h = LV_DT / 10
    ys = np.empty((T, 2))
    for t in range(T):
        for _ in range(10):
            x = np.abs(x + x * (r - LV_A @ x) * h + LV_SIG * x * math.sqrt(h) * rng.standard_normal(3))
        ys[t] = x[0] + LV_SD * rng.standard_normal(), rng.poisson(np.log1p(np.exp(x[2])))
    return ys


MODELS = {'lorenz': (lorenz_drift, lorenz_disp, LORENZ_DT, LORENZ_M0, LORENZ_C0, lorenz_opdf),
          'lv': (lv_drift, lv_disp, LV_DT, LV_M0, LV_C0, lv_opdf)}
_G = {}   # SymPy closures shared with forked workers (lambdified functions do not pickle)


def _one(job):
    model, N, mode = job
    _, _, _, m0, c0, opdf = MODELS[model]
    ocms, omean, omean_var = _G[model]
    T = dict(N_T)[N]
    ys = _G['ys'][model][:T]
    mi = omd.generate_graded_lexico_multi_indices(3, 2 * N - 1)
    inds = omd.gram_and_hankel_indices_graded_lexico(N, 3)
    cms0 = np.array([omd.raw_moments_mvn_kan(np.zeros(3), c0, n) for n in mi])
    if mode == 'central':
        m, means, nell = omd.moment_filter_nd_cms((ocms, 'multi-index'), omean, opdf, ys, (mi, inds), cms0, m0)
        return m, means, None, nell
    scale0 = np.sqrt(np.diag(c0))

    def oscms(x, idx, mean, scale):
        return ocms(x, idx, mean) / np.prod(np.asarray(scale) ** np.asarray(idx), axis=-1)
    m, means, scales, nell = omd.moment_filter_nd_scms((oscms, 'multi-index'), omean_var, opdf, ys, (mi, inds),
                                                       cms0 / np.prod(scale0 ** mi, axis=-1), m0, scale0)
    return m, means, scales, nell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--procs', type=int, default=max(1, min(8, (os.cpu_count() or 2) - 1)))
    a = ap.parse_args()
    t0 = time.time()
    _G['ys'] = {'lorenz': lorenz_ys(T_LONG, seed=1), 'lv': lv_ys(T_LONG, seed=2)}
    mi_max = omd.generate_graded_lexico_multi_indices(3, 2 * max(N for N, _ in N_T) - 1)
    for model, (drift, disp, dt, *_) in MODELS.items():   # one table for both N: the closures look multi-indices up
        _, ocms, omean, omean_var = tme_sympy.sde_cond_moments_tme_nd(drift, disp, 3, dt, 2, mi_max)
        _G[model] = (ocms, omean, omean_var)
    print(f'tables in {time.time() - t0:.0f} s', flush=True)
    jobs = [(model, N, mode) for model in MODELS for N, _ in N_T for mode in MODES]
    if a.procs <= 1:
        res = [_one(j) for j in jobs]
    else:
        with mp.get_context('fork').Pool(a.procs) as pool:
            res = pool.map(_one, jobs, chunksize=1)
    out = {'lorenz_dt': LORENZ_DT, 'lorenz_sd': LORENZ_SD, 'lorenz_m0': LORENZ_M0, 'lorenz_c0': LORENZ_C0,
           'lv_A': LV_A, 'lv_sig': LV_SIG, 'lv_dt': LV_DT, 'lv_sd': LV_SD, 'lv_m0': LV_M0, 'lv_c0': LV_C0,
           'lorenz_ys': _G['ys']['lorenz'], 'lv_ys': _G['ys']['lv']}
    for (model, N, mode), (m, means, scales, nell) in zip(jobs, res):
        key = f'{model}_N{N}_{mode}'
        out[f'{key}_moments'], out[f'{key}_means'], out[f'{key}_nell'] = m, means, np.float64(nell)
        if scales is not None:
            out[f'{key}_scales'] = scales
        bad = ~np.isfinite(m).all(axis=1)
        print(f'{key}: nell {nell:.10f}, first non-finite step {int(np.argmax(bad)) if bad.any() else -1}', flush=True)
    path = os.path.join(HERE, 'filter_nd3.npz')
    np.savez_compressed(path, **out)
    print(f'filter_nd3.npz: {os.path.getsize(path) / 1024:.0f} KiB in {time.time() - t0:.0f} s', flush=True)


if __name__ == '__main__':
    main()
