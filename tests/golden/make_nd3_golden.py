"""Freeze the oracle's d = 3 filters over long horizons as tests/golden/filter_nd3.npz.

The NumPy oracle (oracle/multi_dims.py with the SymPy TME tables of oracle/tme_sympy.py) takes ~0.15 s per step at N = 3 and
~1.2 s at N = 4, too slow to run inside a GPU test at these horizons.  Models: Lorenz-63 in units of 10 with a Gaussian factor
on x_0 and the 3-species Lotka--Volterra model with dispersion diag(sigma_k x_k), a Gaussian factor on x_0 and a
Poisson-softplus factor on x_2, both of tests/nd3_models.py; their parameters are stored next to the outputs and checked by
the test.  Operator TME-2 tables; one seeded replicate of each; N = 3 at T = 200 and N = 4 at T = 50 (the
first 50 measurements); central and scaled modes.  Run from the repository root:

    python tests/golden/make_nd3_golden.py [--procs P] [--out PATH]
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

from oracle import multi_dims as omd, tme_sympy  # noqa: E402
from tests.nd3_models import DT as LORENZ_DT, M0 as LORENZ_M0, C0 as LORENZ_C0, SD as LORENZ_SD  # noqa: E402
from tests.nd3_models import LV_A, LV_C0, LV_DT, LV_M0, LV_SD, LV_SIG, MODELS, lorenz_drift  # noqa: E402

T_LONG = 200
N_T = ((3, 200), (4, 50))
MODES = ('central', 'scaled')


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


FROZEN = ('lorenz', 'lv')     # of tests/nd3_models.MODELS
_G = {}   # SymPy closures shared with forked workers (lambdified functions do not pickle)


def _one(job):
    model, N, mode = job
    m0, c0, opdf = MODELS[model].mean0, MODELS[model].cov0, MODELS[model].opdf
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
    ap.add_argument('--out', default=os.path.join(HERE, 'filter_nd3.npz'), help='where to write the record')
    a = ap.parse_args()
    t0 = time.time()
    _G['ys'] = {'lorenz': lorenz_ys(T_LONG, seed=1), 'lv': lv_ys(T_LONG, seed=2)}
    mi_max = omd.generate_graded_lexico_multi_indices(3, 2 * max(N for N, _ in N_T) - 1)
    for model in FROZEN:   # one table for both N: the closures look multi-indices up
        m = MODELS[model]
        _, ocms, omean, omean_var = tme_sympy.sde_cond_moments_tme_nd(m.drift, m.disp, 3, m.dt, 2, mi_max)
        _G[model] = (ocms, omean, omean_var)
    print(f'tables in {time.time() - t0:.0f} s', flush=True)
    jobs = [(model, N, mode) for model in FROZEN for N, _ in N_T for mode in MODES]
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
    np.savez_compressed(a.out, **out)
    print(f'{os.path.basename(a.out)}: {os.path.getsize(a.out) / 1024:.0f} KiB in {time.time() - t0:.0f} s', flush=True)


if __name__ == '__main__':
    main()
