"""The Gaussian-filter envelope cases in 50-digit arithmetic, as a golden fixture.

    python tests/golden/make_gaussian_filters_exact.py [--procs P]      writes tests/golden/gaussian_filters_exact.npz (numbers only)

tests/gaussian_filters_exact.py holds the one list of cases and the arbiters (sigma_point_mp, ekf_mp, adf_closed_form).  For
every case this stores, per replicate: the inputs exactly as the arbiter saw them (coefficient table, likelihood parameters,
rule, initial law, measurements), the arbiter's outputs rounded once to fp64, and the outputs of the fp64 restatement
(tests/gaussian_filters_ref.py) on the same inputs.  mpmath is far too slow to run beside the GPU tests (a 64-point rule of a
d = 2 state costs seconds per replicate), so the tests read this file; tests/test_host_gaussian_filters.py regenerates two cheap
cases and compares them with the stored arrays bit for bit, and re-runs the restatement on every stored case.
"""
import argparse
import multiprocessing as mp_
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

from tests import gaussian_filters_exact as X  # noqa: E402


def _one(i):
    t0 = time.time()
    case = X.cases()[i]
    return case.name, X.freeze(case), time.time() - t0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--procs', type=int, default=max(1, min(16, (os.cpu_count() or 2)) - 1))
    ap.add_argument('--out', type=str, default=X.FIXTURE)
    a = ap.parse_args()
    t0 = time.time()
    cases = X.cases()
    order = sorted(range(len(cases)), key=lambda i: -(cases[i].n_points + 1) * cases[i].ys.size)   # the slow cases first
    arrays = {}
    with mp_.get_context('fork').Pool(a.procs) as pool:
        for name, got, dt in pool.imap_unordered(_one, order, chunksize=1):
            arrays.update(got)
            print(f'{name}: {dt:.1f} s', flush=True)
    path = os.path.join(HERE, a.out)
    np.savez_compressed(path, **{k: arrays[k] for k in sorted(arrays)})
    print(f'{len(cases)} cases, {os.path.getsize(path) / 1024:.0f} KiB in {time.time() - t0:.0f} s')
