#!/usr/bin/env python
"""Benchmark of the Gaussian filters (mfs_gaussian_filter_1d / _nd).  One JSON line per case and method.

Shapes, each as the Gauss--Hermite filter (GH-11) and as the EKF:
  benes_bernoulli   dardel/benes_bernoulli: TME-3, T = 100, B = 1000 Monte-Carlo data sets
  well_poisson_grid dardel/parameter_estimation/ghf_ekf.py as a grid: one data set, (p1, p2) on a 128 x 128 grid = 16 384
                    parameter points as per-replicate tables, TME-2, T = 1000
  prey_predator     dardel/prey_predator/ghf_ekf.py: d = 2, GH-11 = 121 points, Euler--Maruyama, T = 2000, B = 1000
Times are HIP-event times around the whole host-pointer call (uploads, ONE kernel launch that holds the time loop, downloads
of means, covariances and running nells into pinned memory); one warm-up call, then `--repeats` timed ones, the median
reported.  `nll_only_ms` is the same call without the mean / covariance outputs (what a likelihood grid needs).  Kernel times
come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_gaussian_filters.py --repeats 1`.
`--scaling` adds the Benes--Bernoulli GH-11 case over B = 1 .. 131 072: a kernel bound by its chain of T dependent steps
takes the same time until the device is full.  The time of the NumPy restatement of the tests for ONE replicate is printed as
context, not as a target.  `bench.py` stays the project's flagship measurement; this tool is for DESIGN.md section 3.9.

    python tools/bench_gaussian_filters.py [--repeats 5] [--quick] [--scaling]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mfs_amd import _lib, synth                                                                        # noqa: E402
from mfs_amd.classical_filters_smoothers import (SigmaPoints, gaussian_transition, gaussian_transition_nd,   # noqa: E402
                                                 measurement_moments)
from mfs_amd.multi_dims import ss_models as ss_models_nd                                               # noqa: E402
from mfs_amd.multi_dims.filtering import _model_struct                                                 # noqa: E402
from mfs_amd.one_dim import ss_models                                                                  # noqa: E402
from mfs_amd.one_dim.filtering import build_model_struct                                               # noqa: E402
from tools.bench_brute_force import Timer                                                              # noqa: E402

GH_ORDER = 11


def benes_bernoulli(B, T):
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=0)
    return 1, gaussian_transition(drift, dispersion, dt, 'tme-3'), measurement_moments(pmf), ys, [0.], [[0.3]]


def well_poisson_grid(B, T):
    side = int(round(B ** 0.5))
    assert side * side == B, 'the parameter grid is square'
    g1, g2 = np.meshgrid(np.linspace(0.5, 6., side), np.linspace(1., 6., side), indexing='ij')
    p1, p2 = g1.reshape(-1), g2.reshape(-1)
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models.well_poisson(3.)
    ys, _ = synth.well_poisson_batch(1, T, 3., 3., dt, seed=0)
    return 1, gaussian_transition(lambda x: drift(x, p1), dispersion, dt, 'tme-2'), \
        measurement_moments(lambda y, x: pmf(y, x, p2)), np.repeat(ys, B, axis=0), [0.], [[0.3]]


def prey_predator(B, T):
    dt, _, _, _, drift, dispersion, _, pmf, _ = ss_models_nd.prey_predator(np.zeros((1, 2), dtype=int))
    ys, _ = synth.prey_predator_batch(B, T, dt, seed=0)
    return 2, gaussian_transition_nd(drift, dispersion, 2, dt, 'euler'), measurement_moments(pmf), ys, [1., 1.], \
        1.5e-3 * np.eye(2)


def bench(timer, case, setting, method, T, B, repeats, cpu_context=False):
    L = _lib.lib()
    d, trans, meas, ys, m0, v0 = setting(B, T)
    lik = meas.spec(d)
    model, keep = _model_struct(trans.tables, [lik], B) if d == 2 else build_model_struct(trans.tables, lik, B)
    entry = L.mfs_gaussian_filter_nd if d == 2 else L.mfs_gaussian_filter_1d
    sgps = SigmaPoints.gauss_hermite(d, GH_ORDER)
    xi, w = np.ascontiguousarray(sgps.xi), np.ascontiguousarray(sgps.w)
    n_points = sgps.n_points if method == 'ghf' else 0
    ys = np.ascontiguousarray(ys, dtype=np.float64)
    m0, v0 = np.ascontiguousarray(m0, dtype=np.float64), np.ascontiguousarray(v0, dtype=np.float64)
    means, covs, nells = (_lib.pinned_empty(s) for s in ((B, T, d), (B, T, d, d), (B, T)))
    fn = np.empty(B, dtype=np.int32)

    def run(stream, full=True):
        _lib.check(entry(C.byref(model), _lib.GF_METHOD['sigma_point' if method == 'ghf' else 'ekf'], n_points, _lib.ptr(xi),
                         _lib.ptr(w), T, B, _lib.ptr(m0), _lib.ptr(v0), 0, _lib.ptr(ys), _lib.ptr(means) if full else None,
                         _lib.ptr(covs) if full else None, _lib.ptr(nells), _lib.ptr(fn), 0, stream))

    timer.time_ms(run)                      # warm-up: the pool allocates its blocks, the code object loads
    ms = [timer.time_ms(run) for _ in range(repeats)]
    nll_only = [timer.time_ms(lambda s: run(s, full=False)) for _ in range(repeats)]
    med = float(np.median(ms))
    row = dict(case=case, method=method, d=d, n_points=n_points, lanes_per_replicate=1 if method == 'ekf' else min(64, 1 << (n_points - 1).bit_length()),
               T=T, B=B, ms_median=round(med, 3), ms_all=[round(v, 3) for v in ms],
               nll_only_ms=round(float(np.median(nll_only)), 3), filter_steps_per_s=float(B) * T / (med * 1e-3),
               output_bytes=int(means.nbytes + covs.nbytes + nells.nbytes), nell_first=float(nells[0, -1]),
               nan_replicates=int((fn >= 0).sum()))
    if cpu_context:
        from tests import gaussian_filters_ref as G
        tables = trans.tables
        t0 = time.perf_counter()
        ref = G.gaussian_filter_ref(tables, lik, G.SIGMA_POINT if method == 'ghf' else G.EKF, sgps, m0, v0, ys[0])
        row['numpy_restatement_one_replicate_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        row['nell_first_numpy'] = float(ref.nells[-1])
    del keep
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='small shapes: checks the tool, not the device')
    ap.add_argument('--scaling', action='store_true', help='also Benes--Bernoulli GH-11, T = 100, over B = 1 .. 131 072')
    a = ap.parse_args()
    shapes = dict(benes_bernoulli=(benes_bernoulli, 100, 1000), well_poisson_grid=(well_poisson_grid, 1000, 16384),
                  prey_predator=(prey_predator, 2000, 1000))
    if a.quick:
        shapes = dict(benes_bernoulli=(benes_bernoulli, 10, 5), well_poisson_grid=(well_poisson_grid, 10, 9),
                      prey_predator=(prey_predator, 10, 5))
    timer = Timer()
    print(json.dumps(dict(case='device', name=_lib.device_name(0))), flush=True)
    for case, (setting, T, B) in shapes.items():
        for method in ('ghf', 'ekf'):
            # the parameter grid's restatement would need one table per replicate: context for the shared-table cases only
            print(json.dumps(bench(timer, case, setting, method, T, B, a.repeats, cpu_context=case != 'well_poisson_grid')),
                  flush=True)
    if a.scaling:
        for B in ((1, 8) if a.quick else (1, 64, 1024, 4096, 16384, 65536, 131072)):
            print(json.dumps(bench(timer, 'benes_bernoulli_scaling', benes_bernoulli, 'ghf', 100, B, a.repeats)), flush=True)


if __name__ == '__main__':
    main()
