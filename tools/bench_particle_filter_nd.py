#!/usr/bin/env python
"""Benchmark of the d = 2 bootstrap particle filter (mfs_particle_filter_nd).  One JSON line per case.

Shapes: prey--predator at the driver's shape (dardel/prey_predator/pf.py: 10 000 particles, T = 2000, stratified resampling, the
Gaussian-sum initial law, one Bernoulli factor on the prey) with the Euler proposal and with `tme-2`, for B = 1, 64 and 512
Monte-Carlo keys.  Times are HIP-event times around the whole host-pointer call (uploads, the initial draw, 5 T launches,
downloads of the summaries; the (B, T, n, 2) samples are not requested); one warm-up call, then `--repeats` timed ones.  The
split by kernel comes from one further call with MFS_PF_SPLIT=1 (an event after every launch, a wait per step;
include/mfs_hip.h).  `bench.py` stays the project's flagship measurement; this tool is for DESIGN.md section 6.

    python tools/bench_particle_filter_nd.py [--repeats 3] [--quick] [--batches 1,64,512]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mfs_amd import _lib                                                                   # noqa: E402
from mfs_amd.classical_filters_smoothers import gaussian_transition_nd                     # noqa: E402
from mfs_amd.classical_filters_smoothers.smc import _chol2                                 # noqa: E402
from mfs_amd.multi_dims import ss_models                                                   # noqa: E402
from mfs_amd.multi_dims.filtering import _model_struct, _trace_likelihood                  # noqa: E402
from tools.bench_brute_force import Timer                                                  # noqa: E402

SPLIT = ('propagate_scan', 'offsets', 'resample', 'covariance', 'finalize')
MI = ((0, 0), (0, 1), (1, 0))


def bench(timer, method, n, T, B, repeats):
    L = _lib.lib()
    dt, _, _, gs, drift, dispersion, _, pmf, _ = ss_models.prey_predator(MI)
    trans = gaussian_transition_nd(drift, dispersion, 2, dt, method)
    ys = np.ascontiguousarray((np.random.default_rng(0).random((B, T, 1)) < 0.5), dtype=np.float64)
    model, keep = _model_struct(trans.tables, _trace_likelihood(pmf, 2), B)
    seeds = np.arange(1, B + 1, dtype=np.uint64)
    cumw, mmean, mchol = (np.ascontiguousarray(v, dtype=np.float64) for v in (np.cumsum(gs.weights), gs.means, _chol2(gs.covs)))
    means, covs, nell, fn = np.empty((B, T, 2)), np.empty((B, T, 2, 2)), np.empty(B), np.empty(B, dtype=np.int32)

    def run(stream):
        _lib.check(L.mfs_particle_filter_nd(C.byref(model), n, T, B, _lib.RESAMPLE['stratified'], _lib.ptr(seeds),
                                            cumw.shape[0], _lib.ptr(cumw), _lib.ptr(mmean), _lib.ptr(mchol), None, 0,
                                            _lib.ptr(ys), None, _lib.ptr(means), _lib.ptr(covs), _lib.ptr(nell), _lib.ptr(fn), 0,
                                            stream))

    timer.time_ms(run)                      # warm-up: the pool allocates its blocks
    ms = [timer.time_ms(run) for _ in range(repeats)]
    os.environ['MFS_PF_SPLIT'] = '1'
    try:
        split_total = timer.time_ms(run)
    finally:
        os.environ['MFS_PF_SPLIT'] = '0'
    split = (C.c_double * 5)()
    _lib.check(L.mfs_pf_last_split_ms(split))
    med = float(np.median(ms))
    del keep
    return dict(case=f'prey_predator_pf_{method}', n=n, T=T, B=B, resampling='stratified', ms_median=med,
                ms_all=[round(v, 3) for v in ms], particle_steps_per_s=float(B) * n * T / (med * 1e-3),
                split_ms=dict(zip(SPLIT, (round(v, 3) for v in split))), split_call_ms=round(split_total, 3),
                nell_first=float(nell[0]), any_nan=bool((fn >= 0).any()), samples_returned=False)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='small shapes: checks the tool, not the device')
    ap.add_argument('--batches', default=None, help='comma-separated replicate counts (default 1,64,512; --quick: 1,3)')
    a = ap.parse_args()
    n, T = (1500, 5) if a.quick else (10000, 2000)
    batches = [int(v) for v in a.batches.split(',')] if a.batches else ([1, 3] if a.quick else [1, 64, 512])
    timer = Timer()
    print(json.dumps(dict(case='device', name=_lib.device_name(0))), flush=True)
    for method in ('euler', 'tme-2'):
        for B in batches:
            print(json.dumps(bench(timer, method, n, T, B, a.repeats)), flush=True)


if __name__ == '__main__':
    main()
