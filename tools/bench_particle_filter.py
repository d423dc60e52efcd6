#!/usr/bin/env python
"""Benchmark of the bootstrap particle filter (mfs_particle_filter_1d).  One JSON line per case.

Shapes: Benes--Bernoulli at the paper's shape (dardel/benes_bernoulli/pf.py: 10 000 particles, proposal tme-3, stratified
resampling, T = 100) for B = 1000 Monte-Carlo keys, without and with the paper's characteristic-function grid (2000 points on
[-2, 2]); and the convergence shape (dardel/convergence/convergence_pf.py: 100 000 particles, a linear-Gaussian model) for
B = 16.  Times are HIP-event times around the whole host-pointer call (uploads, the initial draw, 5 T launches, downloads of
the summaries; the (B, T, n) samples are not requested); one warm-up call, then `--repeats` timed ones.  The split by kernel
comes from one further call with MFS_PF_SPLIT=1 (an event after every launch, a wait per step; include/mfs_hip.h).  The time of
the NumPy restatement of the tests for ONE replicate is printed beside the first shape as context, not as a target.
`bench.py` stays the project's flagship measurement; this tool is for DESIGN.md section 6.

    python tools/bench_particle_filter.py [--repeats 3] [--quick]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mfs_amd import _lib, stats, synth                                                     # noqa: E402
from mfs_amd.classical_filters_smoothers import gaussian_transition                        # noqa: E402
from mfs_amd.one_dim import ss_models                                                      # noqa: E402
from mfs_amd.one_dim.filtering import _trace_likelihood, build_model_struct                # noqa: E402
from mfs_amd.utils import GaussianSum1D                                                    # noqa: E402
from tools.bench_brute_force import Timer                                                  # noqa: E402

SPLIT = ('propagate_scan', 'offsets', 'resample', 'cf_variance', 'finalize')


def benes_bernoulli(B, T):
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=0)
    return gaussian_transition(drift, dispersion, dt, 'tme-3'), pmf, ic, np.ascontiguousarray(ys, dtype=np.float64)


def linear_gaussian(B, T):
    ell, sigma, dt, r = 1., 0.5, 1e-2, 0.1
    rng = np.random.default_rng(0)
    F, Q = math.exp(-dt / ell), sigma ** 2 * (1 - math.exp(-2 * dt / ell))
    x, ys = sigma * rng.standard_normal(B), np.empty((B, T))
    for t in range(T):
        x = F * x + math.sqrt(Q) * rng.standard_normal(B)
        ys[:, t] = x + math.sqrt(r) * rng.standard_normal(B)
    trans = gaussian_transition(lambda v: -1 / ell * v, lambda _: math.sqrt(2) * sigma / math.sqrt(ell), dt, 'tme-3')
    return trans, (lambda y, v: stats.norm_pdf(y, v, math.sqrt(r))), GaussianSum1D.new([0.], [sigma ** 2], [1.]), ys


def bench(timer, case, setting, n, T, B, nz, repeats, cpu_context=False):
    L = _lib.lib()
    trans, pdf, ic, ys = setting(B, T)
    model, keep = build_model_struct(trans.tables, _trace_likelihood(pdf), B)
    seeds = np.arange(1, B + 1, dtype=np.uint64)
    cumw, mmean, mvar = (np.ascontiguousarray(v, dtype=np.float64) for v in (np.cumsum(ic.weights), ic.means, ic.variances))
    zs = np.linspace(-2., 2., nz) if nz else None
    means, variances, nell, fn = np.empty((B, T)), np.empty((B, T)), np.empty(B), np.empty(B, dtype=np.int32)
    cfs = _lib.pinned_empty((B, T, nz), dtype=np.complex128) if nz else None

    def run(stream):
        _lib.check(L.mfs_particle_filter_1d(C.byref(model), n, T, B, _lib.RESAMPLE['stratified'], _lib.ptr(seeds),
                                            cumw.shape[0], _lib.ptr(cumw), _lib.ptr(mmean), _lib.ptr(mvar), None, 0,
                                            _lib.ptr(ys), nz, _lib.ptr(zs), None, _lib.ptr(means), _lib.ptr(variances),
                                            _lib.ptr(cfs), _lib.ptr(nell), _lib.ptr(fn), 0, stream))

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
    row = dict(case=case, n=n, T=T, B=B, nz=nz, resampling='stratified', ms_median=med, ms_all=[round(v, 3) for v in ms],
               particle_steps_per_s=float(B) * n * T / (med * 1e-3), split_ms=dict(zip(SPLIT, (round(v, 3) for v in split))),
               split_call_ms=round(split_total, 3), nell_first=float(nell[0]), any_nan=bool((fn >= 0).any()),
               samples_returned=False, cfs_bytes=int(cfs.nbytes) if nz else 0)
    if cpu_context:
        from tests import particle_filter_ref as P
        t0 = time.perf_counter()
        ref = P.particle_filter_ref(lambda b: trans, lambda b: pdf, ys[:1], lambda b: ic, seeds[:1], n, 'stratified')
        row['numpy_restatement_one_replicate_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        row['nell_first_numpy'] = float(ref[4][0])
    del keep
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='small shapes: checks the tool, not the device')
    a = ap.parse_args()
    n, T, B, nz, n_conv, B_conv = (1500, 5, 8, 300, 5000, 2) if a.quick else (10000, 100, 1000, 2000, 100000, 16)
    timer = Timer()
    print(json.dumps(dict(case='device', name=_lib.device_name(0))), flush=True)
    print(json.dumps(bench(timer, 'benes_bernoulli_pf', benes_bernoulli, n, T, B, 0, a.repeats, cpu_context=True)), flush=True)
    print(json.dumps(bench(timer, 'benes_bernoulli_pf_cf', benes_bernoulli, n, T, B, nz, a.repeats)), flush=True)
    print(json.dumps(bench(timer, 'linear_gaussian_pf_convergence', linear_gaussian, n_conv, T, B_conv, 0, a.repeats)), flush=True)


if __name__ == '__main__':
    main()
