#!/usr/bin/env python
"""Benchmark of the brute-force grid filter (mfs_grid_filter_1d) and of its fp64 matrix-core GEMM.  One JSON line per case.

Workload: Benes--Bernoulli at the paper's shape (dardel/benes_bernoulli/brute_force.py: 2000 grid points, 100 sub-steps per
measurement, chapman-tme-3; T = 100), B in {1, 64, 1000}, both routes.  Times are HIP-event times around the whole host-pointer
call (uploads, K, K^S, the time loop, downloads of the summaries; the (B, T, n) pdfs are not requested).  Then the GEMM alone
at 2048^3 as TFLOP/s and as a fraction of the 78.6 TFLOP/s fp64 matrix peak, and, if librocblas loads in this process,
rocblas_dgemm at the same shape as a yardstick.  `bench.py` stays the project's flagship measurement; this tool is for
DESIGN.md section 6.

With --nz m the call is mfs_grid_filter_1d_cf at zs = linspace(-2, 2, m) (the driver's frequencies at m = 2000): the time
then includes the table, one more product per measurement and the download of the (B, T, m) complex cfs into pinned memory.

    python tools/bench_brute_force.py [--batches 1,64,1000] [--repeats 3] [--quick] [--nz 0] [--routes power,stepwise] [--no-gemm]
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

from mfs_amd import _lib, synth                                                          # noqa: E402
from mfs_amd.classical_filters_smoothers.brute_force import transition_on_grid          # noqa: E402
from mfs_amd.one_dim import ss_models                                                    # noqa: E402

FP64_MATRIX_PEAK_TFLOPS = 78.6
GRID_LO, GRID_HI = -6., 6.


class Timer:
    """HIP events on a stream of the library's."""

    def __init__(self):
        L = _lib.lib()
        self.stream, self.e0, self.e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(L.mfs_stream_create(C.byref(self.stream)))
        _lib.check(L.mfs_event_create(C.byref(self.e0)))
        _lib.check(L.mfs_event_create(C.byref(self.e1)))

    def time_ms(self, fn):
        L = _lib.lib()
        _lib.check(L.mfs_event_record(self.e0, self.stream))
        fn(self.stream)
        _lib.check(L.mfs_event_record(self.e1, self.stream))
        ms = C.c_float()
        _lib.check(L.mfs_event_elapsed_ms(self.e0, self.e1, C.byref(ms)))
        return float(ms.value)


def bench_filter(timer, n, S, T, B, route, repeats, nz=0):
    L = _lib.lib()
    dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli()
    xs = np.linspace(GRID_LO, GRID_HI, n)
    mean, sd = transition_on_grid(drift, dispersion, xs, dt, S, 'chapman-tme-3')
    ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=0)
    ys = np.ascontiguousarray(ys, dtype=np.float64)
    init_ps = np.ascontiguousarray(ic.pdf(xs))
    lik = np.array([0., 0., 0., 0.2])      # logistic(x^3 / 5)
    means, variances, nell, fn = np.empty((B, T)), np.empty((B, T)), np.empty(B), np.empty(B, dtype=np.int32)

    zs = np.linspace(-2., 2., nz) if nz else None
    cfs = _lib.pinned_empty((B, T, nz), dtype=np.complex128) if nz else None

    def run(stream):
        if nz:
            _lib.check(L.mfs_grid_filter_1d_cf(n, T, B, S, int(route == 'power'), _lib.ptr(xs), _lib.ptr(mean), _lib.ptr(sd),
                                               _lib.LIK['bernoulli_logistic'], 4, _lib.ptr(lik), 0, _lib.ptr(init_ps), 0,
                                               _lib.ptr(ys), nz, _lib.ptr(zs), None, _lib.ptr(means), _lib.ptr(variances),
                                               _lib.ptr(cfs), _lib.ptr(nell), _lib.ptr(fn), 0, stream))
            return
        _lib.check(L.mfs_grid_filter_1d(n, T, B, S, int(route == 'power'), _lib.ptr(xs), _lib.ptr(mean), _lib.ptr(sd),
                                        _lib.LIK['bernoulli_logistic'], 4, _lib.ptr(lik), 0, _lib.ptr(init_ps), 0,
                                        _lib.ptr(ys), None, _lib.ptr(means), _lib.ptr(variances), _lib.ptr(nell), _lib.ptr(fn),
                                        0, stream))

    timer.time_ms(run)                      # warm-up: the pool allocates its blocks
    ms = [timer.time_ms(run) for _ in range(repeats)]
    n_pad, b_pad = -(-n // 64) * 64, -(-B // 64) * 64
    squarings = (S.bit_length() - 1) + (bin(S).count('1') - 1) if route == 'power' and S > 1 else 0
    flop = 2. * n_pad ** 3 * squarings + 2. * n_pad * n_pad * b_pad * T * (1 if route == 'power' and S > 1 else S)
    row = dict(case='benes_bernoulli_grid_filter', n=n, substeps=S, T=T, B=B, route=route, pred_method='chapman-tme-3',
               grid=f'linspace({GRID_LO}, {GRID_HI}, {n})', ms_median=float(np.median(ms)), ms_all=[round(v, 3) for v in ms],
               padded_gemm_tflop=flop / 1e12, tflops_padded=flop / 1e9 / float(np.median(ms)),
               nell_first=float(nell[0]), any_nan=bool((fn >= 0).any()), pdfs_returned=False)
    if nz:
        m_pad = -(-nz // 64) * 64
        row.update(nz=nz, zs=f'linspace(-2, 2, {nz})', cf_padded_gemm_tflop=2. * 2 * m_pad * n_pad * b_pad * T / 1e12,
                   cfs_gigabytes=cfs.nbytes / 1e9, cf_abs_max=float(np.nanmax(np.abs(cfs[0]))))
    return row


def bench_gemm(timer, size, iters):
    L = _lib.lib()
    rng = np.random.default_rng(0)
    A, Bm = rng.random((size, size)), rng.random((size, size))
    dA, dB, dC = _lib.DeviceBuffer.from_array(A), _lib.DeviceBuffer.from_array(Bm), _lib.DeviceBuffer(size * size * 8)

    def run(stream):
        for _ in range(iters):
            _lib.check(L.mfs_grid_gemm_dev(size, size, size, dA.ptr, dB.ptr, dC.ptr, stream))

    timer.time_ms(run)
    ms = timer.time_ms(run) / iters
    tf = 2. * size ** 3 / 1e9 / ms
    out = [dict(case='grid_gemm_fp64', M=size, N=size, K=size, ms=ms, tflops=tf, fraction_of_peak=tf / FP64_MATRIX_PEAK_TFLOPS,
                peak_tflops=FP64_MATRIX_PEAK_TFLOPS)]
    out.append(bench_rocblas(timer, size, iters, dA, dB, dC, tf))
    for b in (dA, dB, dC):
        b.free()
    return out


def bench_rocblas(timer, size, iters, dA, dB, dC, ours_tf):
    """rocblas_dgemm on the same buffers, loaded through ctypes in this process only (the library links no BLAS)."""
    rb, why = None, ''
    for path in ('librocblas.so', os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'librocblas.so')):
        try:
            rb = C.CDLL(path)
            break
        except OSError as e:
            why = str(e)
    if rb is None:
        return dict(case='rocblas_dgemm_fp64', available=False, reason=why)
    handle = C.c_void_p()
    if rb.rocblas_create_handle(C.byref(handle)) != 0:
        return dict(case='rocblas_dgemm_fp64', available=False, reason='rocblas_create_handle failed')
    rb.rocblas_set_stream(handle, timer.stream)
    one, zero = C.c_double(1.), C.c_double(0.)
    OP_NONE = 111
    rb.rocblas_dgemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    status = []

    def run(_stream):
        for _ in range(iters):   # row-major C = A B is column-major C^T = B^T A^T
            status.append(rb.rocblas_dgemm(handle, OP_NONE, OP_NONE, size, size, size, C.byref(one), dB.ptr, size, dA.ptr, size,
                                           C.byref(zero), dC.ptr, size))

    timer.time_ms(run)
    ms = timer.time_ms(run) / iters
    rb.rocblas_destroy_handle(handle)
    if any(status):
        return dict(case='rocblas_dgemm_fp64', available=False, reason=f'rocblas_dgemm returned {max(status)}')
    tf = 2. * size ** 3 / 1e9 / ms
    return dict(case='rocblas_dgemm_fp64', available=True, M=size, N=size, K=size, ms=ms, tflops=tf,
                fraction_of_peak=tf / FP64_MATRIX_PEAK_TFLOPS, grid_gemm_over_rocblas=ours_tf / tf)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batches', default='1,64,1000')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='a small shape (n = 256, S = 10, T = 10): checks the tool, not the device')
    ap.add_argument('--nz', type=int, default=0, help='frequencies of the posteriors\' characteristic functions (0: none, '
                                                      'mfs_grid_filter_1d as before)')
    ap.add_argument('--routes', default='power,stepwise')
    ap.add_argument('--no-gemm', action='store_true', help='skip the GEMM-alone rows')
    a = ap.parse_args()
    n, S, T, size, iters = (256, 10, 10, 256, 2) if a.quick else (2000, 100, 100, 2048, 200)
    timer = Timer()
    print(json.dumps(dict(case='device', name=_lib.device_name(0))), flush=True)
    for B in [int(v) for v in a.batches.split(',')]:
        for route in a.routes.split(','):
            print(json.dumps(bench_filter(timer, n, S, T, B, route, a.repeats, a.nz)), flush=True)
    if not a.no_gemm:
        for row in bench_gemm(timer, size, iters):
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
