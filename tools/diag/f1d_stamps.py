"""Phase stamps of the 1-D fast kernel on a headline-shaped case (N = 15, Benes-Bernoulli, TME-3, central; B = 64 is one wave
per SIMD, so the plan picks the one-wave build).  MFS_FAST_BUILD=generic stamps the generic one-wave build, the default
the specialised one.  Read the SHARES: the stamps themselves (a clock read and an add to a global counter by lane 0) cost
cycles, and the Horner wait stamp drains the LDS queue where the plain build would not."""
import sys, os, ctypes as C, numpy as np
sys.path.insert(0, '.')
from mfs_amd import _lib, synth
_lib.LIB_PATH = os.path.abspath('tools/diag/libmfs_stamps.so')
from mfs_amd.one_dim import filtering, moments, ss_models
N, T, B = 15, int(os.environ.get('STAMP_T', '200')), 64
dt, _, _, ic, drift, dispersion, _, pmf, _ = ss_models.benes_bernoulli(N)
_, c, _, mu, _ = moments.sde_cond_moments_tme(drift, dispersion, dt, 3)
ys, _ = synth.benes_bernoulli_batch(B, T, dt, seed=100)
m, means, nell, fn = filtering.moment_filter_cms(c, mu, pmf, ic.cms, ic.mean, ys, return_first_nan=True)
st = (C.c_ulonglong * 32)()
L = _lib.lib(); L.mfs_debug_stamps.argtypes = [C.c_void_p]; print('rc', L.mfs_debug_stamps(st))
st = np.array(list(st), dtype=np.float64)
print('build', os.environ.get('MFS_FAST_BUILD', 'specialised (default)'), ' T', T)
halves = st[9]
steps = halves / 2
print('iterations per quadrature: predict half', st[11] / steps, 'update half', st[12] / steps)
print('filter 0 first_nan', fn[0], 'half-steps', halves, 'laguerre iterations per quadrature', st[10] / halves)
# (slot, label): every phase occurs once per step, except the Hankel gather (both halves)
phases = [
    (0, 'hankel gather (both halves)'),
    (1, 'predict: elimination (poison decision; atoms rule)'),
    (13, 'predict: tanh'),
    (15, 'predict: horner, all rows'),
    (18, 'predict: mean reduction'),
    (5, 'predict: operator moments -> table'),
    (7, 'predict: moment reduction'),
    (16, 'update: elimination'),
    (2, 'update: jacobi coefficients'),
    (3, 'update: laguerre'),
    (4, 'update: weights'),
    (17, 'update: likelihood + p_y reduction'),
    (6, 'update: mean reduction, powers -> table, log p_y'),
    (8, 'update: moment reduction'),
]
tot = sum(st[i] for i, _ in phases)
for i, n in phases:
    print(f'{n:52s} {st[i] / steps:9.0f} cycles per step   {100 * st[i] / tot:5.1f} % of stamped')
print(f'{"  of horner: LDS reads issued + waited for":52s} {st[14] / steps:9.0f} cycles per step   {100 * st[14] / tot:5.1f} %')
print(f'{"  of horner: arithmetic (and the stamp itself)":52s} {(st[15] - st[14]) / steps:9.0f} cycles per step   {100 * (st[15] - st[14]) / tot:5.1f} %')
print('stamped cycles per step', tot / steps)
