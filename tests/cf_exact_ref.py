"""Views of tests/golden/cf_exact.npz (written by tests/golden/make_cf_exact.py) shared by
tests/test_host_characteristic_ref.py and tests/test_gpu_characteristic_envelope.py: the exact-arithmetic characteristic
function of the N-point moment rule on fp64 inputs, N = 2..32, the floor both suites measure against, and the fp64 NumPy
oracle's own error e_ref.  The fixture is loaded once and never written to."""
import functools
import importlib.util
import os
from typing import NamedTuple, Optional

import numpy as np

from oracle import one_dim as o

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ('scaled', 'central', 'raw', 'large')
GRIDS = ('narrow', 'wide', 'discrete')
ORDERS = tuple(range(2, 33))
U53 = 2.0 ** -53
NARROW_FLOORS = 4.      # condition on the reference, narrow grid: e_ref <= 4 floors
WIDE_BOUND = 1e-10      # condition on the reference, wide grid and discrete laws
DISC_BOUND = 1e-9       # discrete laws: exact rule of the fp64 moments against the closed form


class Case(NamedTuple):
    N: int
    grid: str                 # 'narrow' | 'wide' | 'discrete'
    kind: str                 # 'scaled' | 'central' | 'raw' | 'large' | 'discrete'
    vec: int
    ms: np.ndarray            # (2N,)
    mean: Optional[float]     # None = not passed
    scale: Optional[float]
    z: np.ndarray             # (33,)
    exact: np.ndarray         # (33,) complex128: the exact rule's cf, rounded
    zx: float                 # max |z x_n| over the grid and the exact rule's nodes
    closed: Optional[np.ndarray] = None   # discrete laws: sum_k p_k exp(i z a_k), rounded

    @property
    def id(self):
        return f'N{self.N}-{self.kind}{self.vec}-{self.grid}'

    @property
    def floor(self):
        return floor_of(self.N, self.zx)


def floor_of(N, zx):
    """What rounding alone costs an fp64 evaluation of sum_n w_n exp(i z x_n): N for the sum, max|z x_n| for the rounding of
    the phases, in units of 2^-53."""
    return (N + zx) * U53


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location('make_cf_exact', os.path.join(HERE, 'golden', 'make_cf_exact.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(os.path.join(HERE, 'golden', 'cf_exact.npz')) as f:
        d = {k: f[k] for k in f.files}
    for v in d.values():
        v.setflags(write=False)
    return d


def _opt(v):
    return None if np.isnan(v) else float(v)


@functools.lru_cache(maxsize=None)
def all_cases():
    f = fixture()
    out = []
    for i in range(len(f['N'])):
        out.append(Case(int(f['N'][i]), 'narrow', KINDS[f['kind'][i]], int(f['vec'][i]), f['ms'][f['ms_off'][i]:f['ms_off'][i + 1]],
                        _opt(f['mean'][i]), _opt(f['scale'][i]), f['narrow_z'][i], f['narrow_cf'][i], float(f['narrow_zx'][i])))
    for j, i in enumerate(f['wide_case']):
        c = out[i]
        out.append(c._replace(grid='wide', z=f['wide_z'][j], exact=f['wide_cf'][j], zx=float(f['wide_zx'][j])))
    for i in range(len(f['disc_N'])):
        out.append(Case(int(f['disc_N'][i]), 'discrete', 'discrete', int(f['disc_vec'][i]),
                        f['disc_ms'][f['disc_off'][i]:f['disc_off'][i + 1]], None, None, f['disc_z'], f['disc_cf_rule'][i],
                        float(f['disc_zx'][i]), f['disc_cf_closed'][i]))
    return tuple(out)


def cases(N=None, grid=None, kind=None):
    return [c for c in all_cases() if (N is None or c.N == N) and (grid is None or c.grid == grid)
            and (kind is None or c.kind == kind)]


def vectors(N):
    """The order's five mixture laws in their scaled presentation: (ms (5, 2N), mean (5,), scale (5,))."""
    cs = sorted(cases(N, 'narrow', 'scaled'), key=lambda c: c.vec)
    return np.stack([c.ms for c in cs]), np.array([c.mean for c in cs]), np.array([c.scale for c in cs])


def oracle_cf(c: Case):
    return o.characteristic_fn(c.z, c.ms, 0. if c.mean is None else c.mean, 1. if c.scale is None else c.scale)


@functools.lru_cache(maxsize=None)
def _e_ref():
    return {c.id: float(np.abs(oracle_cf(c) - c.exact).max()) for c in all_cases()}


def e_ref(c: Case):
    """max |fp64 oracle - exact| over the case's grid, computed once per session from the oracle on the same fp64 inputs."""
    return _e_ref()[c.id]
