"""Exact-arithmetic characteristic functions of the N-point moment rule, N = 2..32, as a golden fixture.

    python tests/golden/make_cf_exact.py [--procs P]          writes tests/golden/cf_exact.npz (numbers only)

`characteristic_fn` maps 2N moments to phi(z) = sum_n w_n exp(i z x_n) with (w, x) the Gauss rule of the moments
(mfs/one_dim/moments.py:309-337).  oracle/exact_mp.py forms that rule in 100-digit arithmetic, where rounding is invisible,
and `mp.expj` evaluates the sum; the result, rounded to complex128, is what every fp64 implementation -- the NumPy oracle,
the HIP kernel -- is scored against.  The inputs are fp64 numbers: moments are computed in mpmath, rounded ONCE, and the
rounded values are what the exact rule, the oracle and the device all receive.

Per order N, V = 5 laws that are not Gaussian: three-component Gaussian mixtures (component means N(0, 0.6^2), variances
U[0.3, 0.9], weights Dirichlet(1, 1, 1)), each in three presentations:

    scaled   standardised moments + mean + scale          central   central moments + mean          raw   raw moments

plus one large-location case (vector 0's standardised moments, mean = 1000, scale = 0.5).  Two frequency grids of 33 points,
symmetric and containing z = 0: narrow, |z scale| <= 2, for every N; wide, |z scale| <= 8, for N <= 12.  A third family for
N <= 12: N-atom discrete laws (perturbed Chebyshev points on [-2, 2], Dirichlet(4, .., 4) weights), whose rule IS the law, so
phi(z) = sum_k p_k exp(i z a_k) is known without any quadrature; closed form and exact-rule value are both stored (|z| <= 4).

A draw is kept only if (i) the exact Cholesky is positive definite in every presentation, (ii) the cf at 100 and at 140
digits agree to 1e-30, and (iii) the conditions on the reference that tests/test_host_characteristic_ref.py asserts hold:
the fp64 oracle is within 4 floors of exact on the narrow grid, floor = (N + max|z x_n|) 2^-53, and within 1e-10 on the wide
grid and on the discrete laws, and (iv) for a discrete law the exact rule's cf is within 1e-9 of the closed form (the gap
is the fp64 rounding of the input moments).  A draw that misses one is replaced by the next attempt of its seed sequence -- never skipped --
and the attempt number is stored.
"""
import argparse
import multiprocessing as mp_
import os
import sys
import time

for _v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):   # forked workers + threaded BLAS deadlock
    os.environ.setdefault(_v, '1')

import mpmath as mp  # noqa: E402
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import exact_mp, one_dim as o  # noqa: E402

SEED = 20261019
V = 5                       # mixture laws per order
VD = 2                      # discrete laws per order
ORDERS = tuple(range(2, 33))
WIDE_NMAX = 12              # the oracle's own error on the wide grid reaches 1e-10 near N = 16
DISC_NMAX = 12
DPS, DPS_CHECK = 100, 140
NZ = 33
U_NARROW = np.linspace(-2., 2., NZ)      # z scale
U_WIDE = np.linspace(-8., 8., NZ)
Z_DISC = np.linspace(-4., 4., NZ)
KINDS = ('scaled', 'central', 'raw', 'large')
LARGE_MEAN, LARGE_SCALE = 1000., 0.5
NARROW_FLOORS = 4.          # condition on the reference, narrow grid: e_ref <= 4 floors
WIDE_BOUND = 1e-10          # condition on the reference, wide grid and discrete laws
DISC_BOUND = 1e-9           # discrete laws: exact rule of the fp64 moments against the closed form of the law
U53 = 2.0 ** -53


def floor_of(N, zx):
    return (N + zx) * U53


# ---------------------------------------------------------------------------------------------------------------------
# laws
# ---------------------------------------------------------------------------------------------------------------------
def _normal_moment(m, v, p):
    """E[(m + sqrt(v) Z)^p], Z standard normal, in the working precision."""
    return mp.fsum(mp.binomial(p, k) * m ** (p - k) * v ** (k // 2) * (mp.fac2(k - 1) if k else 1)
                   for k in range(0, p + 1, 2))


def mixture_presentations(N, rng):
    """The three presentations of one mixture law: {kind: (ms fp64 (2N,), mean or None, scale or None)}."""
    mp.mp.dps = DPS
    ws = rng.dirichlet(np.ones(3))
    mus = rng.normal(scale=0.6, size=3)
    vs = rng.uniform(0.3, 0.9, size=3)
    wm = [mp.mpf(float(w)) for w in ws]
    tot = mp.fsum(wm)
    wm = [w / tot for w in wm]
    mm, vm = [mp.mpf(float(m)) for m in mus], [mp.mpf(float(v)) for v in vs]
    raw = [mp.fsum(w * _normal_moment(m, v, p) for w, m, v in zip(wm, mm, vm)) for p in range(2 * N)]
    mean = raw[1]
    cen = [mp.fsum(w * _normal_moment(m - mean, v, p) for w, m, v in zip(wm, mm, vm)) for p in range(2 * N)]
    sd = mp.sqrt(cen[2])
    std = [cen[p] / sd ** p for p in range(2 * N)]
    f = lambda xs: np.array([float(x) for x in xs])   # noqa: E731
    return {'scaled': (f(std), float(mean), float(sd)), 'central': (f(cen), float(mean), None), 'raw': (f(raw), None, None)}


def discrete_law(N, rng):
    """Atoms (fp64, taken exactly), probabilities (mpf, normalised exactly) and the fp64 raw moments of an N-atom law."""
    mp.mp.dps = DPS
    k = np.arange(N)
    atoms = -np.cos((k + 0.5) * np.pi / N) * 2.0 + rng.uniform(-0.2, 0.2, N) / N
    probs = rng.dirichlet(np.ones(N) * 4)
    am = [mp.mpf(float(a)) for a in atoms]
    pm = [mp.mpf(float(p)) for p in probs]
    tot = mp.fsum(pm)
    pm = [p / tot for p in pm]
    ms = np.array([float(mp.fsum(p * a ** q for p, a in zip(pm, am))) for q in range(2 * N)])
    return atoms, pm, ms


# ---------------------------------------------------------------------------------------------------------------------
# exact values
# ---------------------------------------------------------------------------------------------------------------------
def exact_rule(ms, mean, scale, dps=DPS):
    """(w, x) of oracle.exact_mp.moment_quadrature on the fp64 inputs, as mpf lists; None if G is not positive definite."""
    mp.mp.dps = dps
    return exact_mp.moment_quadrature([mp.mpf(float(v)) for v in ms], mp.mpf(float(0. if mean is None else mean)),
                                      mp.mpf(float(1. if scale is None else scale)))


def cf_of_rule(w, x, zs):
    """sum_n w_n exp(i z x_n) in the working precision, one mpc per z."""
    return [mp.fsum(wi * mp.expj(mp.mpf(float(z)) * xi) for wi, xi in zip(w, x)) for z in zs]


def _round(vals):
    return np.array([complex(v) for v in vals], dtype=np.complex128)


def _agree(a, b):
    return max(abs(u - v) for u, v in zip(a, b)) <= mp.mpf(10) ** -30


def grids_of(N, scale):
    s = 1. if scale is None else scale
    out = {'narrow': U_NARROW / s}
    if N <= WIDE_NMAX:
        out['wide'] = U_WIDE / s
    return out


def evaluate(N, ms, mean, scale, check=True):
    """Exact cf of one case on its grids: {grid: (z, cf complex128, max|z x|)}, or None if the draw has to be replaced
    (not positive definite; with `check`, also 100 against 140 digits)."""
    rule = exact_rule(ms, mean, scale)
    if rule is None:
        return None
    w, x = rule
    hi = exact_rule(ms, mean, scale, DPS_CHECK) if check else None
    if check and hi is None:
        return None
    out = {}
    for grid, zs in grids_of(N, scale).items():
        mp.mp.dps = DPS
        vals = cf_of_rule(w, x, zs)
        if check:
            mp.mp.dps = DPS_CHECK
            if not _agree(vals, cf_of_rule(hi[0], hi[1], zs)):
                return None
        zx = max(abs(float(z)) for z in zs) * max(abs(float(xi)) for xi in x)
        out[grid] = (zs, _round(vals), zx)
    return out


def reference_ok(N, ms, mean, scale, ev):
    """The two conditions on the fp64 oracle (see the module docstring)."""
    for grid, (zs, exact, zx) in ev.items():
        ref = o.characteristic_fn(zs, ms, 0. if mean is None else mean, 1. if scale is None else scale)
        if not np.all(np.isfinite(ref)):
            return False
        e_ref = np.abs(ref - exact).max()
        if e_ref > (NARROW_FLOORS * floor_of(N, zx) if grid == 'narrow' else WIDE_BOUND):
            return False
    return True


def mixture_cases(N, v, attempt, check=True):
    """The cases of mixture law v of order N at a given attempt: list of dicts, or None if the draw is to be replaced."""
    pres = mixture_presentations(N, np.random.default_rng([SEED, N, v, attempt]))
    if v == 0:
        pres['large'] = (pres['scaled'][0], LARGE_MEAN, LARGE_SCALE)
    cases = []
    for kind in KINDS:
        if kind not in pres:
            continue
        ms, mean, scale = pres[kind]
        ev = evaluate(N, ms, mean, scale, check)
        if ev is None or (check and not reference_ok(N, ms, mean, scale, ev)):
            return None
        cases.append(dict(N=N, kind=KINDS.index(kind), vec=v, attempt=attempt, ms=ms, mean=mean, scale=scale, ev=ev))
    return cases


def discrete_case(N, v, attempt, check=True):
    atoms, pm, ms = discrete_law(N, np.random.default_rng([SEED, N, 100 + v, attempt]))
    rule = exact_rule(ms, None, None)
    if rule is None:
        return None
    mp.mp.dps = DPS
    vals = cf_of_rule(rule[0], rule[1], Z_DISC)
    closed = cf_of_rule(pm, [mp.mpf(float(a)) for a in atoms], Z_DISC)
    if check:
        hi = exact_rule(ms, None, None, DPS_CHECK)
        mp.mp.dps = DPS_CHECK
        if hi is None or not _agree(vals, cf_of_rule(hi[0], hi[1], Z_DISC)):
            return None
    zx = np.abs(Z_DISC).max() * max(abs(float(xi)) for xi in rule[1])
    exact = _round(vals)
    if check:
        if np.abs(exact - _round(closed)).max() > DISC_BOUND:
            return None
        ref = o.characteristic_fn(Z_DISC, ms)
        if not np.all(np.isfinite(ref)) or np.abs(ref - exact).max() > WIDE_BOUND:
            return None
    xs = np.sort([float(xi) for xi in rule[1]])
    return dict(N=N, vec=v, attempt=attempt, ms=ms, atoms=atoms, probs=np.array([float(p) for p in pm]), rule=exact,
                closed=_round(closed), zx=zx, atom_err=np.abs(xs - np.sort(atoms)).max())


def cases_of_order(N, attempts=None, check=True):
    """Everything the fixture holds for order N.  attempts = {('mix' | 'disc', v): attempt} replays stored attempts (and a
    replayed draw that fails is an error); None searches from attempt 0."""
    mix, disc = [], []
    for family, count, make, dest in (('mix', V, mixture_cases, mix), ('disc', VD if N <= DISC_NMAX else 0, discrete_case, disc)):
        for v in range(count):
            if attempts is not None:
                got = make(N, v, attempts[family, v], check)
                if got is None:
                    raise RuntimeError(f'N = {N}, {family} {v}: the stored attempt does not reproduce')
            else:
                for attempt in range(64):
                    got = make(N, v, attempt, check)
                    if got is not None:
                        break
                else:
                    raise RuntimeError(f'N = {N}, {family} {v}: no admissible draw in 64 attempts')
            dest.extend(got if family == 'mix' else [got])
    return mix, disc


def pack(per_order):
    """The fixture's arrays from [(mix cases, discrete cases)] in order of N."""
    mix = [c for m, _ in per_order for c in m]
    disc = [c for _, d in per_order for c in d]
    wide = [i for i, c in enumerate(mix) if 'wide' in c['ev']]
    nanif = lambda v: np.nan if v is None else v   # noqa: E731
    out = {
        'seed': SEED, 'dps': DPS, 'dps_check': DPS_CHECK,
        'N': np.array([c['N'] for c in mix], dtype=np.int32), 'kind': np.array([c['kind'] for c in mix], dtype=np.int8),
        'vec': np.array([c['vec'] for c in mix], dtype=np.int8), 'attempt': np.array([c['attempt'] for c in mix], dtype=np.int16),
        'ms': np.concatenate([c['ms'] for c in mix]), 'ms_off': np.cumsum([0] + [len(c['ms']) for c in mix]),
        'mean': np.array([nanif(c['mean']) for c in mix]), 'scale': np.array([nanif(c['scale']) for c in mix]),   # NaN = not passed
        'narrow_z': np.stack([c['ev']['narrow'][0] for c in mix]), 'narrow_cf': np.stack([c['ev']['narrow'][1] for c in mix]),
        'narrow_zx': np.array([c['ev']['narrow'][2] for c in mix]),
        'wide_case': np.array(wide, dtype=np.int32),
        'wide_z': np.stack([mix[i]['ev']['wide'][0] for i in wide]), 'wide_cf': np.stack([mix[i]['ev']['wide'][1] for i in wide]),
        'wide_zx': np.array([mix[i]['ev']['wide'][2] for i in wide]),
        'disc_N': np.array([c['N'] for c in disc], dtype=np.int32), 'disc_vec': np.array([c['vec'] for c in disc], dtype=np.int8),
        'disc_attempt': np.array([c['attempt'] for c in disc], dtype=np.int16),
        'disc_ms': np.concatenate([c['ms'] for c in disc]), 'disc_off': np.cumsum([0] + [len(c['ms']) for c in disc]),
        'disc_atoms': np.concatenate([c['atoms'] for c in disc]), 'disc_probs': np.concatenate([c['probs'] for c in disc]),
        'disc_z': Z_DISC, 'disc_cf_rule': np.stack([c['rule'] for c in disc]), 'disc_cf_closed': np.stack([c['closed'] for c in disc]),
        'disc_zx': np.array([c['zx'] for c in disc]), 'disc_atom_err': np.array([c['atom_err'] for c in disc]),
    }
    return out


def _order(N):
    t0 = time.time()
    got = cases_of_order(N)
    return N, got, time.time() - t0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--procs', type=int, default=max(1, min(16, (os.cpu_count() or 2)) - 1))
    ap.add_argument('--out', type=str, default='cf_exact.npz')
    a = ap.parse_args()
    t0 = time.time()
    res = {}
    with mp_.get_context('fork').Pool(a.procs) as pool:
        for N, got, dt in pool.imap_unordered(_order, sorted(ORDERS, reverse=True), chunksize=1):   # the slow orders first
            res[N] = got
            print(f'N = {N}: {len(got[0])} + {len(got[1])} cases in {dt:.0f} s, attempts '
                  f'{sorted({c["attempt"] for c in got[0] + got[1]})}', flush=True)
    path = os.path.join(HERE, a.out)
    np.savez_compressed(path, **pack([res[N] for N in ORDERS]))
    print(f'{os.path.getsize(path) / 1024:.0f} KiB in {time.time() - t0:.0f} s')
