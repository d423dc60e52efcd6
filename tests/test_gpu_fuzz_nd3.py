"""A seeded randomised sweep of the d = 3 entry points against the oracle, shaped like tests/test_gpu_fuzz_nd.py: order
N in {2, 3, 4}, transition family (operator TME-1 / TME-2 tables, TME-normal-2 / -3 and Euler closures), representation
(raw / central / scaled), stable off / on, model (Lorenz-63, 3-species Lotka--Volterra, 3-D OU), length and data seed drawn
at random; T is capped by N (12 / 6 / 3 at N = 2 / 3 / 4) to bound the oracle's CPU time.  Every case: replicate 1 of a
batch of 2 against oracle/multi_dims.py at 1e-6 with the natural-magnitude floor, and the NaN criterion of
tests/test_gpu_fuzz_1d.py (compare() of tests/nd_support.py).  Raw moments about the origin of Lorenz-63 at
N = 4 (a law of sd 0.1 centred at (0.1, 0.1, 2.4)) have a Gram matrix singular to working precision from the start; that
combination runs in central mode, as tests/test_gpu_nd3.py does.  (The same sweep run off-line over 180 cases, seeds 1-30,
with the final kernels and criterion: no failure.)"""
import numpy as np
import pytest

from tests.nd3_models import MODELS, family
from tests.nd_support import MODES, compare, initial, run_device, run_oracle, tables

pytestmark = pytest.mark.gpu

FAMILIES = ('tme_1', 'tme_2', 'tme_normal_2', 'tme_normal_3', 'euler')
T_MAX = {2: 12, 3: 6, 4: 3}


def draw_cases(seed, n=6):
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        N = int(rng.integers(2, 5))
        fam = str(rng.choice(FAMILIES))
        mode = str(rng.choice(MODES))
        stable = bool(rng.integers(0, 2))
        model = str(rng.choice(sorted(MODELS)))
        T = int(rng.integers(2, T_MAX[N] + 1))
        dseed = int(rng.integers(1, 10 ** 6))
        if mode == 'raw' and N == 4 and model == 'lorenz':
            mode = 'central'
        cases.append((N, fam, mode, stable, model, T, dseed))
    return cases


def run_case(N, fam, mode, stable, model, T, dseed):
    mi, inds = tables(3, N)
    m = MODELS[model]
    fns, sig, ofns = family(model, fam, N)
    st = initial(mi, m.mean0, m.cov0)
    ys = m.ys(2, T, dseed)
    got = run_device(mode, fns, sig, m.pdf, ys, mi, inds, st, stable)
    ref = run_oracle(mode, ofns, sig, m.opdf, ys[1], mi, inds, st, stable, completed=True)
    compare(got, 1, ref, mi, inds, f'N={N} {fam} {mode} stable={stable} {model} T={T} seed={dseed}')


@pytest.mark.parametrize('seed', [5, 6])
def test_random_nd3_cases_match_oracle(seed):
    for case in draw_cases(seed):
        run_case(*case)
