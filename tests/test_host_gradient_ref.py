"""The condition on the reference of tests/test_gpu_gradient_envelope.py, checked without a GPU (tests/gradient_ref.py).

The device's gradient is held to 2e-6 of max_p |g_ref| against Richardson-combined central differences of the CPU C port
along random directions in table space.  Before that means anything the reference has to be better than the bound by a wide
margin, and that is a statement about the C port alone: its values at the steps h = 1e-3, 3e-4 and 1e-4 must agree within
1e-7 of max_p |g_ref| (truncation shrinks with h, rounding grows, so agreement over a decade bounds both).  Every case the
device file runs is checked here; a case that misses the condition gets other measurements or a shorter run in
gradient_ref._RUNS, never a wider bound."""
import ast
import os

import numpy as np
import pytest

from oracle import c_oracle
from tests import gradient_ref as G

_worst = {}


@pytest.mark.parametrize('case', G.ALL_CASES, ids=lambda c: c.id)
def test_reference_values_at_three_steps_agree(case):
    nell, grad = G.reference(case)
    assert nell.shape == (case.B,) and grad.shape == (case.B, case.P)
    assert np.all(np.isfinite(nell)) and np.all(np.isfinite(grad))
    assert np.all(np.abs(grad).max(axis=-1) > 0.)
    spread = G.reference_spread(case).max()
    key = (case.group, case.N)
    _worst[key] = max(_worst.get(key, 0.), spread)
    assert spread <= G.SPREAD_BOUND, f'{case.id}: spread {spread:.2e} of max |g_ref|'


def test_worst_spread_per_order():
    """The figures DESIGN.md section 4 quotes (run after the cases above; prints with -s)."""
    for group in sorted({g for g, _ in _worst}):
        print(group, ' '.join(f'N={N}: {s:.1e}' for (g, N), s in sorted(_worst.items()) if g == group))
    assert all(s <= G.SPREAD_BOUND for s in _worst.values())


@pytest.mark.parametrize('case', G.POISON_AT_START, ids=lambda c: c.id)
def test_orders_without_a_rule_poison_in_the_first_step(case):
    """Model E at N = 15, 16: the C port returns NaN from step 0 on for every replicate (gradient_ref._no_rule)."""
    x = G.inputs(case)
    bs = G.base(case.model, case.mode, case.N)
    kind, umap, K, mxc, lik_kind = G._kinds(bs)
    m, _, _, nell = c_oracle.filter_1d(G.MODES.index(case.mode), case.N, x.ys, x.m0, x.mean0, x.scale0, kind, umap, K,
                                       x.coef, mxc, lik_kind, x.lp)
    assert np.all(np.isnan(nell)) and np.all(np.isnan(m[:, 0]))


def test_case_list_is_the_one_the_device_file_runs():
    """The device file is read, not imported (tests/test_host_test_layers.py): it must draw on each of the lists that make up
    ALL_CASES."""
    groups = ('EVERY_INSTANTIATION', 'MATRIX', 'BATCHING', 'GEOMETRY', 'LONG')
    assert G.ALL_CASES == sum((getattr(G, g) for g in groups), [])
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_gradient_envelope.py')) as f:
        used = {n.attr for n in ast.walk(ast.parse(f.read()))
                if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == 'G'}
    assert set(groups) <= used
    ids = [c.id for c in G.ALL_CASES + G.POISON_AT_START]
    assert len(set(ids)) == len(ids)
    assert {(c.N, c.P) for c in G.EVERY_INSTANTIATION} == {(N, P) for N in range(2, 17) for P in range(1, 5)}
    assert {c.N for c in G.MATRIX} == set(G.MATRIX_N) and {c.mode for c in G.MATRIX} == set(G.MODES)
    assert {c.model for c in G.MATRIX} == {'A2', 'B', 'C', 'D', 'E'}


def test_directions_move_every_nonzero_entry_and_keep_zeros():
    for case in (G.EVERY_INSTANTIATION[-1], G.BATCHING[3], G.MATRIX[0]):
        x = G.inputs(case)
        for tab, d in ((x.coef, x.dcoef), (x.lp, x.dlik)):
            moved = np.broadcast_to(tab[:, None] != 0., d.shape)
            assert np.all((d != 0.) == moved)
            assert np.all(np.abs(d) <= np.abs(tab[:, None]))
        if case.P > 1:
            assert not np.array_equal(x.dcoef[:, 0], x.dcoef[:, 1])
