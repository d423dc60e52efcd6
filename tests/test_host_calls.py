"""The Python host layer hands the C ABI exactly what tests/golden/host_calls.npz froze (tests/golden/make_host_calls.py).

libmfs_hip.so is a function of its arguments, so equality here -- entry-point names, scalars, descriptor bytes, the tables
the descriptors point to, array bytes, returned bytes, exception and warning text, with no tolerance anywhere -- means the
public filters compute what they computed when the fixture was made.  No GPU and no library: the recorder stands in for it."""
import importlib.util
import json
import os

import numpy as np
import pytest


def _load_generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'make_host_calls.py')
    spec = importlib.util.spec_from_file_location('make_host_calls', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_generator()


@pytest.fixture(scope='module')
def frozen(golden_dir):
    with np.load(os.path.join(golden_dir, 'host_calls.npz')) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope='module')
def replayed():
    with pytest.MonkeyPatch.context() as mp:
        return gen.record(mp)


def test_case_list_and_coverage(frozen, replayed):
    assert sorted(frozen) == sorted(replayed)
    assert {k[:-5] for k in frozen if k.endswith('/meta')} == set(gen.CASES)
    gen.check_coverage(frozen)
    gen.check_coverage(replayed)


@pytest.mark.parametrize('name', list(gen.CASES))
def test_case_reaches_the_c_abi_unchanged(frozen, replayed, name):
    want, got = json.loads(str(frozen[f'{name}/meta'])), json.loads(str(replayed[f'{name}/meta']))
    assert got.get('raised') == want.get('raised')
    assert got['warnings'] == want['warnings']
    assert [c['entry'] for c in got['calls']] == [c['entry'] for c in want['calls']]
    assert got == want                    # scalars, dtypes, shapes, SHA-256 of the large arrays, what was returned
    keys = sorted(k for k in frozen if k.startswith(name + '/') and not k.endswith('/meta'))
    assert keys == sorted(k for k in replayed if k.startswith(name + '/') and not k.endswith('/meta'))
    for k in keys:
        a, b = replayed[k], frozen[k]
        assert (a.dtype, a.shape) == (b.dtype, b.shape) and a.tobytes() == b.tobytes(), k

