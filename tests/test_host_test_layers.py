"""The import layers of tests/: test modules (test_*.py) share code through plain support modules only (plan_api.py,
nd_support.py, nd_envelope_models.py, nd3_models.py, the *_ref.py yardsticks, ...), every import is absolute
(`from tests import x`, `from tests.x import y`), and no support module reaches a test module, directly or through another
support module.  Every tests/**/*.py is parsed, none is imported: no GPU and no library."""
import ast
import glob
import os

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
FILES = sorted(glob.glob(os.path.join(TESTS, '**', '*.py'), recursive=True))


def _module(path):
    """tests/golden/make_x.py -> 'tests.golden.make_x'."""
    rel = os.path.relpath(path, os.path.dirname(TESTS))[:-3].split(os.sep)
    return '.'.join(rel[:-1] if rel[-1] == '__init__' else rel)


MODULES = {_module(p): p for p in FILES}


def _is_test(module):
    return module.rsplit('.', 1)[-1].startswith('test_')


def _imports(path):
    """-> [(line, relative level, dotted name)] of every import statement of the file, at any depth; `from a import b` gives
    'a.b', which names a module when b is one."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            out += [(node.lineno, 0, a.name) for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            out += [(node.lineno, node.level, f'{node.module}.{a.name}' if node.module else a.name) for a in node.names]
    return out


def _where(path, line):
    return f'{os.path.relpath(path, TESTS)}:{line}'


def test_the_walk_sees_the_tests():
    assert 'tests.nd_support' in MODULES and 'tests.test_host_test_layers' in MODULES and 'tests.golden.make_nd3_golden' in MODULES
    assert any(name == 'ast' for _, _, name in _imports(__file__))


def test_no_relative_imports():
    bad = [_where(p, line) for p in FILES for line, level, _ in _imports(p) if level > 0]
    assert not bad, bad


def test_no_import_names_a_test_module():
    """Neither `import tests.test_x`, nor `from tests import test_x`, nor `from tests.test_x import y`."""
    bad = [f'{_where(p, line)}: {name}' for p in FILES for line, _, name in _imports(p)
           if any(part.startswith('test_') for part in name.split('.'))]
    assert not bad, bad


def _reached(module, seen):
    """Every module of tests/ that `module` imports, directly or through the modules it imports."""
    for _, _, name in _imports(MODULES[module]):
        parts = name.split('.')
        for n in range(len(parts), 0, -1):
            target = '.'.join(parts[:n])
            if target in MODULES and target not in seen:
                seen.add(target)
                _reached(target, seen)
            if target in MODULES:
                break
    return seen


@pytest.mark.parametrize('module', [m for m in MODULES if not _is_test(m) and not m.endswith('conftest')])
def test_support_modules_reach_no_test_module(module):
    reached = _reached(module, set())
    assert not [m for m in reached if _is_test(m)], sorted(reached)
