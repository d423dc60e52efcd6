"""The import layers of tests/: test modules (test_*.py) share code through plain support modules only (plan_api.py,
one_dim_support.py, nd_support.py, nd_envelope_models.py, nd3_models.py, the *_ref.py yardsticks, ...), every import is
absolute (`from tests import x`, `from tests.x import y`), no support module reaches a test module, directly or through
another support module, and the project's own modules (mfs_amd, oracle, tests) are imported at module level, where a reader
and this file see them.  Every tests/**/*.py is parsed, none is imported: no GPU and no library."""
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


def _imports_in_functions(path):
    """-> [(line, dotted name)] of the import statements inside a function body, at any depth."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    out = []
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
            for node in ast.walk(fn):
                if isinstance(node, ast.Import):
                    out += [(node.lineno, a.name) for a in node.names]
                elif isinstance(node, ast.ImportFrom) and node.module:
                    out += [(node.lineno, node.module)]
    return sorted(set(out))


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


# (file under tests/, imported module) -> why this import of a project module stays inside a function
IN_FUNCTION_IMPORTS = {
    # The two exact-arithmetic yardsticks, and the golden generator of the second, import with mpmath and NumPy alone;
    # only the function that hands numbers to the product, or builds the product's host tables, loads it.
    ('device_math_ref.py', 'mfs_amd'): 'call() is the one function that needs the library',
    ('gaussian_filters_exact.py', 'mfs_amd'): 'host_tables() builds the product\'s tables',
    ('gaussian_filters_exact.py', 'mfs_amd.classical_filters_smoothers'): 'the rules come from the product\'s SigmaPoints',
    ('gaussian_filters_exact.py', 'mfs_amd.tme_poly'): 'host_tables() builds the product\'s tables',
    ('gaussian_filters_exact.py', 'mfs_amd.tme_poly_nd'): 'host_tables() builds the product\'s tables',
    ('gaussian_filters_exact.py', 'tests'): 'restatement_of() is the one user of tests/gaussian_filters_ref.py',
}


def test_project_modules_are_imported_at_module_level():
    found = {(os.path.relpath(p, TESTS), name): line for p in FILES for line, name in _imports_in_functions(p)
             if name.split('.')[0] in ('mfs_amd', 'oracle', 'tests')}
    bad = [f'{_where(os.path.join(TESTS, f), line)}: {name}' for (f, name), line in found.items()
           if (f, name) not in IN_FUNCTION_IMPORTS]
    assert not bad, bad
    stale = sorted(set(IN_FUNCTION_IMPORTS) - set(found))
    assert not stale, f'listed but no longer there: {stale}'
