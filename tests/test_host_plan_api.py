"""tests/plan_api.py without a library or a GPU: what assert_same_bits accepts and refuses, and what build_switches does to
the environment."""
import os

import numpy as np
import pytest

from tests.plan_api import SWITCHES, Outputs, assert_same_bits, build_switches


def _record():
    moments = np.arange(24, dtype=np.float64).reshape(2, 3, 4) / 7.
    moments[1, 1:] = np.nan                                     # a replicate poisoned at step 1
    means = np.array([[0.5, -0.25, 0.], [1.5, np.nan, np.nan]])
    return Outputs(moments, means, None, np.array([3.25, np.nan]), np.array([-1, 1], dtype=np.int32))


def _changed(field, edit):
    rec = _record()
    x = rec._asdict()[field].copy()
    x = edit(x)
    return rec._replace(**{field: x})


def _flip_low_bit(x):
    x.view(np.uint64)[0, 0, 1] ^= 1
    return x


def _set(index, value):
    def edit(x):
        x[index] = value
        return x
    return edit


def test_equal_records_with_nans_in_equal_places_pass():
    assert_same_bits(_record(), _record())
    assert_same_bits(_record()[1:], _record()[1:])
    assert_same_bits([np.float64(-0.)], [np.array(-0.)])       # a sequence of anything array-like


REFUSED = {
    'one flipped low mantissa bit': _changed('moments', _flip_low_bit),
    '-0.0 against 0.0': _changed('means', _set((0, 2), -0.)),
    'a NaN against a number': _changed('nell', _set(0, np.nan)),
    'a NaN in a different place': _changed('means', lambda x: np.array([[0.5, -0.25, 0.], [np.nan, 1.5, np.nan]])),
    'an int32 first_nan that differs': _changed('first_nan', _set(1, 2)),
    'a shape mismatch': _changed('nell', lambda x: x[:, None]),
    'a dtype mismatch': _changed('first_nan', lambda x: x.astype(np.int64)),
    'a record that is one output shorter': _record()[:-1],
    'None against an array': _record()._replace(means=None),
}


@pytest.mark.parametrize('case', list(REFUSED))
def test_differences_are_refused(case):
    other = REFUSED[case]
    if case == '-0.0 against 0.0':
        assert np.array_equal(other.means, _record().means, equal_nan=True)      # a comparison of values would pass
    for a, b in ((_record(), other), (other, _record())):
        with pytest.raises(AssertionError):
            assert_same_bits(a, b, case)


def test_the_label_is_in_the_failure_message():
    with pytest.raises(AssertionError, match='second run: grad'):
        assert_same_bits([np.zeros(2), np.zeros(3)], [np.zeros(2), np.ones(3)], 'second run', names=('nell', 'grad'))


@pytest.fixture
def fake_environ(monkeypatch):
    """os.environ replaced by a dict for the test: nothing here touches the environment of the process."""
    monkeypatch.setattr(os, 'environ', {'HOME': '/nowhere', 'MFS_FAST_BUILD': 'generic', 'MFS_SOLVER': 'dense'})
    return os.environ


def test_switches_are_cleared_set_and_restored(monkeypatch, fake_environ):
    before = dict(fake_environ)
    with build_switches(monkeypatch, MFS_PREDICT_RULE='recompute', MFS_FAST_PARTNER='0'):
        inside = {name: os.environ.get(name) for name in SWITCHES}
    assert inside == dict.fromkeys(SWITCHES, None) | {'MFS_PREDICT_RULE': 'recompute', 'MFS_FAST_PARTNER': '0'}
    assert os.environ is fake_environ and fake_environ == before


def test_switches_are_restored_when_the_body_raises(monkeypatch, fake_environ):
    fake_environ['MFS_FAST_TRAITS'] = 'runtime'
    before = dict(fake_environ)
    with pytest.raises(ZeroDivisionError):
        with build_switches(monkeypatch, MFS_FAST_BUILD='generic'):
            assert os.environ['MFS_FAST_BUILD'] == 'generic' and 'MFS_FAST_TRAITS' not in os.environ
            1 / 0
    assert os.environ is fake_environ and fake_environ == before


def test_an_unknown_switch_is_a_mistake(monkeypatch, fake_environ):
    with pytest.raises(AssertionError):
        with build_switches(monkeypatch, MFS_FAST_BIULD='generic'):
            pass
