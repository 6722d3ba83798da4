"""The table of device input modes (semireward_amd/data/modes.py): which record a configuration turns on, the refusal of two keys set
together, and that AlgorithmBase's three booleans say the same as its ``input_mode``."""
import argparse

import pytest

from semireward_amd.core.algorithmbase import AlgorithmBase
from semireward_amd.data.modes import MODES, active_mode

KEYS = ("device_tokens", "device_audio", "device_data")              # the fixed order of the table
PAIRS = {("device_audio", "device_data"): r"device_audio and device_data are two input pipelines \(waveforms / images\): set one of them",
         ("device_tokens", "device_data"): r"device_tokens and device_data are two input pipelines \(token batches / images\): set one of them",
         ("device_tokens", "device_audio"): r"device_tokens and device_audio are two input pipelines \(token batches / waveforms\): set one of them"}


class _Seen(Exception):
    pass


class _Probe(AlgorithmBase):
    """Stops where the first dataset would be looked at: what __init__ decided from the yaml keys alone."""

    def set_dataset(self):
        raise _Seen(self.input_mode, {k: getattr(self, k) for k in KEYS})


def _args(**kw):
    return argparse.Namespace(num_classes=2, num_train_iter=2, **kw)


def test_the_table_keeps_its_order():
    assert tuple(m.key for m in MODES) == KEYS


def test_no_key_no_mode():
    for kw in ({}, {k: False for k in KEYS}):
        assert active_mode(_args(**kw)) is None
        with pytest.raises(_Seen) as e:
            _Probe(_args(**kw), None)
        assert e.value.args == (None, {k: False for k in KEYS})


@pytest.mark.parametrize("key", KEYS)
def test_one_key_its_record_and_the_booleans_agree(key):
    mode = active_mode(_args(**{key: True}))
    assert mode is MODES[KEYS.index(key)] and mode.key == key
    assert active_mode(_args(), also=key) is mode
    with pytest.raises(_Seen) as e:
        _Probe(_args(**{key: True}), None)
    seen, flags = e.value.args
    assert seen is mode and flags == {k: k == key for k in KEYS}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_two_keys_are_refused_with_the_pinned_message(pair):
    for order in (pair, pair[::-1]):
        a = _args(**{k: True for k in order})
        with pytest.raises(ValueError, match=PAIRS[pair]):
            active_mode(a)
        with pytest.raises(ValueError, match=PAIRS[pair]):
            _Probe(a, None)
