"""The trainer's capture guard (``runtime/trainer.py _no_gc``): dead cycles are collected before
the block and the cyclic collector stays off inside it, so no finalizer of an object that died
earlier runs in the middle of a stream capture."""
import gc
import weakref

import pytest

from ewdml.runtime.trainer import _no_gc


class _Node:
    pass


def _dead_cycle():
    a = _Node()
    a.me = a
    return weakref.ref(a)


def test_collects_before_and_keeps_the_collector_off_inside():
    assert gc.isenabled()
    gc.disable()  # so that the cycle below is certainly still there at the block's entry
    old = _dead_cycle()
    gc.enable()
    assert old() is not None
    with _no_gc():
        assert old() is None  # collected on entry
        assert not gc.isenabled()
        inner = _dead_cycle()
        junk = [[_Node() for _ in range(100)] for _ in range(200)]  # far past gen-0's threshold
        assert inner() is not None and len(junk) == 200
    assert gc.isenabled()
    gc.collect()
    assert inner() is None


def test_restores_the_collector_state_and_passes_exceptions_on():
    gc.disable()
    try:
        with _no_gc():
            assert not gc.isenabled()
        assert not gc.isenabled()  # it was off before: left off
    finally:
        gc.enable()
    with pytest.raises(KeyError):
        with _no_gc():
            raise KeyError("x")
    assert gc.isenabled()
