"""CPU tests of the slot-indexed streaming step (fe_step_slots, fe_state_reset_slots, Engine.step_slots / reset_slots, StreamPool):
argument checks that come before any device work, and the pool's slot bookkeeping with the engine calls stubbed."""
from ctypes import c_void_p

import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import StreamPool

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)


def _err():
    return _lib.load().fe_last_error().decode()


def test_slot_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    assert lib.fe_step_slots(NULL, P, 256, P, 4, P, P, 256, 1, 1, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()
    assert lib.fe_state_reset_slots(NULL, P, 4, P, 1, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


def test_slot_entry_points_refuse_the_baseline_families():
    eng = Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xt"][0]), None)
    lib = eng.lib
    assert lib.fe_step_slots(eng._h, P, 256, P, 4, P, P, 256, 1, 1, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert "FastEnhancer family" in _err() and "dptransformer" in _err()
    assert lib.fe_state_reset_slots(eng._h, P, 4, P, 1, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert "FastEnhancer family" in _err()


def test_slot_entry_points_refuse_the_noncausal_model_as_fe_step_does():
    eng = Engine(product_config("fe_nc"), None)
    assert eng.lib.fe_state_reset_slots(eng._h, P, 4, P, 1, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()
    assert eng.lib.fe_step_slots(eng._h, P, 256, P, 4, P, P, 256, 1, 1, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()


def test_state_reset_slots_checks_its_arguments():
    eng = Engine(product_config("fe_b"), None)
    lib = eng.lib
    for args in [(NULL, 4, P, 1), (P, 4, NULL, 1), (P, 4, P, 0), (P, 4, P, 5), (P, 0, P, 1)]:
        assert lib.fe_state_reset_slots(eng._h, *args, NULL) == FE_ERR_INVALID_ARG, args
        assert "1 <= n <= capacity" in _err()


def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


@pytest.mark.parametrize("slots,match", [
    ([1, 2, 2], "duplicate"),
    ([0, -1], "outside"),
    ([3, 8], "outside"),
    ([0, 9], "outside"),
    (torch.tensor([4, 4], dtype=torch.int32), "duplicate"),
    (torch.tensor([8]), "outside"),
    (torch.tensor([0.0, 1.0]), "integer"),
    ([0, 1.5], "integer"),
    ([True], "integer"),
    ([], "0 slots"),
])
def test_host_slots_are_checked_before_any_device_call(monkeypatch, slots, match):
    eng = Engine(product_config("fe_b"), None)
    _no_native(monkeypatch, eng)
    with pytest.raises(ValueError, match=match):
        eng.step_slots(torch.zeros(2, 256), torch.zeros(1), 8, slots)
    with pytest.raises(ValueError, match=match):
        eng.reset_slots(torch.zeros(1), 8, slots)


def test_valid_host_slots_pass_the_check(monkeypatch):
    """a valid list gets as far as the device requirement (this engine has none), numpy-style integers included"""
    import numpy as np
    eng = Engine(product_config("fe_b"), None)
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        eng.step_slots(torch.zeros(3, 256), torch.zeros(1), 8, [7, 0, np.int64(3)])


class _StubEngine:
    """what StreamPool needs of an Engine, recorded instead of run"""
    def __init__(self):
        self.calls = []

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        self.calls.append(("reset", capacity, list(slots)))

    def step_slots(self, wav_in, state, capacity, slots, wav_out=None, T=1):
        self.calls.append(("step", capacity, list(slots), T))
        return wav_in


def test_stream_pool_hands_out_resets_and_reuses_slots():
    eng = _StubEngine()
    pool = StreamPool(eng, 3)
    a, b, c = pool.open(), pool.open(), pool.open()
    assert (a, b, c) == (0, 1, 2)
    assert eng.calls == [("reset", 3, [0]), ("reset", 3, [1]), ("reset", 3, [2])]
    with pytest.raises(RuntimeError, match="all 3 slots are open"):
        pool.open()
    pool.close(b)
    assert pool.active == [0, 2]
    with pytest.raises(ValueError, match="not open"):
        pool.close(b)
    assert pool.open() == 1                     # the freed slot is reused, and reset again
    assert eng.calls[-1] == ("reset", 3, [1])
    x = torch.zeros(2, 4)
    assert pool.step([2, 0], x) is x
    assert eng.calls[-1] == ("step", 3, [2, 0], 1)
    pool.close(2)
    with pytest.raises(ValueError, match="slot 2 is not open"):
        pool.step([0, 2], x)
    assert eng.calls[-1][0] == "step" and eng.calls[-1][2] == [2, 0]      # (refused before any engine call)


def test_stream_pool_needs_a_capacity():
    with pytest.raises(ValueError):
        StreamPool(_StubEngine(), 0)
