"""CPU tests of fe_step_pool - fe_step_slots for every family with a streaming state (fe_step_pool, Engine.step_pool, family.slot_step and
which of step_slots / step_pool StreamPool.step calls): the declarations, the argument checks that come before any device work, and the
pool's choice with the engine calls recorded instead of run."""
import re
from ctypes import c_void_p
from pathlib import Path

import pytest
import torch

from common import hip_engine, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.family import slot_step
from fastenhancer_amd.serving import StreamPool

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"

# (wav_in, in_stride, state, capacity, slots, wav_out, out_stride, n, T) of every refusal fe_step_slots makes before device work, H = 256
BAD_ARGS = [
    (NULL, 256, P, 4, P, P, 256, 2, 1), (P, 256, NULL, 4, P, P, 256, 2, 1), (P, 256, P, 4, NULL, P, 256, 2, 1), (P, 256, P, 4, P, NULL, 256, 2, 1),
    (P, 256, P, 4, P, P, 256, 0, 1), (P, 256, P, 4, P, P, 256, -1, 1), (P, 256, P, 4, P, P, 256, 5, 1), (P, 256, P, 0, P, P, 256, 1, 1),
    (P, 256, P, 4, P, P, 256, 2, 0), (P, 256, P, 4, P, P, 256, 2, -2),
    (P, 255, P, 4, P, P, 256, 2, 1), (P, 256, P, 4, P, P, 255, 2, 1), (P, 3 * 256 - 1, P, 4, P, P, 3 * 256, 2, 3), (P, 3 * 256, P, 4, P, P, 256, 2, 3),
]


def _err():
    return _lib.load().fe_last_error().decode()


def test_the_header_declares_fe_step_pool_and_the_binding_types_it_like_fe_step_slots():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(fe_step_(?:pool|slots))\s*\(([^)]*)\)\s*;", text)}
    assert set(decls) == {"fe_step_pool", "fe_step_slots"}
    assert decls["fe_step_pool"] == decls["fe_step_slots"]                           # the same parameter list, word for word
    assert _lib.SYMBOLS["fe_step_pool"] == _lib.SYMBOLS["fe_step_slots"]
    lib = _lib.load()
    assert lib.fe_step_pool.argtypes == lib.fe_step_slots.argtypes and lib.fe_step_pool.restype == lib.fe_step_slots.restype


def test_step_pool_refuses_a_null_handle():
    lib = _lib.load()
    assert lib.fe_step_pool(NULL, P, 256, P, 4, P, P, 256, 1, 1, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("name", ["fe_b", "bsrnn_xxt", "fspen", "lisennet"])
def test_step_pool_answers_every_bad_call_as_fe_step_slots_does(name):
    """code and wording of fe_step_slots on a FastEnhancer handle in the same condition (these handles have no weights: the call is refused
    before its arguments are looked at, as fe_step_slots refuses it; tests/test_gpu_step_pool.py repeats the cases on loaded handles)"""
    ref, eng = hip_engine("fe_b"), hip_engine(name)
    assert ref.cfg.hop_size == eng.cfg.hop_size == 256
    for args in BAD_ARGS + [(P, 256, P, 4, P, P, 256, 2, 1)]:
        want = (ref.lib.fe_step_slots(ref._h, *args, NULL), _err())
        assert want[0] != 0
        got = (eng.lib.fe_step_pool(eng._h, *args, NULL), _err())
        assert got == want, (args, got, want)


def test_step_pool_refuses_the_noncausal_model_as_fe_step_does():
    eng = hip_engine("fe_nc")
    assert eng.lib.fe_step_pool(eng._h, P, 256, P, 4, P, P, 256, 1, 1, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err() and "use fe_offline" in _err()


def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


@pytest.mark.parametrize("name", ["bsrnn_xxt", "lisennet"])
@pytest.mark.parametrize("slots,match", [
    ([1, 2, 2], "duplicate"),
    ([0, -1], "outside"),
    ([3, 8], "outside"),
    (torch.tensor([4, 4], dtype=torch.int32), "duplicate"),
    (torch.tensor([0.0, 1.0]), "integer"),
    ([True], "integer"),
    ([], "0 slots"),
])
def test_step_pool_checks_host_slots_before_any_native_call(monkeypatch, name, slots, match):
    eng = hip_engine(name)
    _no_native(monkeypatch, eng)
    with pytest.raises(ValueError, match=match):
        eng.step_pool(torch.zeros(2, 256), torch.zeros(1), 8, slots)


def test_step_pool_rejects_bad_shapes_as_step_slots_does(monkeypatch):
    """the checks are step_slots' own (one code path): the same exception for the same call, and nothing reaches the library"""
    ref, eng = hip_engine("fe_b"), hip_engine("fspen")
    with pytest.raises(_lib.FEError, match="needs a GPU"):          # a valid call gets as far as the device requirement
        eng.step_pool(torch.zeros(3, 256), torch.zeros(1), 8, [7, 0, 3])
    _no_native(monkeypatch, ref)
    _no_native(monkeypatch, eng)
    for wav_in, slots in [(torch.zeros(2, 256), [0, 1, 2, 3, 4, 5, 6, 7, 8]), (torch.zeros(2, 256), [9]), (torch.zeros(2, 256), [1, 1])]:
        with pytest.raises(ValueError) as want:
            ref.step_slots(wav_in, torch.zeros(1), 8, slots)
        with pytest.raises(ValueError) as got:
            eng.step_pool(wav_in, torch.zeros(1), 8, slots)
        assert str(got.value) == str(want.value)


class _StubEngine:
    """what StreamPool.step needs of an Engine, recorded instead of run"""
    def __init__(self, cfg=None):
        if cfg is not None:
            self.cfg = cfg
        self.calls = []

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        self.calls.append(("reset", capacity, list(slots)))

    def step_slots(self, wav_in, state, capacity, slots, wav_out=None, T=1):
        self.calls.append(("step_slots", capacity, list(slots), T))
        return wav_in

    def step_pool(self, wav_in, state, capacity, slots, wav_out=None, T=1):
        self.calls.append(("step_pool", capacity, list(slots), T))
        return wav_in


@pytest.mark.parametrize("name,call", [("bsrnn_xxt", "step_pool"), ("bsrnn_s", "step_pool"), ("fspen", "step_pool"), ("lisennet", "step_pool"),
                                       ("fe_b", "step_slots"), ("fe_dpt_t", "step_slots"), (None, "step_slots")])
def test_stream_pool_step_calls_the_familys_slotted_step(name, call):
    eng = _StubEngine(product_config(name) if name else None)
    assert slot_step(eng) == getattr(eng, call)
    pool = StreamPool(eng, 4)
    a, b, c = pool.open(), pool.open(), pool.open()
    del eng.calls[:]
    x = torch.zeros(2, 8)
    assert pool.step([c, a], x, T=2) is x
    assert eng.calls == [(call, 4, [c, a], 2)]
    pool.close(a)
    with pytest.raises(ValueError, match=f"slot {a} is not open"):
        pool.step([c, a], x)
    assert len(eng.calls) == 1                      # (refused before any engine call)
