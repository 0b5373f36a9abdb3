"""CPU tests of the pinned streaming steps (fe_step_pinned, fe_step_slots_pinned, Engine.step_pinned / step_slots_pinned,
StreamPool.step_host): the declarations, and the argument checks that come before any device work - pageable or device audio is refused
before the library is called, so no kernel ever sees memory it would fault on."""
import os
import re
from ctypes import c_void_p

import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import StreamPool

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG, FE_ERR_NO_WEIGHTS = -1, -2, -4
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastenhancer_hip.h")


def _err():
    return _lib.load().fe_last_error().decode()


def _pinned(lib, h, in_stride=256, out_stride=256, B=4, T=1, wav_in=P, state=P, wav_out=P):
    return lib.fe_step_pinned(h, wav_in, in_stride, state, wav_out, out_stride, B, T, NULL)


def _slots_pinned(lib, h, in_stride=256, out_stride=256, cap=8, n=4, T=1, wav_in=P, state=P, slots=P, wav_out=P):
    return lib.fe_step_slots_pinned(h, wav_in, in_stride, state, cap, slots, wav_out, out_stride, n, T, NULL)


def test_header_and_bindings_declare_both_entry_points():
    text = open(HEADER).read()
    assert re.search(r"int fe_step_pinned\(fe_handle\* h, const float\* wav_in_host, size_t in_stride, float\* state_dev, float\* wav_out_host,"
                     r"\s+size_t out_stride,\s+int B, int T, void\* stream\);", text)
    assert re.search(r"int fe_step_slots_pinned\(fe_handle\* h, const float\* wav_in_host, size_t in_stride, float\* state_dev, int capacity,"
                     r"\s+const int\* slots_dev,\s+float\* wav_out_host, size_t out_stride, int n, int T, void\* stream\);", text)
    assert "pin_memory()" in text
    lib = _lib.load()
    assert lib.fe_step_pinned.argtypes is not None and len(lib.fe_step_pinned.argtypes) == 9
    assert lib.fe_step_slots_pinned.argtypes is not None and len(lib.fe_step_slots_pinned.argtypes) == 11


def test_pinned_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    assert _pinned(lib, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()
    assert _slots_pinned(lib, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


def test_pinned_entry_points_refuse_the_baseline_families():
    eng = Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xt"][0]), None)
    assert _pinned(eng.lib, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "fe_step_pinned" in _err() and "FastEnhancer family" in _err()
    assert _slots_pinned(eng.lib, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "fe_step_slots_pinned" in _err() and "FastEnhancer family" in _err()


def test_pinned_entry_points_refuse_the_noncausal_model_as_fe_step_does():
    eng = Engine(product_config("fe_nc"), None)
    for rc in (_pinned(eng.lib, eng._h), _slots_pinned(eng.lib, eng._h)):
        assert rc == FE_ERR_UNSUPPORTED_CONFIG
        assert "the noncausal model has no streaming step" in _err()


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(T=0), dict(wav_in=NULL), dict(wav_out=NULL), dict(state=NULL)])
def test_step_pinned_checks_its_arguments(kw):
    eng = Engine(product_config("fe_b"), None)
    assert _pinned(eng.lib, eng._h, **kw) == FE_ERR_INVALID_ARG, kw
    assert "1 <= n <= capacity" in _err()


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=9), dict(cap=0), dict(T=0), dict(slots=NULL), dict(wav_in=NULL), dict(wav_out=NULL),
                                dict(state=NULL)])
def test_step_slots_pinned_checks_its_arguments(kw):
    eng = Engine(product_config("fe_b"), None)
    assert _slots_pinned(eng.lib, eng._h, **kw) == FE_ERR_INVALID_ARG, kw
    assert "1 <= n <= capacity" in _err()


def test_pinned_strides_are_checked():
    eng = Engine(product_config("fe_b"), None)            # hop 256
    for fn in (_pinned, _slots_pinned):
        assert fn(eng.lib, eng._h, in_stride=255) == FE_ERR_INVALID_ARG
        assert "in_stride 255 < T*H" in _err()
        assert fn(eng.lib, eng._h, in_stride=512, out_stride=511, T=2) == FE_ERR_INVALID_ARG
        assert "out_stride 511 < T*H" in _err()


def test_valid_arguments_reach_the_weights_check():
    """strides and counts that pass get as far as the handle's readiness (no weights here) - no pointer is looked at before that"""
    eng = Engine(product_config("fe_b"), None)
    assert _pinned(eng.lib, eng._h, B=1, in_stride=0, out_stride=0) == FE_ERR_NO_WEIGHTS          # (one row: its stride is not used)
    assert "fe_load_weights" in _err()
    assert _slots_pinned(eng.lib, eng._h, in_stride=300, out_stride=1024) == FE_ERR_NO_WEIGHTS
    assert "fe_load_weights" in _err()


def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


def _not_host(rows, cols):
    """a tensor that is not in host memory (meta: no storage at all; a CUDA tensor takes the same branch on the GPU machines)"""
    return torch.empty(rows, cols, device="meta")


@pytest.mark.parametrize("bad", ["pageable", "device"])
def test_engine_pinned_steps_refuse_unpinned_audio_before_any_native_call(monkeypatch, bad):
    eng = Engine(product_config("fe_b"), None)
    _no_native(monkeypatch, eng)
    x = torch.zeros(3, 256) if bad == "pageable" else _not_host(3, 256)
    match = "page-locked"
    with pytest.raises(ValueError, match=match):
        eng.step_pinned(x, torch.zeros(1))
    with pytest.raises(ValueError, match=match):
        eng.step_slots_pinned(x, torch.zeros(1), 8, [0, 1, 2])


def test_engine_pinned_steps_refuse_an_unpinned_output(monkeypatch):
    """the input is checked first; a pinned input cannot be made here (no GPU), so the output check is reached through a stand-in
    that reports itself pinned"""
    eng = Engine(product_config("fe_b"), None)
    _no_native(monkeypatch, eng)

    class PinnedLooking(torch.Tensor):
        def is_pinned(self, *a, **k):
            return True
    x = torch.zeros(3, 256).as_subclass(PinnedLooking)
    for y in (torch.zeros(3, 256), _not_host(3, 256)):
        with pytest.raises(ValueError, match="wav_out"):
            eng.step_pinned(x, torch.zeros(1), wav_out=y)
        with pytest.raises(ValueError, match="wav_out"):
            eng.step_slots_pinned(x, torch.zeros(1), 8, [0, 1, 2], wav_out=y)
    with pytest.raises(ValueError, match=r"float32 \[3, 512\]"):
        eng.step_pinned(x, torch.zeros(1), T=2)                    # (rows of T*H samples)


class _StubEngine:
    """what StreamPool needs of an Engine, recorded instead of run"""
    def __init__(self):
        self.calls = []

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        self.calls.append(("reset", capacity, list(slots)))

    def step_slots_pinned(self, wav_in, state, capacity, slots, wav_out=None, T=1):
        self.calls.append(("step_pinned", capacity, list(slots), T))
        return wav_in


def test_stream_pool_step_host_refuses_closed_slots_and_forwards():
    eng = _StubEngine()
    pool = StreamPool(eng, 4)
    a, b = pool.open(), pool.open()
    x = torch.zeros(2, 4)
    assert pool.step_host([b, a], x, T=2) is x
    assert eng.calls[-1] == ("step_pinned", 4, [b, a], 2)
    pool.close(a)
    with pytest.raises(ValueError, match=f"slot {a} is not open"):
        pool.step_host([b, a], x)
    assert eng.calls[-1][2] == [b, a] and len(eng.calls) == 3       # (refused before any engine call)


def test_stream_pool_step_host_refuses_unpinned_audio(monkeypatch):
    eng = Engine(product_config("fe_b"), None)
    pool = StreamPool.__new__(StreamPool)          # (no state buffer without a GPU: the pool's bookkeeping only)
    pool.engine, pool.capacity, pool.state, pool._free, pool._open = eng, 4, torch.zeros(1), [], {0, 1}
    _no_native(monkeypatch, eng)
    for x in (torch.zeros(2, 256), _not_host(2, 256)):
        with pytest.raises(ValueError, match="page-locked"):
            pool.step_host([1, 0], x)
