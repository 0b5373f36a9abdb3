"""CPU tests of fe_step_pool_streams[_pinned] - the packet step for every family with a streaming state (fe_step_pool_streams*,
Engine.step_pool_streams*, family.packet_step and which packet step PacketPool.tick calls): the declarations, the argument checks that come
before any device work, and the pool's choice and refusals with the engine calls recorded instead of run."""
import re
from ctypes import c_void_p
from pathlib import Path

import pytest
import torch

from common import hip_engine, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.family import packet_step
from fastenhancer_amd.serving import PacketPool

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
TWINS = {"fe_step_pool_streams": "fe_step_streams", "fe_step_pool_streams_pinned": "fe_step_streams_pinned"}

# the argument table of tests/test_cpu_stream_packets.py (test_stream_entry_points_check_their_arguments), the formats included
BAD_ARGS = [dict(wav_in=NULL), dict(state=NULL), dict(desc=NULL), dict(wav_out=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0),
            dict(T_max=0), dict(T_max=-2), dict(in_count=0), dict(out_count=0), dict(fmt=2), dict(fmt=-1), dict(fmt=16)]


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, NULL)


# ------------------------------------------------------------------ the ABI
def test_the_header_declares_both_functions_and_the_binding_types_them_like_fe_step_streams():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(fe_step_(?:pool_)?streams(?:_pinned)?)\s*\(([^)]*)\)\s*;", text)}
    assert set(decls) == set(TWINS) | set(TWINS.values())
    lib = _lib.load()
    for fn, twin in TWINS.items():
        assert decls[fn] == decls[twin]                                              # the same parameter list, word for word
        assert _lib.SYMBOLS[fn] == _lib.SYMBOLS[twin]
        assert getattr(lib, fn).argtypes == getattr(lib, twin).argtypes and getattr(lib, fn).restype == getattr(lib, twin).restype


@pytest.mark.parametrize("fn", TWINS)
def test_pool_streams_refuses_a_null_handle(fn):
    lib = _lib.load()
    assert _call(lib, fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("fn", TWINS)
@pytest.mark.parametrize("name", ["fe_b", "bsrnn_xxt", "fspen", "lisennet"])
def test_pool_streams_answers_every_bad_call_as_fe_step_streams_does(name, fn):
    """code and wording of fe_step_streams[_pinned] on a FastEnhancer handle in the same condition, under the new function's name (the last
    call is a good one: these handles have no weights, and that refusal is the same too)"""
    ref, eng = hip_engine("fe_b"), hip_engine(name)
    assert ref.cfg.hop_size == eng.cfg.hop_size == 256
    for kw in BAD_ARGS + [dict()]:
        code, text = _call(ref.lib, TWINS[fn], ref._h, **kw), _err()
        assert code != 0
        if kw:
            assert code == FE_ERR_INVALID_ARG and TWINS[fn] + ":" in text, (kw, text)
        want = (code, text.replace(TWINS[fn] + ":", fn + ":"))
        got = (_call(eng.lib, fn, eng._h, **kw), _err())
        assert got == want, (kw, got, want)


@pytest.mark.parametrize("fn", TWINS)
def test_pool_streams_refuses_the_noncausal_model_as_fe_step_does(fn):
    eng = hip_engine("fe_nc")
    assert _call(eng.lib, fn, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err() and "use fe_offline" in _err()


@pytest.mark.parametrize("fn", TWINS.values())
def test_fe_step_streams_itself_still_refuses_a_bsrnn_handle(fn):
    eng = hip_engine("bsrnn_xxt")
    assert _call(eng.lib, fn, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "FastEnhancer family" in _err() and fn in _err()


# ------------------------------------------------------------------ Engine.step_pool_streams*: step_streams' host checks
def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


class _Pinned(torch.Tensor):
    """a CPU tensor that passes for page-locked memory (no CPU-only process can pin one): the buffer checks let it through to the descriptors'"""
    def is_pinned(self, *a, **kw):
        return True


class _Dev(torch.Tensor):
    """... and one that passes for a device tensor"""
    is_cuda = property(lambda self: True)


def _same_refusal(ref_call, new_call, fix=lambda s: s):
    with pytest.raises(ValueError) as want:
        ref_call()
    with pytest.raises(ValueError) as got:
        new_call()
    assert str(got.value) == fix(str(want.value))


@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen", "lisennet"])
def test_step_pool_streams_checks_descriptors_and_buffers_as_step_streams_does(monkeypatch, name):
    """one code path (_step_streams): the same exception for the same call, and nothing reaches the library"""
    ref, eng = hip_engine("fe_b"), hip_engine(name)
    _no_native(monkeypatch, ref)
    _no_native(monkeypatch, eng)
    f, s, st = torch.zeros(1024), torch.zeros(1024, dtype=torch.int16), torch.zeros(1)
    pf, ps = f.clone(), s.clone()
    bad_desc = [[(0, 1, 0, 0), (0, 1, 256, 256)],        # duplicate slot
                [(8, 1, 0, 0)], [(-1, 1, 0, 0)],         # slot outside
                [(0, 3, 0, 0)], [(0, -1, 0, 0)],         # hops outside [0, T_max]
                [(0, 2, 513, 0)], [(0, 1, -1, 0)], [(0, 2, 0, 600)],      # ranges outside
                [], torch.zeros(2, 4, dtype=torch.int32)]
    for pinned in (False, True):
        old = ref.step_streams_pinned if pinned else ref.step_streams
        new = eng.step_pool_streams_pinned if pinned else eng.step_pool_streams
        a = torch.zeros(1024, dtype=torch.int16).as_subclass(_Pinned if pinned else _Dev)      # audio that passes the buffer checks
        for desc in bad_desc:
            _same_refusal(lambda: old(a, st, 8, desc, a, T_max=2), lambda: new(a, st, 8, desc, a, T_max=2))
        ok = [(0, 1, 0, 0)]
        with pytest.raises(_lib.FEError, match="needs a GPU"):         # a valid call gets as far as the device requirement
            new(a, st, 8, ok, a, T_max=2)
        _same_refusal(lambda: old(f, st, 8, ok, s), lambda: new(f, st, 8, ok, s))                                        # dtype mix
        _same_refusal(lambda: old(torch.zeros(4, dtype=torch.float64), st, 8, ok, f), lambda: new(torch.zeros(4, dtype=torch.float64), st, 8, ok, f))
        _same_refusal(lambda: old(f, st, 8, ok, f), lambda: new(f, st, 8, ok, f),                                        # unpinned / not on the device
                      fix=lambda t: t.replace("fe_step_streams_pinned", "fe_step_pool_streams_pinned"))
        _same_refusal(lambda: old(s, st, 8, ok, s, T_max=0), lambda: new(s, st, 8, ok, s, T_max=0),
                      fix=lambda t: t.replace("fe_step_streams_pinned", "fe_step_pool_streams_pinned"))
    with pytest.raises(ValueError, match="page-locked"):
        eng.step_pool_streams_pinned(ps, st, 8, [(0, 1, 0, 0)], ps)
    with pytest.raises(ValueError, match="must be a device tensor"):
        eng.step_pool_streams(pf, st, 8, [(0, 1, 0, 0)], pf)


@pytest.mark.parametrize("name", ["fe_b", "bsrnn_xxt", "fspen", "lisennet"])
@pytest.mark.parametrize("kw", [dict(min_gain=torch.zeros(8)), dict(levels=torch.zeros(8, 4)), dict(bank=torch.zeros(8, dtype=torch.int32)),
                                dict(chunk=True), dict(min_gain=torch.zeros(8), bank=torch.zeros(8, dtype=torch.int32))])
def test_step_pool_streams_takes_no_controls_banks_or_chunk(monkeypatch, name, kw):
    eng = hip_engine(name)
    _no_native(monkeypatch, eng)
    s = torch.zeros(1024, dtype=torch.int16)
    for call in (eng.step_pool_streams, eng.step_pool_streams_pinned):
        with pytest.raises(ValueError, match=" / ".join(kw)):
            call(s, torch.zeros(1), 8, [(0, 1, 0, 0)], s, **kw)


# ------------------------------------------------------------------ PacketPool with the engine calls recorded
class _Cfg:
    hop_size = 256


class _StubEngine:
    """what PacketPool needs of an Engine, recorded instead of run"""
    def __init__(self, cfg=None):
        self.cfg = cfg if cfg is not None else _Cfg()
        self.calls = []

    def new_state(self, B):
        self.calls.append(("new_state", B))
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        self.calls.append(("reset", capacity, list(slots)))

    def new_pinned(self, *shape, dtype=torch.float32):
        self.calls.append(("new_pinned",) + tuple(shape))
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        pass

    def _packets(self, call, wav_in, state, capacity, desc, wav_out, T_max, kw):
        assert wav_in.dtype == wav_out.dtype == torch.int16 and not kw
        self.calls.append((call, capacity, list(desc), T_max))
        return wav_out

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, **kw):
        return self._packets("step_streams_pinned", wav_in, state, capacity, desc, wav_out, T_max, kw)

    def step_pool_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, **kw):
        return self._packets("step_pool_streams_pinned", wav_in, state, capacity, desc, wav_out, T_max, kw)

    def step_streams(self, *a, **kw):
        raise AssertionError("the device-audio step is not a PacketPool's")

    step_pool_streams = step_streams


@pytest.mark.parametrize("name,call", [("bsrnn_xxt", "step_pool_streams_pinned"), ("bsrnn_s", "step_pool_streams_pinned"),
                                       ("fspen", "step_pool_streams_pinned"), ("lisennet", "step_pool_streams_pinned"),
                                       ("fe_b", "step_streams_pinned"), ("fe_dpt_t", "step_streams_pinned"), (None, "step_streams_pinned")])
def test_packet_pool_tick_calls_the_familys_packet_step(name, call):
    eng = _StubEngine(product_config(name) if name else None)
    assert packet_step(eng, pinned=True) == getattr(eng, call)
    assert packet_step(eng, pinned=False) == getattr(eng, call[:-len("_pinned")])
    H = eng.cfg.hop_size
    pool = PacketPool(eng, 4, ring_hops=4, T_max=2)
    a, b, c = pool.open(), pool.open(), pool.open()
    del eng.calls[:]
    pool.push(a, torch.zeros(H - 1, dtype=torch.int16))               # no complete hop
    pool.push(b, torch.zeros(H, dtype=torch.int16))                   # one
    pool.push(c, torch.zeros(3 * H + 5, dtype=torch.int16))           # three: T_max caps the launch at two
    R = 4 * H
    want = [(b, 1, b * R, b * R), (c, 2, c * R, c * R)]               # the descriptors tick documents: (slot, hops, in_offset, out_offset), 0-hop streams left out
    assert pool.tick() == want
    assert eng.calls == [(call, 4, want, 2)]
    assert pool.tick() == [(c, 1, c * R + 2 * H, c * R + 2 * H)]
    assert pool.tick() == [] and len(eng.calls) == 2                  # no hop: no launch
    assert pool.pull(b).numel() == H and pool.pull(c).numel() == 3 * H and pool.pull(a).numel() == 0


@pytest.mark.parametrize("name,family", [("bsrnn_xxt", "BSRNN"), ("bsrnn_s", "BSRNN"), ("fspen", "FSPEN"), ("lisennet", "LiSenNet")])
def test_a_baseline_packet_pool_refuses_the_fastenhancer_controls_before_any_engine_call(name, family):
    eng = _StubEngine(product_config(name))
    with pytest.raises(ValueError, match=family):
        PacketPool(eng, 4, ring_hops=4, meters=True)
    with pytest.raises(ValueError, match=family):
        PacketPool(eng, 4, ring_hops=16, T_max=1, backlog_hops=8)
    assert eng.calls == []
    pool = PacketPool(eng, 4, ring_hops=4)
    s = pool.open()
    del eng.calls[:]
    with pytest.raises(ValueError, match=family):
        pool.set_suppression_limit(s, -20.0)
    with pytest.raises(ValueError, match=family):
        pool.set_bank(s, 1)
    with pytest.raises(ValueError, match=family):
        pool.open(bank=1)
    assert eng.calls == [] and pool.active == [s]                     # (no slot was opened either)
    pool.set_suppression_limit(s, None)                               # lifting a limit, bank 0: what every stream has
    pool.set_bank(s, 0)
    assert pool.suppression_limit(s) is None and pool.bank(s) == 0
    assert pool.open(bank=0) != s
    assert [c[0] for c in eng.calls] == ["reset"]


def test_a_fastenhancer_packet_pool_keeps_its_controls():
    eng = _StubEngine(product_config("fe_b"))
    pool = PacketPool(eng, 4, ring_hops=16, T_max=1, meters=True, backlog_hops=8)
    s = pool.open()
    pool.set_suppression_limit(s, -20.0)
    assert abs(pool.suppression_limit(s) + 20.0) < 1e-5
