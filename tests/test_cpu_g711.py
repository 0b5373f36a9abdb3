"""CPU tests of G.711 (FE_AUDIO_ULAW / FE_AUDIO_ALAW) in the resampler: the numpy oracle's own checks, fastenhancer_amd.g711 against the
oracle on every byte and every sample, the C ABI's acceptance and refusals before any device work, the argument checks of
Resampler's in_format= / out_format=, and client_format= of the two resampled pools with the engine and the resamplers recorded instead of
run (the stand-ins of test_cpu_ring_resample.py)."""
import re
from ctypes import c_void_p
from pathlib import Path

import numpy as np
import pytest
import torch

import g711_oracle as go
import test_cpu_ring_resample as crr
from common import hip_engine
from fastenhancer_amd import _lib, g711
from fastenhancer_amd.resample import Resampler
from fastenhancer_amd.serving import ResampledPacketPool, RingResampledPacketPool

FE_ERR_INVALID_ARG = -1
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
PINNED_TEXT = "neither FE_AUDIO_F32 (0) nor FE_AUDIO_S16 (1)"
STREAM_FNS = ("fe_resample_streams", "fe_resample_streams_pinned", "fe_resample_rings", "fe_resample_rings_pinned")
LAW_CODE = {"ulaw": 4, "alaw": 5}


def _err():
    return _lib.load().fe_last_error().decode()


# ------------------------------------------------------------------ the contract
def test_the_oracle_meets_the_contract():
    """the four tables' digests, the anchors, enc(dec(b)) == b, dec(enc(q)) non-decreasing, the round-trip error; audioop where it imports"""
    go.check_contract()


@pytest.mark.parametrize("law", go.LAWS)
def test_the_package_module_equals_the_oracle_on_every_byte_and_every_sample(law):
    d = g711.decode(torch.from_numpy(go.ALL_BYTES.copy()), law)
    assert d.dtype == torch.int16 and d.numpy().tolist() == go.dec_table(law).tolist()
    e = g711.encode(torch.from_numpy(go.ALL_SAMPLES.copy()), law)
    assert e.dtype == torch.uint8 and e.numpy().tolist() == go.enc_table(law).tolist()
    x = torch.from_numpy(go.ALL_SAMPLES.copy()).view(256, 256)            # any shape
    assert g711.encode(x, law).shape == x.shape and torch.equal(g711.encode(x, law).view(-1), e)
    with pytest.raises(ValueError, match="'ulaw' or 'alaw'"):
        g711.decode(torch.zeros(4, dtype=torch.uint8), "g722")
    with pytest.raises(ValueError, match="uint8"):
        g711.decode(torch.zeros(4, dtype=torch.int16), law)
    with pytest.raises(ValueError, match="int16"):
        g711.encode(torch.zeros(4, dtype=torch.uint8), law)


def test_the_header_defines_the_two_formats_and_the_binding_has_them():
    text = HEADER.read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(FE_AUDIO_\w+)\s+(\d+)", text)}
    assert defs == {"FE_AUDIO_F32": 0, "FE_AUDIO_S16": 1, "FE_AUDIO_ULAW": 4, "FE_AUDIO_ALAW": 5}
    assert (_lib.FE_AUDIO_ULAW, _lib.FE_AUDIO_ALAW) == (4, 5) and (_lib.FE_AUDIO_F32, _lib.FE_AUDIO_S16) == (0, 1)


# ------------------------------------------------------------------ the C ABI: accepted by the resampler, refused by the model steps
def _whole(lib, rs, in_dev=P, in_stride=100, in_format=0, n_in=100, out_dev=P, out_stride=34, out_format=0, B=1):
    return lib.fe_resample(rs, in_dev, in_stride, in_format, n_in, out_dev, out_stride, out_format, B, NULL)


def _streams(lib, fn, rs, x=P, in_count=1024, in_format=1, state=P, capacity=4, desc=P, out=P, out_count=1024, out_format=1, produced=NULL, n=1,
             n_in_max=960):
    return getattr(lib, fn)(rs, x, in_count, in_format, state, capacity, desc, out, out_count, out_format, produced, n, n_in_max, NULL)


FORMAT_PAIRS = [(4, 4), (5, 5), (4, 5), (4, 0), (5, 1), (0, 4), (1, 5)]          # each side on its own


@pytest.mark.parametrize("fmt_in,fmt_out", FORMAT_PAIRS)
def test_fe_resample_takes_the_two_formats_and_answers_with_the_other_arguments_error(fmt_in, fmt_out):
    lib, rs = _lib.load(), Resampler(48000, 16000)
    kw = dict(in_format=fmt_in, out_format=fmt_out)
    assert _whole(lib, rs._h, n_in=0, **kw) == FE_ERR_INVALID_ARG and "fe_resample: bad argument" in _err()
    # the checks BEHIND the format check answer: the formats passed it
    assert _whole(lib, rs._h, out_stride=33, **kw) == FE_ERR_INVALID_ARG and "strides" in _err() and "FE_AUDIO" not in _err()
    assert _whole(lib, rs._h, B=70000, **kw) == FE_ERR_INVALID_ARG and "grid" in _err()
    assert rs.last_kernel() == ""


@pytest.mark.parametrize("fn", STREAM_FNS)
@pytest.mark.parametrize("fmt_in,fmt_out", FORMAT_PAIRS)
def test_the_stream_and_ring_entry_points_take_the_two_formats(fn, fmt_in, fmt_out):
    lib, down, up = _lib.load(), Resampler(48000, 16000), Resampler(16000, 48000)
    kw = dict(in_format=fmt_in, out_format=fmt_out)
    for bad in (dict(n_in_max=0), dict(n=0), dict(out=NULL)):
        assert _streams(lib, fn, down._h, **bad, **kw) == FE_ERR_INVALID_ARG and fn + ": bad argument" in _err(), bad
    # behind the format check: the table `produced`
    assert _streams(lib, fn, up._h, n_in_max=2 ** 31 - 1, **kw) == FE_ERR_INVALID_ARG and "produced" in _err() and "FE_AUDIO" not in _err()
    assert down.last_kernel() == up.last_kernel() == ""


@pytest.mark.parametrize("fn", ["fe_resample_streams_pinned", "fe_resample_rings_pinned"])
def test_the_pinned_twins_look_a_byte_buffer_up_and_refuse_pageable_memory(fn):
    lib, rs = _lib.load(), Resampler(8000, 16000)
    x = torch.zeros(1024, dtype=torch.uint8)
    rc = _streams(lib, fn, rs._h, x=c_void_p(x.data_ptr()), out=c_void_p(x.data_ptr()), in_format=4, out_format=5)
    assert rc == FE_ERR_INVALID_ARG and fn + ": in is not page-locked host memory" in _err()


@pytest.mark.parametrize("fmt", [2, 3, 16, -1])
def test_the_other_codes_stay_invalid_in_the_pinned_words(fmt):
    lib, rs = _lib.load(), Resampler(48000, 16000)
    for side in ("in_format", "out_format"):
        assert _whole(lib, rs._h, **{side: fmt}) == FE_ERR_INVALID_ARG and PINNED_TEXT in _err() and f"{side} {fmt} is" in _err()
        for fn in STREAM_FNS:
            assert _streams(lib, fn, rs._h, **{side: fmt}) == FE_ERR_INVALID_ARG and PINNED_TEXT in _err() and f"{fn}: {side} {fmt} is" in _err()
        # a G.711 law on the other side does not let it through
        other = "out_format" if side == "in_format" else "in_format"
        assert _whole(lib, rs._h, **{side: fmt, other: 4}) == FE_ERR_INVALID_ARG and PINNED_TEXT in _err()


@pytest.mark.parametrize("fn", ["fe_step_streams", "fe_step_streams_pinned", "fe_step_pool_streams", "fe_step_pool_streams_pinned"])
@pytest.mark.parametrize("fmt", [4, 5])
def test_the_model_steps_keep_refusing_the_two_codes(fn, fmt):
    """... with the message they give for format 2"""
    eng = hip_engine("fspen" if "pool" in fn else "fe_b")

    def call(f):
        return getattr(eng.lib, fn)(eng._h, P, 1024, P, 4, P, P, 1024, 1, 1, f, NULL)
    assert call(2) == FE_ERR_INVALID_ARG
    want = _err()
    assert f"{fn}: format 2 is {PINNED_TEXT}" == want
    assert call(fmt) == FE_ERR_INVALID_ARG and _err() == want.replace("format 2", f"format {fmt}")


# ------------------------------------------------------------------ Resampler: in_format= / out_format=
def test_resampler_keywords_are_checked_before_any_native_call(monkeypatch):
    rs = Resampler(8000, 16000)
    called = []
    for name in STREAM_FNS + ("fe_resample",):
        monkeypatch.setattr(rs.lib, name, lambda *a, _n=name: called.append(_n) or 0)
    st = torch.zeros(4, rs.state_floats)
    for pinned, rings, call in ((False, False, rs.step_streams), (True, False, rs.step_streams_pinned), (False, True, rs.step_rings),
                                (True, True, rs.step_rings_pinned)):
        cls = crr._Pinned if pinned else crr._Dev
        u8, s16 = torch.zeros(1024, dtype=torch.uint8).as_subclass(cls), torch.zeros(1024, dtype=torch.int16).as_subclass(cls)
        desc = [(0, 10, 0, 0, 1024, 0, 1024, 0)] if rings else [(0, 10, 0, 0)]
        # uint8 without a keyword: the message of before
        with pytest.raises(ValueError, match="x must be a contiguous, non-empty float32 or int16 tensor"):
            call(u8, st, 4, desc, s16, 960)
        with pytest.raises(ValueError, match="out must be a contiguous, non-empty float32 or int16 tensor"):
            call(s16, st, 4, desc, u8, 960)
        # a law wants uint8 on its side, and names the law and the dtype
        with pytest.raises(ValueError, match="x: G.711 ulaw .* torch.uint8, got torch.int16"):
            call(s16, st, 4, desc, s16, 960, in_format="ulaw")
        with pytest.raises(ValueError, match="out: G.711 alaw .* torch.uint8, got torch.int16"):
            call(u8, st, 4, desc, s16, 960, in_format="ulaw", out_format="alaw")
        with pytest.raises(ValueError, match="x must be a contiguous, non-empty float32 or int16 tensor"):
            call(u8, st, 4, desc, u8, 960, out_format="alaw")            # the law of one side says nothing about the other
        for kw in (dict(in_format="g722"), dict(out_format="s16"), dict(in_format=4)):
            with pytest.raises(ValueError, match="must be None, 'ulaw' or 'alaw'"):
                call(u8, st, 4, desc, u8, 960, **kw)
        with pytest.raises(TypeError):                                     # keyword-only
            call(u8, st, 4, desc, u8, 960, None, "ulaw", "alaw")
        # the other checks are those of before, and a valid call gets as far as the device requirement
        with pytest.raises(ValueError, match="page-locked" if pinned else "device tensor"):
            call(torch.zeros(1024, dtype=torch.uint8), st, 4, desc, u8, 960, in_format="ulaw", out_format="alaw")
        for kw in (dict(in_format="ulaw", out_format="alaw"), dict(in_format="alaw", out_format="ulaw")):
            with pytest.raises(_lib.FEError, match="needs a GPU"):
                call(u8, st, 4, desc, u8, 960, **kw)
        with pytest.raises(_lib.FEError, match="needs a GPU"):
            call(u8, st, 4, desc, s16, 960, in_format="alaw")
    # whole signals
    u8 = torch.zeros(2, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="x must be a non-empty float32 or int16 tensor"):
        rs(u8)
    with pytest.raises(ValueError, match="x: G.711 alaw .* torch.uint8, got torch.int16"):
        rs(torch.zeros(2, 8, dtype=torch.int16), in_format="alaw")
    with pytest.raises(ValueError, match="must be None, 'ulaw' or 'alaw'"):
        rs(u8, in_format="mulaw")
    with pytest.raises(ValueError, match="out_dtype must be float32 or int16"):
        rs(u8, torch.uint8, in_format="ulaw")
    with pytest.raises(ValueError, match="leave out_dtype alone"):
        rs(torch.zeros(2, 8), torch.int16, out_format="ulaw")
    for args, kw in (((u8,), dict(in_format="ulaw")), ((u8, torch.float32), dict(in_format="alaw")), ((torch.zeros(2, 8),), dict(out_format="ulaw")),
                     ((u8,), dict(in_format="ulaw", out_format="alaw"))):
        with pytest.raises(_lib.FEError, match="needs a GPU"):
            rs(*args, **kw)
    assert called == []


# ------------------------------------------------------------------ the pools: client_format=
class _LawResampler(crr._StubResampler):
    """test_cpu_ring_resample's stand-in, which also takes and records the two keywords and what the buffers were"""
    def __init__(self, log, sr_in, sr_out):
        super().__init__(log, sr_in, sr_out)
        self.formats = []

    def _emit(self, state, slot, n):
        made, y = super()._emit(state, slot, n)
        return made, y.to(self.formats[-1][3])                      # (samples in the output buffer's type: bytes under a law)

    def step_streams_pinned(self, x, state, capacity, desc, out, n_in_max, produced=None, *, in_format=None, out_format=None):
        self.formats.append((in_format, out_format, x.dtype, out.dtype))
        return super().step_streams_pinned(x, state, capacity, desc, out, n_in_max, produced=produced)

    def step_rings_pinned(self, x, state, capacity, desc, out, n_in_max, produced=None, *, in_format=None, out_format=None):
        self.formats.append((in_format, out_format, x.dtype, out.dtype))
        return super().step_rings_pinned(x, state, capacity, desc, out, n_in_max, produced=produced)


def _pool(monkeypatch, cls, client_format=None, stub=_LawResampler, **kw):
    log = []
    monkeypatch.setattr(cls, "_make_resampler", staticmethod(lambda a, b, device: stub(log, a, b)))
    if client_format is not None:
        kw["client_format"] = client_format
    return cls(crr._StubEngine(log), capacity=3, ring_hops=4, client_rate=8000, T_max=2, max_packet=256, **kw)


@pytest.mark.parametrize("law", go.LAWS)
@pytest.mark.parametrize("cls", [ResampledPacketPool, RingResampledPacketPool])
def test_a_law_pool_stages_bytes_and_passes_the_law_to_both_launches(monkeypatch, cls, law):
    pool = _pool(monkeypatch, cls, law)
    assert pool.client_format == law
    assert pool._cin.dtype == pool._cout.dtype == torch.uint8 and tuple(pool._cin.shape) == (3, 256)
    # the model-rate side is what it was
    assert pool.inner.ring_in.dtype == pool.inner.ring_out.dtype == torch.int16
    if cls is ResampledPacketPool:
        assert pool._min.dtype == pool._mout.dtype == torch.int16
    s = pool.open()
    empty = pool.pull(s)
    assert empty.dtype == torch.uint8 and empty.numel() == 0
    for bad in (torch.zeros(160, dtype=torch.int16), np.zeros(160, dtype=np.int16), torch.zeros(160), torch.zeros(2, 80, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=f"1-D uint8 array of G.711 {law} bytes"):
            pool.push(s, bad)
    assert pool._pending[s] == 0
    rng = np.random.default_rng(3)
    got = 0
    for tick in range(12):
        pool.push(s, rng.integers(0, 256, size=128, dtype=np.uint8))                    # arrays as well as tensors
        pool.push(s, torch.from_numpy(rng.integers(0, 256, size=128, dtype=np.uint8)))
        with pytest.raises(OverflowError, match="max_packet = 256"):
            pool.push(s, torch.zeros(1, dtype=torch.uint8))
        pool.tick()
        y = pool.pull(s)
        assert y.dtype == torch.uint8 and y.dim() == 1
        got += y.numel()
    assert got > 8 * 256
    # the law reached every launch, on the client's side only
    assert len(pool.to_model.formats) == 12 and set(pool.to_model.formats) == {(law, None, torch.uint8, torch.int16)}
    assert len(pool.to_client.formats) >= 10 and set(pool.to_client.formats) == {(None, law, torch.int16, torch.uint8)}


@pytest.mark.parametrize("cls", [ResampledPacketPool, RingResampledPacketPool])
def test_s16_is_the_default_and_the_calls_and_messages_of_before(monkeypatch, cls):
    for fmt in (None, "s16"):
        # (test_cpu_ring_resample's own stand-in takes no keyword: a call that passed one would be a TypeError)
        pool = _pool(monkeypatch, cls, fmt, stub=crr._StubResampler)
        assert pool.client_format == "s16" and pool._cin.dtype == pool._cout.dtype == torch.int16
        s = pool.open()
        assert pool.pull(s).dtype == torch.int16
        with pytest.raises(ValueError, match=r"a packet is a 1-D int16 array, got torch.uint8 \(160,\)"):
            pool.push(s, torch.zeros(160, dtype=torch.uint8))
        for _ in range(4):
            pool.push(s, torch.zeros(256, dtype=torch.int16))
            pool.tick()
        assert pool.pull(s).dtype == torch.int16
    for bad in ("g722", "f32", None, 4):
        with pytest.raises(ValueError, match="client_format must be 's16', 'ulaw' or 'alaw'"):
            cls(crr._StubEngine([]), 2, 2, 8000, client_format=bad)
    with pytest.raises(TypeError):                                         # keyword-only
        cls(crr._StubEngine([]), 2, 2, 8000, 1, None, 16000, "ulaw")


@pytest.mark.parametrize("law", go.LAWS)
def test_the_ring_law_pool_keeps_the_books_of_the_resampled_law_pool(monkeypatch, law):
    old, new = _pool(monkeypatch, ResampledPacketPool, law), _pool(monkeypatch, RingResampledPacketPool, law)
    rng = np.random.default_rng(5)
    for _ in range(3):
        assert old.open() == new.open()
    for tick in range(25):
        for slot in old.active:
            for _ in range(int(rng.integers(0, 3))):
                x = torch.from_numpy(rng.integers(0, 256, size=128, dtype=np.uint8))
                old.push(slot, x), new.push(slot, x)
        assert new.tick() == old.tick()
        for slot in old.active:
            a, b = old.pull(slot), new.pull(slot)
            assert a.dtype == b.dtype == torch.uint8 and torch.equal(a, b), (tick, slot)
        assert old._consumed == new._consumed and old._pending == new._pending and old._fill == new._fill
    assert torch.equal(old.state_in, new.state_in) and torch.equal(old.state_out, new.state_out) and sum(new._consumed) > 20 * 128
