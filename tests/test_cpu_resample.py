"""CPU tests of the polyphase resampler (fe_resampler_*, fe_resample, fe_resample_streams[_pinned], fastenhancer_amd.resample.Resampler,
serving.ResampledPacketPool, the callers' --resample): the filter and the float64 oracle against scipy, the output counts against brute
force, the declarations, the refusals that come before any device work, and the pool's order of calls with its engine and resamplers
recorded instead of run."""
import re
from ctypes import c_void_p, byref
from pathlib import Path

import numpy as np
import pytest
import torch

import resample_oracle as ro
from fastenhancer_amd import _lib
from fastenhancer_amd.resample import Resampler
from fastenhancer_amd.serving import ResampledPacketPool

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
COUNTS = list(range(200)) + [997, 4096]


def _err():
    return _lib.load().fe_last_error().decode()


# ------------------------------------------------------------------ the filter and the oracle
@pytest.mark.parametrize("sr_in,sr_out", ro.PAIRS)
def test_taps_are_up_times_firwin(sr_in, sr_out):
    """1e-12: double arithmetic gives ~1e-16, fp32 tap resolution is ~1e-7 - the margin cannot hide a wrong tap"""
    from scipy.signal import firwin
    rs = Resampler(sr_in, sr_out)
    up, down = ro.ratio(sr_in, sr_out)
    R = max(up, down)
    assert (rs.up, rs.down, rs.half_len, rs.taps_per_output) == (up, down, 10 * R, ro.taps_per_output(up, down))
    want = up * firwin(20 * R + 1, 1.0 / R, window=("kaiser", 5.0))
    assert np.abs(rs.taps().numpy() - want).max() <= 1e-12
    assert np.abs(ro.taps(up, down) - want).max() <= 1e-12
    assert rs.latency_samples == 10 * R / up


@pytest.mark.parametrize("sr_in,sr_out", ro.PAIRS)
def test_the_oracle_is_resample_poly(sr_in, sr_out):
    from scipy.signal import resample_poly
    up, down = ro.ratio(sr_in, sr_out)
    rng = np.random.default_rng(5)
    for n in (1, ro.taps_per_output(up, down), 997):
        x = rng.standard_normal((2, n))
        want = resample_poly(x, up, down, axis=-1)
        got = ro.resample(x, up, down)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("sr_in,sr_out", ro.PAIRS)
def test_output_counts_against_brute_force(sr_in, sr_out):
    rs = Resampler(sr_in, sr_out)
    up, down = ro.ratio(sr_in, sr_out)
    for n in COUNTS:
        assert rs.out_count(n) == -(-n * up // down)
        assert rs.produced(0, n) == ro.emitted(n, up, down) == ro.emitted_brute(n, up, down), n
    # produced summed over any packetisation is M(total)
    rng = np.random.default_rng(up * 1000 + down)
    for _ in range(3):
        sizes = rng.integers(0, 500, size=40)
        total, made = 0, 0
        for s in sizes:
            made += rs.produced(total, int(s))
            total += int(s)
        assert made == ro.emitted(total, up, down)
    assert rs.out_count(-1) == -1 and rs.produced(-1, 5) == -1 and rs.produced(5, -1) == -1


def test_the_stated_latencies_and_the_error_bound_of_48_to_16():
    assert Resampler(48000, 16000).latency_samples == 30 and Resampler(8000, 16000).latency_samples == 10
    assert 6.0e-6 < ro.error_bound(1, 3, 1.0) < 6.8e-6


def test_state_row_layout():
    for sr_in, sr_out in ro.PAIRS:
        rs = Resampler(sr_in, sr_out)
        assert rs.state_floats == -(-(rs.taps_per_output - 1 + 2) // 4) * 4


# ------------------------------------------------------------------ the ABI
NAMES = ["fe_resampler_create", "fe_resampler_destroy", "fe_resampler_up", "fe_resampler_down", "fe_resampler_taps_per_output", "fe_resampler_half_len",
         "fe_resampler_taps", "fe_resampler_out_count", "fe_resampler_produced", "fe_resampler_state_floats", "fe_resampler_last_kernel", "fe_resample",
         "fe_resample_streams", "fe_resample_streams_pinned"]


def test_the_header_declares_every_function_and_the_binding_types_it():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(fe_resample_streams(?:_pinned)?)\s*\(([^)]*)\)\s*;", text)}
    assert set(decl) == {"fe_resample_streams", "fe_resample_streams_pinned"} and len(set(decl.values())) == 1     # the same parameter list
    assert _lib.SYMBOLS["fe_resample_streams"] == _lib.SYMBOLS["fe_resample_streams_pinned"]
    assert re.search(r"typedef struct fe_resample_desc\s*\{[^}]*int slot, n_in;\s*long long in_offset, out_offset;\s*\}", text)
    import ctypes
    assert ctypes.sizeof(_lib.fe_resample_desc) == 24
    assert Resampler.pack_desc([(3, 7, 1 << 33, 5)]).tolist() == [[3, 7, 0, 2, 5, 0]]


def test_create_refusals():
    lib, h = _lib.load(), c_void_p()
    for a, b in ((0, 16000), (16000, 0), (-8000, 16000), (16000, -1), (16000, 16000)):
        assert lib.fe_resampler_create(a, b, byref(h)) == FE_ERR_INVALID_ARG and not h.value
    assert "equal rates" in _err()
    assert lib.fe_resampler_create(48000, 16000, None) == FE_ERR_INVALID_ARG
    assert lib.fe_resampler_create(48000, 16001, byref(h)) == FE_ERR_UNSUPPORTED_CONFIG and not h.value
    assert "16001 / 48000" in _err() and "640" in _err()           # the message names the reduced ratio
    assert lib.fe_resampler_create(1000, 641, byref(h)) == FE_ERR_UNSUPPORTED_CONFIG and "641 / 1000" in _err()
    with pytest.raises(_lib.FEError, match="equal rates"):
        Resampler(16000, 16000)


def test_every_pair_of_the_usual_rates_fits_but_one():
    """max(up, down) <= 640 holds for every pair of the usual rates except 11.025 <-> 32 kHz, which reduces to 441 / 1280"""
    for a in RATES:
        for b in RATES:
            if a != b and {a, b} != {11025, 32000}:
                rs = Resampler(a, b)
                assert max(rs.up, rs.down) <= 640
    for a, b, ratio in ((11025, 32000, "1280 / 441"), (32000, 11025, "441 / 1280")):
        with pytest.raises(_lib.FEError, match=ratio):
            Resampler(a, b)
    rs = Resampler(48000, 11025)
    assert (rs.up, rs.down, rs.half_len, rs.taps_per_output) == (147, 640, 6400, 88)


def test_queries_on_a_null_handle_and_the_taps_buffer():
    lib = _lib.load()
    assert lib.fe_resampler_up(NULL) == 0 and lib.fe_resampler_state_floats(NULL) == 0 and lib.fe_resampler_out_count(NULL, 5) == -1
    assert lib.fe_resampler_last_kernel(NULL) == b""
    assert lib.fe_resampler_taps(NULL, None, 0) == FE_ERR_INVALID_ARG
    rs = Resampler(48000, 16000)
    assert rs.last_kernel() == ""
    assert lib.fe_resampler_taps(rs._h, None, 0) == 61
    buf = (_lib.c_double * 60)()
    assert lib.fe_resampler_taps(rs._h, buf, 60) == FE_ERR_INVALID_ARG and "61" in _err() and not any(buf)
    lib.fe_resampler_destroy(NULL)


def _whole(lib, rs, in_dev=P, in_stride=100, in_format=0, n_in=100, out_dev=P, out_stride=34, out_format=0, B=1):
    return lib.fe_resample(rs, in_dev, in_stride, in_format, n_in, out_dev, out_stride, out_format, B, NULL)


def test_fe_resample_checks_its_arguments_before_any_device_work():
    lib, rs = _lib.load(), Resampler(48000, 16000)
    assert _whole(lib, NULL) == FE_ERR_INVALID_ARG and "null resampler" in _err()
    for kw in (dict(in_dev=NULL), dict(out_dev=NULL), dict(B=0), dict(B=-1), dict(n_in=0), dict(n_in=-5)):
        assert _whole(lib, rs._h, **kw) == FE_ERR_INVALID_ARG and "fe_resample: bad argument" in _err(), kw
    for kw in (dict(in_format=2), dict(in_format=-1), dict(out_format=2), dict(out_format=16)):
        assert _whole(lib, rs._h, **kw) == FE_ERR_INVALID_ARG and "neither FE_AUDIO_F32 (0) nor FE_AUDIO_S16 (1)" in _err(), kw
    assert "out_format 16" in _err()
    for kw in (dict(in_stride=99), dict(out_stride=33)):
        assert _whole(lib, rs._h, **kw) == FE_ERR_INVALID_ARG and "strides" in _err() and "34 out" in _err(), kw
    assert _whole(lib, rs._h, B=70000) == FE_ERR_INVALID_ARG and "grid" in _err()
    # more workgroups than one launch takes (fewer than 2^32 threads): refused here, not by the launch
    big = dict(n_in=2 ** 39, in_stride=2 ** 39, out_stride=2 ** 39)
    assert _whole(lib, rs._h, **big) == FE_ERR_INVALID_ARG and "exceed the launch grid" in _err() and "split the call" in _err()
    assert _whole(lib, rs._h, n_in=3 * 1024 * 300, in_stride=2 ** 20, out_stride=2 ** 20, B=60000) == FE_ERR_INVALID_ARG and "18000000" not in _err() \
        and "300 tiles x 60000 rows" in _err()


def _streams(lib, fn, rs, x=P, in_count=1024, in_format=1, state=P, capacity=4, desc=P, out=P, out_count=1024, out_format=1, produced=NULL, n=1,
             n_in_max=960):
    return getattr(lib, fn)(rs, x, in_count, in_format, state, capacity, desc, out, out_count, out_format, produced, n, n_in_max, NULL)


@pytest.mark.parametrize("fn", ["fe_resample_streams", "fe_resample_streams_pinned"])
def test_the_stream_entry_points_check_their_arguments_before_any_device_work(fn):
    lib, rs = _lib.load(), Resampler(48000, 16000)
    assert _streams(lib, fn, NULL) == FE_ERR_INVALID_ARG and fn + ": null resampler" in _err()
    bad = [dict(x=NULL), dict(state=NULL), dict(desc=NULL), dict(out=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0), dict(n_in_max=0),
           dict(n_in_max=-3), dict(in_count=0), dict(out_count=0)]
    for kw in bad:
        assert _streams(lib, fn, rs._h, **kw) == FE_ERR_INVALID_ARG and fn + ": bad argument" in _err(), kw
    for kw in (dict(in_format=2), dict(in_format=-1), dict(out_format=3)):
        assert _streams(lib, fn, rs._h, **kw) == FE_ERR_INVALID_ARG and "neither FE_AUDIO_F32 (0) nor FE_AUDIO_S16 (1)" in _err(), kw
    up = Resampler(16000, 48000)
    assert _streams(lib, fn, up._h, n_in_max=2 ** 31 - 1) == FE_ERR_INVALID_ARG and "produced" in _err()


def test_the_pinned_twin_refuses_pageable_memory():
    lib, rs = _lib.load(), Resampler(48000, 16000)
    x = torch.zeros(1024, dtype=torch.int16)
    rc = _streams(lib, "fe_resample_streams_pinned", rs._h, x=c_void_p(x.data_ptr()), out=c_void_p(x.data_ptr()))
    assert rc == FE_ERR_INVALID_ARG and "fe_resample_streams_pinned: in is not page-locked host memory" in _err()


# ------------------------------------------------------------------ Resampler: host checks, then the device requirement
class _Pinned(torch.Tensor):
    """a CPU tensor that passes for page-locked memory (no CPU-only process can pin one)"""
    def is_pinned(self, *a, **kw):
        return True


class _Dev(torch.Tensor):
    """... and one that passes for a device tensor"""
    is_cuda = property(lambda self: True)


def test_resampler_checks_then_needs_a_gpu():
    rs = Resampler(48000, 16000)
    s = torch.zeros(1024, dtype=torch.int16)
    st = torch.zeros(4, rs.state_floats)
    for pinned, call in ((False, rs.step_streams), (True, rs.step_streams_pinned)):
        a = s.clone().as_subclass(_Pinned if pinned else _Dev)
        for desc, msg in (([(0, 10, 0, 0), (0, 10, 100, 100)], "duplicate slots"), ([(4, 1, 0, 0)], "slot 4 is outside"), ([(-1, 1, 0, 0)], "outside"),
                          ([(0, 961, 0, 0)], "n_in 961 is outside"), ([(0, -1, 0, 0)], "n_in -1"), ([(0, 960, 65, 0)], "input range"),
                          ([(0, 1, -1, 0)], "input range"), ([(0, 1, 0, -1)], "negative"), ([], "0 streams"),
                          (torch.zeros(2, 4, dtype=torch.int32), "descriptor tensor")):
            with pytest.raises(ValueError, match=msg):
                call(a, st, 4, desc, a, 960)
        with pytest.raises(ValueError, match="n_in_max"):
            call(a, st, 4, [(0, 1, 0, 0)], a, 0)
        with pytest.raises(ValueError, match="produced must be a contiguous int32 tensor \\[1\\]"):
            call(a, st, 4, [(0, 1, 0, 0)], a, 960, produced=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(ValueError, match="page-locked" if pinned else "device tensor"):
            call(s, st, 4, [(0, 1, 0, 0)], s, 960)
        with pytest.raises(ValueError, match="float32 or int16"):
            call(torch.zeros(4, dtype=torch.float64), st, 4, [(0, 1, 0, 0)], a, 960)
        with pytest.raises(_lib.FEError, match="needs a GPU"):           # a valid call gets as far as the device requirement
            call(a, st, 4, [(0, 10, 0, 0)], a, 960)
    with pytest.raises(ValueError, match="float32 or int16"):
        rs(torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        rs(torch.zeros(2, 8))
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        rs.new_state(4)


# ------------------------------------------------------------------ ResampledPacketPool over a stub engine and stub resamplers
class _StubResampler:
    """the host formulas of the real one; step_streams_pinned records the call and writes `produced` samples of value = the slot's
    call number"""
    def __init__(self, log, sr_in, sr_out, device):
        self.log, self.real, self.tag = log, Resampler(sr_in, sr_out), f"{sr_in}->{sr_out}"
        self.state_floats = self.real.state_floats
        self.count = {}

    def out_count(self, n):
        return self.real.out_count(n)

    def produced(self, consumed, n):
        return self.real.produced(consumed, n)

    def new_state(self, capacity):
        return torch.zeros(capacity, self.state_floats)

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        self.log.append((self.tag, "synchronize"))

    def step_streams_pinned(self, x, state, capacity, desc, out, n_in_max, produced=None):
        self.log.append((self.tag, "step_streams_pinned", list(desc), n_in_max))
        assert tuple(produced.shape) == (len(desc),)           # (what the real one requires)
        for i, (slot, n, i0, o0) in enumerate(desc):
            consumed = int(state[slot, -1])
            made = self.real.produced(consumed, n)
            state[slot, -1] = consumed + n               # (a stand-in for the row: a fresh stream must find 0 here)
            state[slot, 0] = 1.0
            out.view(-1)[o0:o0 + made] = 7
            produced[i] = made
        return out


class _StubPool:
    """PacketPool's public surface: echoes what is pushed, a hop at a time"""
    def __init__(self, log, engine, capacity, ring_hops, T_max):
        self.log, self.H, self.T_max, self.ring, self.capacity = log, 256, T_max, ring_hops * 256, capacity
        self.free, self.buf, self.done = list(range(capacity - 1, -1, -1)), {}, {}

    def open(self):
        slot = self.free.pop()
        self.buf[slot], self.done[slot] = torch.zeros(0, dtype=torch.int16), torch.zeros(0, dtype=torch.int16)
        self.log.append(("inner", "open", slot))
        return slot

    def close(self, slot):
        self.free.append(slot)
        self.log.append(("inner", "close", slot))

    def push(self, slot, pcm):
        self.log.append(("inner", "push", slot, int(pcm.numel())))
        self.buf[slot] = torch.cat([self.buf[slot], pcm.clone()])

    def tick(self):
        self.log.append(("inner", "tick"))
        desc = []
        for slot in sorted(self.buf):
            hops = min(self.buf[slot].numel() // self.H, self.T_max)
            if hops:
                self.done[slot] = torch.cat([self.done[slot], self.buf[slot][:hops * self.H]])
                self.buf[slot] = self.buf[slot][hops * self.H:]
                desc.append((slot, hops, 0, 0))
        return desc

    def pull(self, slot):
        y, self.done[slot] = self.done[slot], torch.zeros(0, dtype=torch.int16)
        self.log.append(("inner", "pull", slot, int(y.numel())))
        return y


class _Engine:
    device = None


def _stub_pool(monkeypatch, log, **kw):
    monkeypatch.setattr(ResampledPacketPool, "_make_pool", staticmethod(lambda engine, capacity, ring_hops, T_max: _StubPool(log, engine, capacity, ring_hops, T_max)))
    monkeypatch.setattr(ResampledPacketPool, "_make_resampler", staticmethod(lambda a, b, device: _StubResampler(log, a, b, device)))
    return ResampledPacketPool(_Engine(), **kw)


def test_resampled_pool_runs_its_five_steps_in_order(monkeypatch):
    log = []
    pool = _stub_pool(monkeypatch, log, capacity=2, ring_hops=8, client_rate=48000, T_max=1, max_packet=1920)
    rs = Resampler(48000, 16000)
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1) and pool.active == [0, 1]
    pool.push(a, torch.ones(960, dtype=torch.int16))
    pool.push(a, np.ones(960, dtype=np.int16))
    pool.push(b, torch.ones(100, dtype=torch.int16))
    del log[:]
    assert pool.tick() == [(0, 1, 0, 0)]              # slot 0: 630 model samples, one hop of T_max = 1; slot 1: 24, none
    made_a, made_b = rs.produced(0, 1920), rs.produced(0, 100)
    assert (made_a, made_b) == (630, 24)
    back = Resampler(16000, 48000).produced(0, 256)
    assert [e[:2] for e in log] == [("48000->16000", "step_streams_pinned"), ("48000->16000", "synchronize"), ("inner", "push"), ("inner", "push"),
                                    ("inner", "tick"), ("inner", "pull"), ("inner", "pull"), ("16000->48000", "step_streams_pinned"),
                                    ("16000->48000", "synchronize")]
    assert log[0][2] == [(0, 1920, 0, 0), (1, 100, 1920, pool._model_cap)] and log[0][3] == 1920
    assert log[2] == ("inner", "push", 0, made_a) and log[3] == ("inner", "push", 1, made_b)
    assert log[7][2] == [(0, 256, 0, 0)] and log[7][3] == 256
    # counters: consumed client samples, nothing pending, what sits in the inner pool
    assert pool._consumed == [1920, 100] and pool._pending == [0, 0] and pool._fill == [made_a - 256, made_b]
    y = pool.pull(a)
    assert y.dtype == torch.int16 and y.numel() == back and bool((y == 7).all())
    assert pool.pull(a).numel() == 0 and pool.pull(b).numel() == 0
    # a tick with nothing pending skips launch 1 and still ticks the inner pool, which has a second hop of slot 0 waiting
    del log[:]
    assert pool.tick() == [(0, 1, 0, 0)]
    assert [e[:2] for e in log] == [("inner", "tick"), ("inner", "pull"), ("inner", "pull"), ("16000->48000", "step_streams_pinned"),
                                    ("16000->48000", "synchronize")]
    assert pool.pull(a).numel() == Resampler(16000, 48000).produced(256, 256)


def test_resampled_pool_refusals(monkeypatch):
    log = []
    with pytest.raises(ValueError, match="use PacketPool"):
        _stub_pool(monkeypatch, log, capacity=2, ring_hops=8, client_rate=16000)
    with pytest.raises(ValueError, match="use PacketPool"):
        _stub_pool(monkeypatch, log, capacity=2, ring_hops=8, client_rate=48000, model_rate=48000)
    with pytest.raises(ValueError, match="max_packet"):
        _stub_pool(monkeypatch, log, capacity=2, ring_hops=8, client_rate=48000, max_packet=0)
    pool = _stub_pool(monkeypatch, log, capacity=2, ring_hops=2, client_rate=48000, max_packet=1000)
    assert _stub_pool(monkeypatch, log, capacity=1, ring_hops=2, client_rate=8000, T_max=3).max_packet == 384       # 3 hops of 256 at half the rate
    with pytest.raises(ValueError, match="slot 0 is not open"):
        pool.push(0, torch.zeros(4, dtype=torch.int16))
    with pytest.raises(ValueError, match="not open"):
        pool.pull(1)
    with pytest.raises(ValueError, match="not open"):
        pool.close(0)
    s = pool.open()
    with pytest.raises(ValueError, match="1-D int16"):
        pool.push(s, torch.zeros(4))
    with pytest.raises(ValueError, match="1-D int16"):
        pool.push(s, torch.zeros(2, 2, dtype=torch.int16))
    pool.push(s, torch.zeros(600, dtype=torch.int16))
    with pytest.raises(OverflowError, match="max_packet = 1000"):
        pool.push(s, torch.zeros(401, dtype=torch.int16))
    assert pool._pending[s] == 600                      # nothing of the refused packet was taken
    pool.push(s, torch.zeros(400, dtype=torch.int16))
    pool.tick()
    # the inner ring (2 hops = 512 samples) holds 324 - 256 = 68 samples; 1000 more client samples become 333 model samples: 401.  With the
    # inner pool stalled they stay there, and of the next 1000 only what keeps the ring within 512 is taken
    assert pool._fill[s] == 68
    pool.push(s, torch.zeros(1000, dtype=torch.int16))
    monkeypatch.setattr(pool.inner, "tick", lambda: [])
    pool.tick()
    assert pool._fill[s] == 401
    pool.push(s, torch.zeros(300, dtype=torch.int16))
    with pytest.raises(OverflowError, match="inner pool's ring holds 512"):
        pool.push(s, torch.zeros(700, dtype=torch.int16))


def test_resampled_pool_slot_reuse_starts_from_a_zero_row(monkeypatch):
    log = []
    pool = _stub_pool(monkeypatch, log, capacity=2, ring_hops=8, client_rate=48000, max_packet=1920)
    s = pool.open()
    pool.push(s, torch.ones(1920, dtype=torch.int16))
    pool.tick()
    assert bool(pool.state_in[s].any()) and bool(pool.state_out[s].any()) and pool._consumed[s] == 1920
    pool.close(s)
    assert not bool(pool.state_in[s].any()) and not bool(pool.state_out[s].any())
    assert pool.active == []
    pool.state_in[s] = 5.0                               # whatever the row holds while the slot is free
    t = pool.open()
    assert t == s and not bool(pool.state_in[t].any()) and not bool(pool.state_out[t].any())
    assert (pool._consumed[t], pool._pending[t], pool._fill[t]) == (0, 0, 0) and pool.pull(t).numel() == 0
    pool.push(t, torch.ones(100, dtype=torch.int16))
    del log[:]
    pool.tick()
    assert log[2] == ("inner", "push", t, 24)            # M(100) of a FRESH stream: (100 - 30) / 3 rounded up


def test_resampled_pool_stays_consistent_when_the_inner_push_raises(monkeypatch):
    """the launch has consumed the samples of every stream by then: the counters say so for all of them, the refused samples are dropped"""
    log = []
    pool = _stub_pool(monkeypatch, log, capacity=2, ring_hops=8, client_rate=48000, max_packet=1920)
    a, b = pool.open(), pool.open()
    pool.push(a, torch.ones(960, dtype=torch.int16))
    pool.push(b, torch.ones(480, dtype=torch.int16))

    def refuse(slot, pcm):
        raise OverflowError("full")
    monkeypatch.setattr(pool.inner, "push", refuse)
    with pytest.raises(OverflowError, match="full"):
        pool.tick()
    assert pool._consumed == [960, 480] and pool._pending == [0, 0] and pool._fill == [0, 0]
    assert [int(pool.state_in[s, -1]) for s in (a, b)] == [960, 480]        # what the (stub) resampler rows hold


# ------------------------------------------------------------------ the callers
def test_read_wav_still_refuses_another_rate_without_the_flag(tmp_path):
    from scipy.io import wavfile
    from fastenhancer_amd.scripts.common import read_wav
    x = (0.1 * np.random.default_rng(0).standard_normal(4800)).astype(np.float32)
    wavfile.write(str(tmp_path / "a.wav"), 48000, x)
    with pytest.raises(ValueError, match="resample the file first"):
        read_wav(str(tmp_path / "a.wav"), 16000)
    with pytest.raises(_lib.FEError, match="needs a GPU"):       # with the flag the file gets as far as the resampler
        read_wav(str(tmp_path / "a.wav"), 16000, resample=True, device="cpu")
    np.testing.assert_array_equal(read_wav(str(tmp_path / "a.wav"), 48000, resample=True, device="cpu"), x)      # the model's rate: nothing to do


@pytest.mark.parametrize("script", ["enhance_dir", "stream_chunks"])
def test_the_callers_have_the_flag_off_by_default(script, capsys):
    import importlib
    mod = importlib.import_module(f"fastenhancer_amd.scripts.{script}")
    for argv in (["--help"], ["--chunk-hops", "8", "--help"]) if script == "stream_chunks" else (["--help"],):
        with pytest.raises(SystemExit):
            mod.main(argv)
        assert "--resample" in capsys.readouterr().out


def test_the_flag_reaches_the_delegated_caller_through_the_switch(tmp_path, monkeypatch):
    """enhance_dir and stream_chunks run test_offline / test_streaming, whose read_wav(path, sr) names no resampling: inside the wrapper's
    call the switch is on (with the caller's device), outside it and without the flag it is off"""
    from scipy.io import wavfile
    from fastenhancer_amd.scripts import common, enhance_dir, stream_chunks, test_offline, test_streaming
    seen = []
    monkeypatch.setattr(test_offline, "main", lambda argv: seen.append(("offline", common._RESAMPLING_ON, list(argv))))
    monkeypatch.setattr(test_streaming, "main", lambda argv: seen.append(("streaming", common._RESAMPLING_ON, list(argv))))
    enhance_dir.main(["-n", "run", "-i", "a", "--resample"])
    enhance_dir.main(["-n", "run", "-i", "a", "--device", "cuda:1", "--resample"])
    enhance_dir.main(["-n", "run", "-i", "a"])
    stream_chunks.main(["--audio-path", "a.wav", "--resample"])
    stream_chunks.main(["--audio-path", "a.wav"])
    assert seen == [("offline", "cuda:0", ["-n", "run", "-i", "a"]),                         # (only --resample is taken out of the arguments)
                    ("offline", "cuda:1", ["-n", "run", "-i", "a", "--device", "cuda:1"]),
                    ("offline", None, ["-n", "run", "-i", "a"]),
                    ("streaming", "cuda:0", ["--audio-path", "a.wav"]),
                    ("streaming", None, ["--audio-path", "a.wav"])]
    assert common._RESAMPLING_ON is None
    x = np.zeros(480, dtype=np.float32)
    wavfile.write(str(tmp_path / "a.wav"), 48000, x)
    with common.resampling("cpu"):
        with pytest.raises(_lib.FEError, match="needs a GPU"):          # read_wav(path, sr) as the delegated callers call it
            common.read_wav(str(tmp_path / "a.wav"), 16000)
        with pytest.raises(ValueError, match="resample the file first"):    # an explicit False stays False
            common.read_wav(str(tmp_path / "a.wav"), 16000, resample=False)
    with pytest.raises(ValueError, match="resample the file first"):
        common.read_wav(str(tmp_path / "a.wav"), 16000)
