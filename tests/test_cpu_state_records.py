"""CPU tests of the state records (fe_state_export_slots / fe_state_import_slots, Engine.export_slots / import_slots, StreamPool.export /
adopt / move / resize, PacketPool's ring carry-over): the ABI, the argument checks that come before any device work, the record size of
every family, and the pools' bookkeeping with the engine calls stubbed."""
import os
import re
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool, StreamPool, carry_ring
from test_cpu_host_queries import make_engine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastenhancer_hip.h")
FE_OK, FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG, FE_ERR_HIP = 0, -1, -2, -3
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
ENTRY_POINTS = ("fe_state_export_slots", "fe_state_import_slots")


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, state=P, capacity=4, slots=P, records=P, n=1):
    return getattr(lib, fn)(h, state, capacity, slots, records, n, NULL)


# ------------------------------------------------------------------ the ABI
def test_header_declares_both_functions_and_the_binding_has_their_signatures():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint (fe_state_(?:export|import)_slots)\s*\((.*?)\);", src, re.S)}
    assert decl == {
        "fe_state_export_slots": "fe_handle* h, const float* state_dev, int capacity, const int* slots_dev, float* records, int n, void* stream",
        "fe_state_import_slots": "fe_handle* h, float* state_dev, int capacity, const int* slots_dev, const float* records, int n, void* stream",
    }
    lib = _lib.load()
    for fn in ENTRY_POINTS:
        assert _lib.SYMBOLS[fn] == (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p])
        assert getattr(lib, fn).restype is c_int and list(getattr(lib, fn).argtypes) == _lib.SYMBOLS[fn][1]


# ------------------------------------------------------------------ argument checks of the library (no GPU: they come first)
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_record_entry_points_refuse_a_null_handle(fn):
    assert _call(_lib.load(), fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("name", ["fe_b", "bsrnn_xt", "fspen", "lisennet"])
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_record_entry_points_check_their_arguments(fn, name):
    eng = make_engine(name)
    bad = [dict(state=NULL), dict(slots=NULL), dict(records=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0), dict(capacity=-2)]
    for kw in bad:
        assert _call(eng.lib, fn, eng._h, **kw) == FE_ERR_INVALID_ARG, kw
        assert fn in _err() and "1 <= n <= capacity" in _err(), (kw, _err())


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_record_entry_points_refuse_the_noncausal_model_as_fe_step_does(fn):
    nc = Engine(product_config("fe_nc"), None)
    assert _call(nc.lib, fn, nc._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_record_entry_points_take_the_baseline_families(fn):
    """BSRNN-xt is not refused as a family: the call gets as far as the device - without one that is FE_ERR_HIP; with one, the lookup of the
    dummy records pointer, which is no memory the kernel may address"""
    eng = Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xt"][0]), None)
    rc = _call(eng.lib, fn, eng._h)
    assert rc != FE_ERR_UNSUPPORTED_CONFIG, _err()
    if torch.cuda.is_available():
        assert rc == FE_ERR_INVALID_ARG and "page-locked" in _err(), (rc, _err())
    else:
        assert rc == FE_ERR_HIP, (rc, _err())


# ------------------------------------------------------------------ the record size
def _record_floats(name):
    """floats of one stream's state from the layout the header documents"""
    from common import FSPEN_KWARGS, LISENNET_KWARGS
    if name in BSRNN_KWARGS:
        kw = BSRNN_KWARGS[name][0]
        return 2 * (512 - 256) + 2 * kw["num_layers"] * 31 * 2 * kw["num_channels"]
    if name == "fspen":
        d = FSPEN_KWARGS[0]["dpe_kwargs"]
        return 2 * (512 - 256) + d["num_blocks"] * d["groups"] * (d["freq"] // d["groups"]) * d["channels"]
    if name == "lisennet":
        nb = LISENNET_KWARGS[0]["n_blocks"]
        return 2 * (512 - 256) + 257 + 4 * 257 + 8 * 128 + 12 * 64 + nb * (32 * 24 + 32 * 2 * 32) + 4 * 256
    c = product_config(name)
    n = 2 * (c.n_fft - c.hop_size)
    if c.dpt:
        n += 2 * c.rf_blocks * c.rf_freq * c.rf_channels * c.lookbehind + 1
    else:
        n += c.rf_blocks * c.rf_freq * c.rf_channels
    if c.time_kernel:
        n += 2 * c.n_layers * (c.kernel_size_time - 1) * c.F1 * c.channels
    return n


@pytest.mark.parametrize("name", ["fe_t", "fe_b", "fe_tk_b", "fe_ln_b", "fe_dprnn_b", "fe_dpt_t", "fe_dpt_b", "bsrnn_xxt", "bsrnn_xt", "fspen", "lisennet"])
def test_a_record_is_the_state_of_one_stream_and_a_state_is_that_many_records(name):
    eng = make_engine(name)
    one = eng.lib.fe_state_floats(eng._h, 1)
    assert one == _record_floats(name) == eng.record_floats
    for B in (3, 5):
        assert eng.lib.fe_state_floats(eng._h, B) == B * one


def _no_native(monkeypatch, eng):
    real = eng.lib

    class Guard:
        def __getattr__(self, name):
            if name == "fe_state_floats":
                return real.fe_state_floats
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


def test_engine_checks_records_before_any_device_call(monkeypatch):
    eng = Engine(product_config("fe_t"), None)
    _no_native(monkeypatch, eng)
    rf = eng.record_floats
    for rec, match in [(torch.zeros(2, rf), "page-locked"), (torch.zeros(2, rf + 1), "float32 tensor"), (torch.zeros(3, rf), "float32 tensor"),
                       (torch.zeros(2, rf, dtype=torch.float64), "float32 tensor"), (torch.zeros(2, 2 * rf)[:, :rf], "back to back"), (None, "float32 tensor")]:
        with pytest.raises(ValueError, match=match):
            eng.import_slots(torch.zeros(1), 8, [1, 2], rec)
        if rec is not None:
            with pytest.raises(ValueError, match=match):
                eng.export_slots(torch.zeros(1), 8, [1, 2], out=rec)
    with pytest.raises(ValueError, match="duplicate"):
        eng.export_slots(torch.zeros(1), 8, [1, 1])
    with pytest.raises(ValueError, match="outside"):
        eng.export_slots(torch.zeros(1), 8, [8])


# ------------------------------------------------------------------ PacketPool's ring carry-over against a per-sample loop
def _carry_reference(src_in, src_out, pushed, stepped, pulled, rd):
    rs = len(src_in)
    dst_in, dst_out = [None] * rd, [None] * rd
    for k in range(stepped, pushed):
        dst_in[k % rd] = int(src_in[k % rs])
    for k in range(pulled, stepped):
        dst_out[k % rd] = int(src_out[k % rs])
    return dst_in, dst_out


H = 16
CARRY_CASES = [
    # (source ring, destination ring, pushed, stepped, pulled)
    (8 * H, 8 * H, 3 * H + 5, 2 * H, H + 3),              # not wrapped, equal rings
    (8 * H, 4 * H, 3 * H + 5, 2 * H, H + 3),              # not wrapped, smaller destination
    (8 * H, 12 * H, 3 * H + 5, 2 * H, H + 3),             # not wrapped, larger destination
    (8 * H, 8 * H, 21 * H + 7, 19 * H, 15 * H + 9),       # the source position wrapped (and what is in flight straddles the ring end)
    (8 * H, 6 * H, 21 * H + 7, 19 * H, 15 * H + 9),       # wrapped, smaller: 5 H + 14 samples into 6 H
    (8 * H, 16 * H, 21 * H + 7, 19 * H, 15 * H + 9),      # wrapped, larger
    (8 * H, 4 * H, 0, 0, 0),                              # the empty stream
    (8 * H, 4 * H, 11 * H, 11 * H, 11 * H),               # empty again: everything stepped and pulled
    (8 * H, 8 * H, 13 * H + 3, 9 * H, 5 * H + 3),         # the exactly-full ring
    (8 * H, 4 * H, 13 * H + 3, 12 * H, 9 * H + 3),        # exactly full in the (smaller) destination
]


@pytest.mark.parametrize("rs,rd,pushed,stepped,pulled", CARRY_CASES)
def test_carry_ring_matches_a_per_sample_loop(rs, rd, pushed, stepped, pulled):
    rng = np.random.default_rng(rs + 3 * rd + pushed)
    src_in = torch.from_numpy(rng.integers(-32768, 32768, size=rs, dtype=np.int16))
    src_out = torch.from_numpy(rng.integers(-32768, 32768, size=rs, dtype=np.int16))
    fill = torch.from_numpy(rng.integers(-32768, 32768, size=rd, dtype=np.int16))
    dst_in, dst_out = fill.clone(), fill.clone()
    keep = (src_in.clone(), src_out.clone())
    assert carry_ring(src_in, src_out, pushed, stepped, pulled, dst_in, dst_out) == (pushed, stepped, pulled)
    assert torch.equal(src_in, keep[0]) and torch.equal(src_out, keep[1])
    want_in, want_out = _carry_reference(src_in.tolist(), src_out.tolist(), pushed, stepped, pulled, rd)
    for got, want in ((dst_in, want_in), (dst_out, want_out)):
        for i in range(rd):              # what is in flight arrived at k mod ring; every other sample of the destination is as it was
            assert int(got[i]) == (int(fill[i]) if want[i] is None else want[i]), i
    assert sum(w is not None for w in want_in) == pushed - stepped and sum(w is not None for w in want_out) == stepped - pulled


def test_carry_ring_refuses_one_sample_too_many_before_copying():
    rs, rd = 8 * H, 4 * H
    src = torch.arange(rs, dtype=torch.int16)
    dst_in, dst_out = torch.full((rd,), -7, dtype=torch.int16), torch.full((rd,), -7, dtype=torch.int16)
    with pytest.raises(OverflowError, match="do not fit"):
        carry_ring(src, src, 13 * H + 4, 12 * H, 9 * H + 3, dst_in, dst_out)          # 4 H + 1 in flight
    assert bool((dst_in == -7).all()) and bool((dst_out == -7).all())
    with pytest.raises(ValueError):
        carry_ring(src, src, 9 * H, 0, 0, dst_in, dst_out)                             # more than the source ring could hold


# ------------------------------------------------------------------ the pools with the engine stubbed
class _Cfg:
    hop_size = 256

    def __eq__(self, other):
        return isinstance(other, _Cfg)


class _OtherCfg(_Cfg):
    pass


class _StubEngine:
    """what the pools need of an Engine: a record is one float per stream (its state), the packet launch copies input hops to the output"""
    record_floats = 1

    def __init__(self, cfg=None):
        self.cfg = cfg or _Cfg()
        self.calls = []

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        state[list(slots)] = 0.0

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        pass

    def export_slots(self, state, capacity, slots, out=None):
        assert state.numel() == capacity
        self.calls.append(("export", capacity, list(slots)))
        rec = state[list(slots)].reshape(-1, 1).clone()
        if out is not None:
            out.copy_(rec)
            return out
        return rec

    def import_slots(self, state, capacity, slots, records):
        assert state.numel() == capacity and tuple(records.shape) == (len(slots), 1)
        self.calls.append(("import", capacity, list(slots)))
        state[list(slots)] = records[:, 0]

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1):
        fin, fout = wav_in.view(-1), wav_out.view(-1)
        for slot, hops, i0, o0 in desc:
            fout[o0:o0 + hops * 256] = fin[i0:i0 + hops * 256]
            state[slot] += hops
        return wav_out


def test_adopt_with_too_few_free_slots_opens_none():
    eng = _StubEngine()
    pool = StreamPool(eng, 3)
    a = pool.open()
    pool.state[a] = 5.0
    free = list(pool._free)
    with pytest.raises(RuntimeError, match="3 records for 2 free slots"):
        pool.adopt(torch.tensor([[1.0], [2.0], [3.0]]))
    assert pool.active == [a] and pool._free == free and eng.calls == []
    assert pool.adopt(torch.tensor([[1.0], [2.0]])) == [1, 2]                          # lowest free slot first, in record order
    assert pool.active == [0, 1, 2] and pool._free == [] and pool.state.tolist() == [5.0, 1.0, 2.0]
    assert eng.calls == [("import", 3, [1, 2])]
    assert pool.adopt(torch.zeros(0, 1)) == []
    rec = pool.export([2, 0])
    assert rec.tolist() == [[2.0], [5.0]] and pool.active == [0, 1, 2]                 # the slots stay open
    pool.close(1)
    with pytest.raises(ValueError, match="slot 1 is not open"):
        pool.export([0, 1])


def test_resize_below_an_open_slot_raises_and_changes_nothing():
    eng = _StubEngine()
    pool = StreamPool(eng, 4)
    for _ in range(3):
        pool.open()
    pool.close(1)
    pool.state[0], pool.state[2] = 3.0, 4.0
    state, free = pool.state, list(pool._free)
    with pytest.raises(ValueError, match="slot 2 is open"):
        pool.resize(2)
    with pytest.raises(ValueError):
        pool.resize(0)
    assert pool.state is state and pool.capacity == 4 and pool._free == free and pool.active == [0, 2] and eng.calls == []
    pool.resize(3)                                                                      # 1 + the highest open slot: the smallest that fits
    assert pool.state is not state and pool.capacity == 3 and pool.state.tolist() == [3.0, 0.0, 4.0]
    assert eng.calls == [("export", 4, [0, 2]), ("import", 3, [0, 2])]
    assert pool.open() == 1
    with pytest.raises(RuntimeError, match="all 3 slots are open"):
        pool.open()
    pool.resize(6)
    assert pool.state.tolist() == [3.0, 0.0, 4.0, 0.0, 0.0, 0.0] and [pool.open() for _ in range(3)] == [3, 4, 5]


def test_move_refuses_a_config_mismatch_and_a_full_destination_before_copying():
    a, b, c = _StubEngine(), _StubEngine(), _StubEngine(_OtherCfg())
    src, dst, other = StreamPool(a, 2), StreamPool(b, 1), StreamPool(c, 2)
    s = src.open()
    src.state[s] = 9.0
    with pytest.raises(ValueError, match="different configs"):
        src.move(s, other)
    with pytest.raises(ValueError, match="not open"):
        src.move(1, dst)
    assert a.calls == b.calls == c.calls == [] and src.active == [s] and other.active == []
    assert src.move(s, dst) == 0
    assert src.active == [] and dst.active == [0] and dst.state.tolist() == [9.0]
    s = src.open()
    with pytest.raises(RuntimeError, match="destination"):
        src.move(s, dst)
    assert src.active == [s]


def _pcm(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-32768, 32768, size=n, dtype=np.int16))


def test_packet_pool_move_and_resize_carry_the_rings_and_counters():
    """a stream fed 160-sample packets moves between pools of different ring_hops while it holds un-stepped input and un-pulled output,
    and lives through a resize: with the identity "model" of the stub what is pulled is what was pushed, in order"""
    eng = _StubEngine()
    pools = [PacketPool(eng, 2, ring_hops=8, T_max=2), PacketPool(eng, 3, ring_hops=5, T_max=2), PacketPool(eng, 2, ring_hops=11, T_max=2)]
    pool, slot = pools[0], None
    pools[1].open()                                                  # (the stream lands in another slot number there)
    slot = pool.open()
    sent, got = [], []
    both = 0
    for tick in range(90):
        x = _pcm(160, tick)
        pool.push(slot, x)
        sent.append(x)
        pool.tick()
        if tick % 7 == 4:
            both += pool._pushed[slot] > pool._stepped[slot] > pool._pulled[slot]     # both kinds of samples in flight
            nxt = pools[(pools.index(pool) + 1) % 3]
            hops = float(pool.state[slot])
            slot, pool = pool.move(slot, nxt), nxt
            assert float(pool.state[slot]) == hops                                      # the state went along
        if tick % 3 == 0:
            got.append(pool.pull(slot))
        if tick == 40:
            pool.resize(pool.capacity + 2)
            assert pool.ring_in.shape[0] == pool.capacity == len(pool._pushed)
    got.append(pool.pull(slot))
    assert both >= 6, both
    sent, got = torch.cat(sent), torch.cat(got)
    assert got.numel() >= 90 * 160 - 2 * 256 and torch.equal(got, sent[:got.numel()])
    small = PacketPool(eng, 1, ring_hops=1, T_max=1)
    pool.push(slot, _pcm(300, 1000))
    before = (pool.active, list(pool._pushed))
    with pytest.raises(OverflowError, match="do not fit"):
        pool.move(slot, small)
    assert (pool.active, list(pool._pushed)) == before and small.active == []
    with pytest.raises(TypeError):
        pool.move(slot, StreamPool(eng, 1))
