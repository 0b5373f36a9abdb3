"""CPU tests of the resampler's ring form (fe_resample_rings[_pinned], Resampler.step_rings[_pinned], serving.RingResampledPacketPool): the
declarations and the binding, the refusals that come before any device work - word for word those of fe_resample_streams[_pinned] - the
host check of list descriptors, and the new pool against ResampledPacketPool with the engine and the resamplers recorded instead of run."""
import ctypes
import re
from ctypes import c_void_p
from pathlib import Path

import numpy as np
import pytest
import torch

import resample_oracle as ro
from fastenhancer_amd import _lib
from fastenhancer_amd.resample import Resampler
from fastenhancer_amd.serving import PacketPool, ResampledPacketPool, RingResampledPacketPool

FE_ERR_INVALID_ARG = -1
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
RING_FNS = {"fe_resample_rings": "fe_resample_streams", "fe_resample_rings_pinned": "fe_resample_streams_pinned"}


def _err():
    return _lib.load().fe_last_error().decode()


# ------------------------------------------------------------------ the ABI
def test_the_header_declares_both_functions_and_the_struct_and_the_binding_types_them():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    lib = _lib.load()
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(fe_resample_rings(?:_pinned)?)\s*\(([^)]*)\)\s*;", text)}
    assert set(decl) == set(RING_FNS) and len(set(decl.values())) == 1                 # the same parameter list
    streams = re.search(r"\bint\s+fe_resample_streams\s*\(([^)]*)\)\s*;", text).group(1)
    assert decl["fe_resample_rings"] == " ".join(streams.split()).replace("fe_resample_desc", "fe_resample_ring_desc")      # ... and fe_resample_streams'
    for name in RING_FNS:
        assert name in _lib.SYMBOLS and hasattr(lib, name)                             # the library exports both
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS["fe_resample_streams"]
    assert re.search(r"typedef struct fe_resample_ring_desc\s*\{\s*int slot, n_in;\s*long long in_base, out_base;\s*int in_len, in_pos;\s*"
                     r"int out_len, out_pos;\s*\}\s*fe_resample_ring_desc;", text)
    assert ctypes.sizeof(_lib.fe_resample_ring_desc) == 40
    # the memory image of a row with a base above 2^32: low word first
    assert Resampler.pack_ring_desc([(3, 7, (1 << 33) + 9, 5, 449, 2, 149, 1)]).tolist() == [[3, 7, 9, 2, 5, 0, 449, 2, 149, 1]]
    assert Resampler.pack_ring_desc([]).shape == (0, 10)
    with pytest.raises(ValueError, match="a ring descriptor is"):
        Resampler.pack_ring_desc([(0, 1, 0, 0)])


def _call(lib, fn, rs, x=P, in_count=1024, in_format=1, state=P, capacity=4, desc=P, out=P, out_count=1024, out_format=1, produced=NULL, n=1, n_in_max=960):
    return getattr(lib, fn)(rs, x, in_count, in_format, state, capacity, desc, out, out_count, out_format, produced, n, n_in_max, NULL)


@pytest.mark.parametrize("fn", sorted(RING_FNS))
def test_the_ring_entry_points_refuse_what_the_stream_entry_points_refuse_in_their_words(fn):
    """the table of test_cpu_resample.py's _streams cases: for every bad argument both calls fail, and the texts differ in the function's name only"""
    lib, down, up = _lib.load(), Resampler(48000, 16000), Resampler(16000, 48000)
    twin = RING_FNS[fn]
    cases = [(NULL, {})]
    cases += [(down._h, kw) for kw in (dict(x=NULL), dict(state=NULL), dict(desc=NULL), dict(out=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0),
                                       dict(n_in_max=0), dict(n_in_max=-3), dict(in_count=0), dict(out_count=0), dict(in_format=2), dict(in_format=-1),
                                       dict(out_format=3))]
    cases += [(up._h, dict(n_in_max=2 ** 31 - 1))]
    for h, kw in cases:
        assert _call(lib, twin, h, **kw) == FE_ERR_INVALID_ARG
        want = _err()
        assert twin in want
        assert _call(lib, fn, h, **kw) == FE_ERR_INVALID_ARG, kw
        assert _err() == want.replace(twin, fn), kw
    assert _call(lib, fn, NULL) == FE_ERR_INVALID_ARG and fn + ": null resampler" in _err()
    assert _call(lib, fn, down._h, in_format=2) == FE_ERR_INVALID_ARG and "neither FE_AUDIO_F32 (0) nor FE_AUDIO_S16 (1)" in _err()
    assert down.last_kernel() == ""                              # nothing was launched


def test_the_pinned_ring_twin_refuses_pageable_memory_in_the_same_words():
    lib, rs = _lib.load(), Resampler(48000, 16000)
    x = torch.zeros(1024, dtype=torch.int16)
    kw = dict(x=c_void_p(x.data_ptr()), out=c_void_p(x.data_ptr()))
    assert _call(lib, "fe_resample_streams_pinned", rs._h, **kw) == FE_ERR_INVALID_ARG
    want = _err()
    assert _call(lib, "fe_resample_rings_pinned", rs._h, **kw) == FE_ERR_INVALID_ARG
    assert _err() == want.replace("fe_resample_streams_pinned", "fe_resample_rings_pinned")
    assert "fe_resample_rings_pinned: in is not page-locked host memory" in _err()


# ------------------------------------------------------------------ Resampler.step_rings*: host checks, then the device requirement
class _Pinned(torch.Tensor):
    """a CPU tensor that passes for page-locked memory (no CPU-only process can pin one)"""
    def is_pinned(self, *a, **kw):
        return True


class _Dev(torch.Tensor):
    """... and one that passes for a device tensor"""
    is_cuda = property(lambda self: True)


#         slot n_in in_base out_base in_len in_pos out_len out_pos      (x has 1024 elements, out 512)
GOOD = (0, 100, 0, 0, 449, 448, 149, 148)
BAD = [((0, 10, 0, 0, 449, 449, 149, 0), "input ring's position 449 is outside"),
       ((0, 10, 0, 0, 449, -1, 149, 0), "input ring's position -1 is outside"),
       ((0, 10, 0, 0, 449, 0, 149, 149), "output ring's position 149 is outside"),
       ((0, 10, 0, 0, 449, 0, 149, -1), "output ring's position -1 is outside"),
       ((0, 0, 0, 0, 0, 0, 149, 0), "input ring's length 0 is less than 1"),
       ((0, 10, 0, 0, 449, 0, 0, 0), "output ring's length 0 is less than 1"),
       ((0, 10, 0, 0, 449, 0, -5, 0), "output ring's length -5 is less than 1"),
       ((0, 450, 0, 0, 449, 0, 149, 0), "n_in 450 is more than the input ring's length 449"),
       ((0, 10, 576, 0, 449, 0, 149, 0), "input ring \\[576, 1025\\) is outside \\[0, 1024\\)"),
       ((0, 10, -1, 0, 449, 0, 149, 0), "input ring \\[-1, 448\\) is outside"),
       ((0, 10, 0, 364, 449, 0, 149, 0), "output ring \\[364, 513\\) is outside \\[0, 512\\)"),
       ((0, 10, 0, -1, 449, 0, 149, 0), "output ring \\[-1, 148\\) is outside"),
       ((4, 10, 0, 0, 449, 0, 149, 0), "slot 4 is outside"),
       ((-1, 10, 0, 0, 449, 0, 149, 0), "slot -1 is outside"),
       ((0, 961, 0, 0, 1024, 0, 512, 0), "n_in 961 is outside"),
       ((0, -1, 0, 0, 449, 0, 149, 0), "n_in -1 is outside")]


def test_step_rings_checks_list_descriptors_before_any_native_call(monkeypatch):
    rs = Resampler(48000, 16000)
    called = []
    for name in RING_FNS:
        monkeypatch.setattr(rs.lib, name, lambda *a, _n=name: called.append(_n) or 0)
    st = torch.zeros(4, rs.state_floats)
    for pinned, call in ((False, rs.step_rings), (True, rs.step_rings_pinned)):
        cls = _Pinned if pinned else _Dev
        x, out = torch.zeros(1024, dtype=torch.int16).as_subclass(cls), torch.zeros(512, dtype=torch.int16).as_subclass(cls)
        for row, msg in BAD:
            with pytest.raises(ValueError, match=msg):
                call(x, st, 4, [row], out, 960)
            with pytest.raises(ValueError, match=msg):          # ... wherever in the list the bad row stands
                call(x, st, 4, [(1,) + GOOD[1:], row], out, 960)
        with pytest.raises(ValueError, match="duplicate slots"):
            call(x, st, 4, [GOOD, GOOD], out, 960)
        with pytest.raises(ValueError, match="0 streams"):
            call(x, st, 4, [], out, 960)
        with pytest.raises(ValueError, match="a ring descriptor is"):
            call(x, st, 4, [(0, 10, 0, 0)], out, 960)
        with pytest.raises(ValueError, match="ring descriptor tensor"):
            call(x, st, 4, torch.zeros(1, 6, dtype=torch.int32), out, 960)
        # the buffer, n_in_max and produced checks of step_streams
        with pytest.raises(ValueError, match="n_in_max"):
            call(x, st, 4, [GOOD], out, 0)
        with pytest.raises(ValueError, match="produced must be a contiguous int32 tensor \\[1\\]"):
            call(x, st, 4, [GOOD], out, 960, produced=torch.zeros(2, dtype=torch.int32))
        with pytest.raises(ValueError, match="page-locked" if pinned else "device tensor"):
            call(torch.zeros(1024, dtype=torch.int16), st, 4, [GOOD], out, 960)
        with pytest.raises(ValueError, match="float32 or int16"):
            call(torch.zeros(4, dtype=torch.float64), st, 4, [GOOD], out, 960)
        with pytest.raises(_lib.FEError, match="needs a GPU"):           # a valid call gets as far as the device requirement
            call(x, st, 4, [GOOD, (1,) + GOOD[1:]], out, 960)
    assert called == []
    Resampler.check_ring_desc([GOOD], 4, 960, 1024, 512)


# ------------------------------------------------------------------ the two pools over one stub engine and stub resamplers
H = 256


class _Cfg:
    hop_size = H


class _StubEngine:
    """what PacketPool needs of an Engine; the launch is recorded and copies every launched input hop to its output place"""
    cfg = _Cfg()
    device = None

    def __init__(self, log):
        self.log, self.calls = log, []

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        pass

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        self.log.append("synchronize")

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1):
        self.log.append("step_streams_pinned")
        self.calls.append((capacity, list(desc), T_max))
        fin, fout = wav_in.view(-1), wav_out.view(-1)
        for slot, hops, i0, o0 in desc:
            fout[o0:o0 + hops * H] = fin[i0:i0 + hops * H]
        return wav_out


class _StubResampler:
    """the host formulas of the contract (resample_oracle); a step records itself, checks every descriptor by the kernel's rules and writes
    `produced` samples per stream, numbered from the stream's output count (so that a sample out of place shows)"""
    def __init__(self, log, sr_in, sr_out):
        self.log, self.tag = log, f"{sr_in}->{sr_out}"
        self.up, self.down = ro.ratio(sr_in, sr_out)
        self.state_floats = 8
        self.descs, self.wrapped = [], 0

    def out_count(self, n):
        return ro.out_count(n, self.up, self.down)

    def produced(self, consumed, n):
        return ro.emitted(consumed + n, self.up, self.down) - ro.emitted(consumed, self.up, self.down)

    def new_state(self, capacity):
        return torch.zeros(capacity, self.state_floats)

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        self.log.append("synchronize")

    def _emit(self, state, slot, n):
        consumed = int(state[slot, -1])
        made, first = self.produced(consumed, n), ro.emitted(consumed, self.up, self.down)
        state[slot, -1] = consumed + n
        state[slot, 0] = 1.0
        return made, (torch.arange(first, first + made) % 30000).to(torch.int16)

    def step_streams_pinned(self, x, state, capacity, desc, out, n_in_max, produced=None):
        self.log.append("step_streams_pinned")
        assert tuple(produced.shape) == (len(desc),)
        for i, (slot, n, i0, o0) in enumerate(desc):
            made, y = self._emit(state, slot, n)
            out.view(-1)[o0:o0 + made] = y
            produced[i] = made
        return out

    def step_rings_pinned(self, x, state, capacity, desc, out, n_in_max, produced=None):
        self.log.append("step_rings_pinned")
        self.descs.append(list(desc))
        assert tuple(produced.shape) == (len(desc),) and 1 <= len(desc) <= capacity
        assert len({d[0] for d in desc}) == len(desc)
        for i, (slot, n, in_base, out_base, in_len, in_pos, out_len, out_pos) in enumerate(desc):
            p = self.produced(int(state[slot, -1]), n)
            # the kernel's rules: a descriptor that broke one would be skipped without a word
            assert 0 <= slot < capacity and 0 <= n <= n_in_max
            assert in_len >= 1 and out_len >= 1 and 0 <= in_pos < in_len and 0 <= out_pos < out_len
            assert n <= in_len and p <= out_len
            assert 0 <= in_base and in_base + in_len <= x.numel() and 0 <= out_base and out_base + out_len <= out.numel()
            made, y = self._emit(state, slot, n)
            self.wrapped += out_pos + made > out_len
            idx = out_base + (out_pos + torch.arange(made)) % out_len
            out.view(-1)[idx] = y
            produced[i] = made
        return out


def _pools(monkeypatch, client_rate, **kw):
    """the oracle pool and the new one, each over a real PacketPool on a stub engine of its own"""
    made = {}
    for cls in (ResampledPacketPool, RingResampledPacketPool):
        log = []
        eng = _StubEngine(log)
        monkeypatch.setattr(cls, "_make_resampler", staticmethod(lambda a, b, device, _log=log: _StubResampler(_log, a, b)))
        made[cls] = (cls(eng, client_rate=client_rate, **kw), eng, log)
    return made[ResampledPacketPool], made[RingResampledPacketPool]


@pytest.mark.parametrize("client_rate", [48000, 8000])
def test_the_ring_pool_keeps_the_books_of_the_resampled_pool(monkeypatch, client_rate):
    """one seeded schedule - 3 slots, 40 ticks, 0 to 2 packets of 20 ms per slot and tick, one slot closed and reopened - through both pools"""
    packet = client_rate // 50
    (old, old_eng, _), (new, new_eng, log) = _pools(monkeypatch, client_rate, capacity=3, ring_hops=4, T_max=2, max_packet=2 * packet)
    assert isinstance(old.inner, PacketPool) and isinstance(new.inner, PacketPool)
    assert not hasattr(new, "_min") and not hasattr(new, "_mout")         # no model-rate staging

    def forbidden(*a, **k):
        raise AssertionError("the ring pool called push / pull of its inner pool")
    monkeypatch.setattr(new.inner, "push", forbidden)
    monkeypatch.setattr(new.inner, "pull", forbidden)
    rng = np.random.default_rng(20)
    slots = [(old.open(), new.open()) for _ in range(3)]
    assert [a for a, _ in slots] == [b for _, b in slots] == [0, 1, 2]
    full_ticks = refused = 0
    for tick in range(40):
        if tick == 17:
            old.close(1), new.close(1)
            assert old.active == new.active == [0, 2]
        if tick == 19:
            assert (old.open(), new.open()) == (1, 1)
        for slot in old.active:
            for _ in range(int(rng.integers(0, 3))):
                x = torch.from_numpy(rng.integers(-32768, 32768, size=packet, dtype=np.int16))
                try:
                    old.push(slot, x)
                except OverflowError as e:
                    with pytest.raises(OverflowError) as got:
                        new.push(slot, x)
                    assert str(got.value) == str(e)
                    refused += 1
                else:
                    new.push(slot, x)
        del log[:]
        pending = any(new._pending[s] for s in new.active)
        want = old.tick()
        assert new.tick() == want
        expect = (["step_rings_pinned"] if pending else []) + (["step_streams_pinned", "step_rings_pinned"] if want else []) \
            + (["synchronize"] if pending or want else [])
        assert log == expect, tick
        full_ticks += len(expect) == 4
        for slot in old.active:
            a, b = old.pull(slot), new.pull(slot)
            assert a.dtype == b.dtype == torch.int16 and torch.equal(a, b), (tick, slot)
        assert old._consumed == new._consumed and old._pending == new._pending and old._fill == new._fill
        for name in ("_pushed", "_stepped", "_pulled"):
            assert getattr(old.inner, name) == getattr(new.inner, name), name
    assert old_eng.calls == new_eng.calls and len(new_eng.calls) >= 30       # the inner engine calls, argument for argument
    assert torch.equal(old.state_in, new.state_in) and torch.equal(old.state_out, new.state_out)
    assert full_ticks >= 20 and log.count("synchronize") <= 1
    # the rings were used as rings: outputs of the first resampler wrapped in the inner input ring
    assert new.to_model.wrapped >= 3 and new.to_client.wrapped == 0
    assert all(d[5] == 0 and d[4] == new.max_packet for call in new.to_model.descs for d in call)          # flat client staging in ...
    assert all(d[7] == 0 and d[6] == new._client_cap for call in new.to_client.descs for d in call)         # ... and out


def test_the_ring_pool_refuses_what_the_resampled_pool_refuses_in_its_words(monkeypatch):
    (old, _, _), (new, _, _) = _pools(monkeypatch, 48000, capacity=2, ring_hops=2, max_packet=1000)
    for pool in (old, new):
        with pytest.raises(ValueError, match="slot 0 is not open"):
            pool.push(0, torch.zeros(4, dtype=torch.int16))
    with pytest.raises(ValueError, match="use PacketPool"):
        RingResampledPacketPool(_StubEngine([]), 2, 2, 16000)
    with pytest.raises(ValueError, match="max_packet"):
        RingResampledPacketPool(_StubEngine([]), 2, 2, 48000, max_packet=0)
    msgs = []
    for pool in (old, new):
        s = pool.open()
        with pytest.raises(ValueError, match="1-D int16"):
            pool.push(s, torch.zeros(4))
        pool.push(s, torch.zeros(600, dtype=torch.int16))
        with pytest.raises(OverflowError, match="max_packet = 1000") as e1:
            pool.push(s, torch.zeros(401, dtype=torch.int16))
        assert pool._pending[s] == 600                      # nothing of the refused packet was taken
        pool.push(s, torch.zeros(400, dtype=torch.int16))
        pool.tick()
        assert pool._fill[s] == 324 - 256                   # the inner ring (2 hops = 512 samples) after one hop
        pool.pull(s)
        # with the inner pool stalled the next 1000 client samples stay in its ring: 68 + 333 = 401 of 512
        monkeypatch.setattr(pool.inner, "tick", lambda: [])
        monkeypatch.setattr(pool.inner, "_enqueue", lambda: [])
        pool.push(s, torch.zeros(1000, dtype=torch.int16))
        pool.tick()
        assert pool._fill[s] == 401
        pool.push(s, torch.zeros(300, dtype=torch.int16))
        with pytest.raises(OverflowError, match="inner pool's ring holds 512") as e2:
            pool.push(s, torch.zeros(700, dtype=torch.int16))
        msgs.append((str(e1.value), str(e2.value)))
    assert msgs[0] == msgs[1]


def test_the_ring_pool_builds_the_inner_pool_it_is_given(monkeypatch):
    seen = []

    class _Inner(PacketPool):
        def __init__(self, engine, capacity, ring_hops, T_max=1, **kw):
            seen.append((capacity, ring_hops, T_max, kw))
            super().__init__(engine, capacity, ring_hops, T_max=T_max)
            self.backlog_hops = kw.get("backlog_hops", 0)
    monkeypatch.setattr(RingResampledPacketPool, "_make_resampler", staticmethod(lambda a, b, device: _StubResampler([], a, b)))
    pool = RingResampledPacketPool(_StubEngine([]), 3, 16, 48000, T_max=2, pool=_Inner, meters=True, backlog_hops=8)
    assert seen == [(3, 16, 2, dict(meters=True, backlog_hops=8))] and isinstance(pool.inner, _Inner)
    # a backlog launch advances up to 8 hops: the staging towards the client is sized for them, max_packet for an ordinary tick
    assert pool._step == 8 * H and pool._client_cap == 3 * 8 * H + 1 and pool.max_packet == 3 * 2 * H
