"""G.711 mu-law and A-law in the resampler on the GPU (FE_AUDIO_ULAW / FE_AUDIO_ALAW: fe_resample, fe_resample_streams[_pinned],
fe_resample_rings[_pinned], client_format= of the two resampled pools).

No tolerance anywhere: the int16 path is the oracle.  A G.711-input call equals the int16-input call on dec(bytes), a G.711-output call equals
enc() of the int16-output call (dec / enc: tests/g711_oracle.py, numpy from the contract's formulas), streams equal the whole-signal call,
rings equal the flat form, and bytes that are not a stream's keep their sentinel - to the byte, at every alignment of a row."""
import numpy as np
import pytest
import torch

import g711_oracle as go
from fastenhancer_amd import _lib
from fastenhancer_amd.engine import _ptr, _stream
from fastenhancer_amd.resample import Resampler
from fastenhancer_amd.serving import FamilyPacketPool, ResampledPacketPool, RingResampledPacketPool

pytestmark = pytest.mark.gpu

FMT = {"f32": _lib.FE_AUDIO_F32, "s16": _lib.FE_AUDIO_S16, "ulaw": 4, "alaw": 5}
SENT = 0xA5
_RS = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rs(sr_in, sr_out):
    if (sr_in, sr_out) not in _RS:
        _RS[(sr_in, sr_out)] = Resampler(sr_in, sr_out, _dev())
    return _RS[(sr_in, sr_out)]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _dec(b, law):
    """uint8 tensor (CPU) -> int16 tensor"""
    return torch.from_numpy(go.dec(b.numpy(), law))


def _enc(q, law):
    """int16 tensor (CPU) -> uint8 tensor"""
    return torch.from_numpy(go.enc(q.numpy(), law))


def _all_bytes(rows, n, seed):
    """rows x n bytes: all 256 values in a seeded shuffle per row, repeated to n"""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([np.resize(rng.permutation(256).astype(np.uint8), n) for _ in range(rows)]))


# ------------------------------------------------------------------ 1. whole signals, the input side
@pytest.mark.parametrize("law", go.LAWS)
@pytest.mark.parametrize("sr_out", [16000, 48000])
def test_whole_signals_of_bytes_equal_the_int16_call_on_the_decoded_bytes(sr_out, law):
    rs, dev = _rs(8000, sr_out), _dev()
    x = _all_bytes(3, 1000, seed=sr_out // 1000 + len(law))
    assert all(len(set(row.tolist())) == 256 for row in x)
    got = rs(x.to(dev), torch.float32, in_format=law)
    assert rs.last_kernel() == "fe_resample_kernel<whole,g711>"
    want = rs(_dec(x, law).to(dev), torch.float32)
    assert rs.last_kernel() == "fe_resample_kernel<whole>"
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, rs.out_count(1000)) and bool((got != 0).any())
    assert _same(got.cpu(), want.cpu())
    # ... and int16 by default
    assert _same(rs(x.to(dev), in_format=law).cpu(), rs(_dec(x, law).to(dev)).cpu())


# ------------------------------------------------------------------ 2. whole signals, the output side, every alignment
N_OUT = [1, 15, 16, 17, 31, 33, 1003]
ROWS = 17


def _float_rows(n, seed):
    """17 rows at peak 0.9 - a slow sine and noise, so that the low-pass keeps the level - and the last row scaled to 1.5: it clips on both sides"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32)
    phase = 2.0 * np.pi * torch.rand(ROWS, 1, generator=g)
    x = 0.6 * torch.sin(2.0 * np.pi * t / 97.0 + phase) + 0.3 * (2.0 * torch.rand(ROWS, n, generator=g) - 1.0)
    assert float(x.abs().max()) < 0.9001
    x[-1] *= 1.5
    return x


def _whole_raw(rs, x, out, out_stride, out_fmt):
    """fe_resample itself: rows of x -> rows of `out_stride` elements from out's first element"""
    B, n_in = x.shape
    _lib.check(rs.lib.fe_resample(rs._h, _ptr(x), n_in, FMT["f32"], n_in, _ptr(out), out_stride, FMT[out_fmt], B, _stream(_dev())), "fe_resample")


@pytest.mark.parametrize("sr_in", [16000, 48000])
def test_byte_rows_at_every_alignment_equal_the_encoded_int16_rows_and_nothing_else_is_written(sr_in):
    rs, dev = _rs(sr_in, 8000), _dev()
    clipped = {law: set() for law in go.LAWS}
    for n_out in N_OUT:
        n_in = n_out * rs.down // rs.up
        assert rs.out_count(n_in) == n_out
        x = _float_rows(n_in, seed=n_out).to(dev)
        s16 = torch.zeros(ROWS, n_out, dtype=torch.int16, device=dev)
        _whole_raw(rs, x, s16, n_out, "s16")
        q = s16.cpu()
        stride = n_out + 1
        bases = set()
        for law in go.LAWS:
            want = _enc(q, law)
            for off in range(16):                 # the buffer's first row at every alignment; the stride walks the rows over the others
                buf = torch.full((16 + ROWS * stride + 32,), SENT, dtype=torch.uint8, device=dev)
                assert buf.data_ptr() % 16 == 0
                _whole_raw(rs, x, buf[off:], stride, law)
                assert rs.last_kernel() == "fe_resample_kernel<whole,g711>"
                o = buf.cpu()
                rows = o[off:off + ROWS * stride].view(ROWS, stride)
                assert torch.equal(rows[:, :n_out], want), (n_out, law, off)
                assert bool((rows[:, n_out:] == SENT).all()) and bool((o[:off] == SENT).all()) and bool((o[off + ROWS * stride:] == SENT).all()), \
                    (n_out, law, off)
                bases |= {(off + b * stride) % 16 for b in range(ROWS)}
            clipped[law] |= set(want[-1].tolist())
        assert bases == set(range(16))
    # the clamp and both clipping codes occurred
    assert {0x80, 0x00} <= clipped["ulaw"] and {0xAA, 0x2A} <= clipped["alaw"]


# ------------------------------------------------------------------ 3. packet streams
SLOTS, CAPACITY = [4, 0, 2, 3], 6
SIZES = [0, 1, 7, 160, 33, 2, 95, 64]


@pytest.mark.parametrize("sr_in,sr_out", [(8000, 16000), (16000, 8000)])
def test_streams_of_bytes_are_the_whole_signal_calls_bytes_under_any_packetisation(sr_in, sr_out):
    """4 slots, 20 calls of seeded packet sizes (0 and 1 among them), mu-law in and A-law out; next to them an int16 run on dec(x) with a state
    table of its own; every call also names a slot out of range and a stream whose outputs would leave the buffer"""
    rs, dev = _rs(sr_in, sr_out), _dev()
    rng = np.random.default_rng(sr_in // 1000)
    calls = [[int(rng.choice(SIZES)) for _ in SLOTS] for _ in range(20)]
    calls[0], calls[1] = [0, 1, 7, 160], [1, 0, 160, 2]
    total = [sum(c[i] for c in calls) for i in range(len(SLOTS))]
    xs = _all_bytes(len(SLOTS), max(total), seed=7)
    n_in_max, cap_out = max(SIZES), rs.out_count(max(SIZES)) + 1
    # the whole-signal calls: bytes in, bytes out
    whole = rs(xs.to(dev), in_format="ulaw", out_format="alaw").cpu()
    assert whole.dtype == torch.uint8 and rs.last_kernel() == "fe_resample_kernel<whole,g711>"
    # odd offsets on both sides, so that no row is aligned by accident; one more stream's room for the bad descriptors
    in_off = [3 + i * (n_in_max + 1) for i in range(len(SLOTS) + 1)]
    out_off = [5 + i * (cap_out + 2) for i in range(len(SLOTS))]
    out_count = 5 + len(SLOTS) * (cap_out + 2)
    fin = torch.zeros(3 + (len(SLOTS) + 1) * (n_in_max + 1), dtype=torch.uint8, device=dev)
    fin16 = torch.zeros(fin.numel(), dtype=torch.int16, device=dev)
    fout = torch.empty(out_count, dtype=torch.uint8, device=dev)
    fout16 = torch.zeros(out_count, dtype=torch.int16, device=dev)
    state, state16 = rs.new_state(CAPACITY), rs.new_state(CAPACITY)
    state[5] = state16[5] = 777.0                 # the row of the stream that is skipped for its output range: plain data, and it stays
    state[5, rs.taps_per_output - 1:] = state16[5, rs.taps_per_output - 1:] = 0.0      # (a count of 0: the stream is checked, not refused for its count)
    produced = torch.full((len(SLOTS) + 2,), -7, dtype=torch.int32, device=dev)
    consumed = [0] * len(SLOTS)
    got = [[] for _ in SLOTS]
    for t, sizes in enumerate(calls):
        host = torch.zeros(fin.numel(), dtype=torch.uint8)
        for i, n in enumerate(sizes):
            host[in_off[i]:in_off[i] + n] = xs[i, consumed[i]:consumed[i] + n]
        host[in_off[-1]:in_off[-1] + n_in_max] = 0x11
        fin.copy_(host)
        fin16.copy_(_dec(host, "ulaw"))
        fout.fill_(SENT)
        rows = [(SLOTS[i], n, in_off[i], out_off[i]) for i, n in enumerate(sizes)]
        p_bad = rs.produced(0, n_in_max)
        assert p_bad >= 2
        bad = [(CAPACITY, n_in_max, in_off[-1], out_off[0]),                 # a slot out of range
               (5, n_in_max, in_off[-1], out_count - p_bad + 1)]             # outputs that end one byte past the buffer
        desc = Resampler.pack_desc(rows + bad).to(dev)
        rs.step_streams(fin, state, CAPACITY, desc, fout, n_in_max, produced=produced, in_format="ulaw", out_format="alaw")
        assert rs.last_kernel() == "fe_resample_kernel<streams,g711>"
        rs.step_streams(fin16, state16, CAPACITY, Resampler.pack_desc(rows).to(dev), fout16, n_in_max)
        assert rs.last_kernel() == "fe_resample_kernel<streams>"
        torch.cuda.synchronize()
        o, o16, p = fout.cpu(), fout16.cpu(), produced.cpu().tolist()
        assert p == [rs.produced(consumed[i], n) for i, n in enumerate(sizes)] + [0, 0], t
        written = torch.zeros(out_count, dtype=torch.bool)
        for i, n in enumerate(sizes):
            y = o[out_off[i]:out_off[i] + p[i]]
            assert torch.equal(y, _enc(o16[out_off[i]:out_off[i] + p[i]], "alaw")), (t, i)       # enc() of the int16 call on dec(x)
            got[i].append(y.clone())
            written[out_off[i]:out_off[i] + p[i]] = True
            consumed[i] += n
        assert bool((o[~written] == SENT).all()), "a byte outside the streams' ranges was written"
        assert _same(state.cpu(), state16.cpu()), t                            # the rows of the int16 run, the skipped streams' among them
    for i in range(len(SLOTS)):
        y = torch.cat(got[i])
        m = ro_emitted(rs, consumed[i])
        assert y.numel() == m > 0 and torch.equal(y, whole[i, :m]), i
    want5 = torch.full((rs.state_floats,), 777.0)
    want5[rs.taps_per_output - 1:] = 0.0
    assert _same(state[5].cpu(), want5) and not bool(state[1].any())


def ro_emitted(rs, n):
    """M(n): what a stream that has consumed n samples has emitted"""
    return rs.produced(0, n)


# ------------------------------------------------------------------ 4. rings
PAD = 5
RING_SIZES = [1, 7, 0, 26, 13, 3, 20]


def _ring_idx(base, length, pos, n):
    return base + (pos + torch.arange(n)) % length


def _ring_run(rs, xs, in_len, out_len, calls, fmt_in, fmt_out, pinned):
    """xs [3, N] (uint8 or int16) through step_rings[_pinned] - rings of in_len / out_len elements with PAD sentinels around each - and, packet
    for packet, through step_streams with the same formats on flat device buffers.  Checks every call; returns (outputs per stream, state)"""
    dev, n_streams = _dev(), xs.shape[0]
    law_in, law_out = (fmt_in if fmt_in in go.LAWS else None), (fmt_out if fmt_out in go.LAWS else None)
    dt_in, dt_out = xs.dtype, (torch.uint8 if law_out else torch.int16)
    sent_in, sent_out = (0x5A if law_in else 12345), (SENT if law_out else 12345)
    n_in_max = max(max(c) for c in calls)
    cap_out = rs.out_count(n_in_max) + 1
    make = (lambda n, dtype, fill: torch.full((n,), fill, dtype=dtype).pin_memory()) if pinned else (lambda n, dtype, fill: torch.full((n,), fill, dtype=dtype, device=dev))
    in_base = [PAD + i * (in_len + PAD) for i in range(n_streams)]
    out_base = [PAD + i * (out_len + PAD) for i in range(n_streams)]
    rin = make(PAD + n_streams * (in_len + PAD), dt_in, sent_in)
    rout = make(PAD + n_streams * (out_len + PAD), dt_out, sent_out)
    produced = make(n_streams, torch.int32, -7)
    state, flat_state = rs.new_state(n_streams), rs.new_state(n_streams)
    fin = torch.zeros(n_streams * n_in_max, dtype=dt_in, device=dev)
    fout = torch.zeros(n_streams * cap_out, dtype=dt_out, device=dev)
    fprod = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    consumed, in_pos, out_pos = [0] * n_streams, [0] * n_streams, [0] * n_streams
    wraps_in, wraps_out = [0] * n_streams, [0] * n_streams
    got = [[] for _ in range(n_streams)]
    call = rs.step_rings_pinned if pinned else rs.step_rings
    name = "fe_resample_kernel<ring,pinned,g711>" if pinned else "fe_resample_kernel<ring,g711>"
    for t, sizes in enumerate(calls):
        host_in = torch.zeros(n_streams * n_in_max, dtype=dt_in)
        ring_host = rin.cpu().clone()
        for i, n in enumerate(sizes):
            x = xs[i, consumed[i]:consumed[i] + n]
            host_in[i * n_in_max:i * n_in_max + n] = x
            ring_host[_ring_idx(in_base[i], in_len, in_pos[i], n)] = x
        fin.copy_(host_in)
        rin.copy_(ring_host)
        rs.step_streams(fin, flat_state, n_streams, [(i, n, i * n_in_max, i * cap_out) for i, n in enumerate(sizes)], fout, n_in_max, produced=fprod,
                        in_format=law_in, out_format=law_out)
        assert rs.last_kernel() == "fe_resample_kernel<streams,g711>"
        rout.fill_(sent_out)
        desc = [(i, n, in_base[i], out_base[i], in_len, in_pos[i], out_len, out_pos[i]) for i, n in enumerate(sizes)]
        call(rin, state, n_streams, desc, rout, n_in_max, produced=produced, in_format=law_in, out_format=law_out)
        torch.cuda.synchronize()
        assert rs.last_kernel() == name
        o, p, fo, fp = rout.cpu(), produced.cpu().tolist(), fout.cpu(), fprod.cpu().tolist()
        assert p == fp == [rs.produced(consumed[i], n) for i, n in enumerate(sizes)], t
        written = torch.zeros(o.numel(), dtype=torch.bool)
        for i, n in enumerate(sizes):
            idx = _ring_idx(out_base[i], out_len, out_pos[i], p[i])
            assert _same(o[idx], fo[i * cap_out:i * cap_out + p[i]]), (t, i)
            got[i].append(o[idx].clone())
            written[idx] = True
            wraps_in[i] += in_pos[i] + n > in_len
            wraps_out[i] += out_pos[i] + p[i] > out_len
            consumed[i], in_pos[i], out_pos[i] = consumed[i] + n, (in_pos[i] + n) % in_len, (out_pos[i] + p[i]) % out_len
        assert bool((o[~written] == sent_out).all()), "an element outside [pos, pos + p) lost its sentinel"
        assert _same(rin.cpu(), ring_host), "the input buffer changed"
        assert _same(state.cpu(), flat_state.cpu()), t
    return [torch.cat(g) for g in got], state.cpu(), wraps_in, wraps_out


RING_CASES = [(8000, 16000, "ulaw", "alaw", 37, 53), (16000, 8000, "alaw", "ulaw", 37, 19), (8000, 16000, "alaw", "s16", 37, 53),
              (16000, 8000, "s16", "ulaw", 37, 19)]


@pytest.mark.parametrize("sr_in,sr_out,fmt_in,fmt_out,in_len,out_len", RING_CASES, ids=[f"{a}-{b}-{fi}-{fo}" for a, b, fi, fo, _, _ in RING_CASES])
def test_byte_rings_equal_the_flat_form_and_pinned_rings_equal_device_rings(sr_in, sr_out, fmt_in, fmt_out, in_len, out_len):
    """rings of 37 and 53 (downwards: 19) elements - no multiples of 16 - that both wrap again and again; three streams with their cycles of sizes
    rotated"""
    rs = _rs(sr_in, sr_out)
    calls = [[RING_SIZES[(t + s) % len(RING_SIZES)] for s in (0, 3, 5)] for t in range(3 * len(RING_SIZES))]
    assert rs.out_count(max(RING_SIZES)) + 1 <= out_len and max(RING_SIZES) <= in_len
    n = sum(c[0] for c in calls)
    xs = _all_bytes(3, n, seed=sr_in // 1000 + len(fmt_in))
    if fmt_in == "s16":
        xs = _dec(xs, "ulaw")
    dev_run = _ring_run(rs, xs, in_len, out_len, calls, fmt_in, fmt_out, pinned=False)
    pin_run = _ring_run(rs, xs, in_len, out_len, calls, fmt_in, fmt_out, pinned=True)
    assert min(dev_run[2]) >= 2 and min(dev_run[3]) >= 2, dev_run[2:]      # every stream's packets and outputs straddled their ring's end
    for a, b in zip(dev_run[0], pin_run[0]):
        assert a.numel() == ro_emitted(rs, n) > 0 and _same(a, b)
    assert _same(dev_run[1], pin_run[1])


def test_a_wrap_inside_a_later_tile_of_bytes():
    """8 -> 16 kHz, one packet of 1200 bytes = three tiles (1024 outputs, 512 inputs each): the input ring wraps at sample 700, the output ring
    at output 1500 - both inside the second tile; each of the tile's two segments is split into head, body and tail on its own"""
    rs, dev = _rs(8000, 16000), _dev()
    n, in_len, out_len = 1200, 1203, 2411
    in_pos, out_pos = in_len - 700, out_len - 1500
    x = _all_bytes(1, 100 + n, seed=31)[0]
    state = rs.new_state(2)
    warm = torch.zeros(256, dtype=torch.uint8, device=dev)
    rs.step_streams(x[:100].to(dev), state, 2, [(1, 100, 0, 0)], warm, n, in_format="ulaw", out_format="ulaw")      # a live stream
    torch.cuda.synchronize()
    flat_state = state.clone()
    p = rs.produced(100, n)
    assert p > 2048 and 1024 < out_len - out_pos < 2048 and 512 < in_len - in_pos < 1024
    want = torch.zeros(p, dtype=torch.uint8, device=dev)
    rs.step_streams(x[100:].to(dev), flat_state, 2, [(1, n, 0, 0)], want, n, in_format="ulaw", out_format="ulaw")
    rin = torch.full((in_len + 2 * PAD,), 0x5A, dtype=torch.uint8)
    rin[_ring_idx(PAD, in_len, in_pos, n)] = x[100:]
    rout = torch.full((out_len + 2 * PAD,), SENT, dtype=torch.uint8, device=dev)
    made = torch.zeros(1, dtype=torch.int32, device=dev)
    rs.step_rings(rin.to(dev), state, 2, [(1, n, PAD, PAD, in_len, in_pos, out_len, out_pos)], rout, n, produced=made, in_format="ulaw", out_format="ulaw")
    torch.cuda.synchronize()
    assert made.cpu().tolist() == [p] and rs.last_kernel() == "fe_resample_kernel<ring,g711>"
    o, idx = rout.cpu(), _ring_idx(PAD, out_len, out_pos, p)
    assert torch.equal(o[idx], want.cpu()) and len(set(want.cpu().tolist())) > 100
    rest = torch.ones(o.numel(), dtype=torch.bool)
    rest[idx] = False
    assert int(rest.sum()) == out_len + 2 * PAD - p and bool((o[rest] == SENT).all())
    assert _same(state.cpu(), flat_state.cpu())


# ------------------------------------------------------------------ 5. the pools
def _drive3(law_pool, s16_pool, ring_pool, schedule, packet, sig, law):
    """one schedule through the three pools: every pull of the law pool is enc() of the s16 pool's, fed dec(bytes); the ring pool returns the law
    pool's bytes, tick lists and state tables"""
    pools = (law_pool, s16_pool, ring_pool)
    sent = {s: 0 for s in law_pool.active}
    ticks = pulled = 0
    for tick, (actions, pushes) in enumerate(schedule):
        for act, slot in actions:
            if act == "close":
                for p in pools:
                    p.close(slot)
            else:
                assert [p.open() for p in pools] == [slot] * 3
                sent[slot] = 0
        for slot, count in pushes:
            for _ in range(count):
                b = sig[slot, sent[slot]:sent[slot] + packet]
                sent[slot] += packet
                law_pool.push(slot, b), ring_pool.push(slot, b), s16_pool.push(slot, _dec(b, law))
        want = law_pool.tick()
        assert s16_pool.tick() == want and ring_pool.tick() == want, tick
        ticks += bool(want)
        for slot in law_pool.active:
            a, q, r = law_pool.pull(slot), s16_pool.pull(slot), ring_pool.pull(slot)
            assert a.dtype == r.dtype == torch.uint8 and q.dtype == torch.int16
            assert torch.equal(a, _enc(q, law)), (tick, slot, a.numel(), q.numel())
            assert torch.equal(r, a), (tick, slot, r.numel(), a.numel())
            pulled += a.numel()
    torch.cuda.synchronize()
    for other in (s16_pool, ring_pool):           # the rows are floats whatever the client's format
        assert _same(law_pool.state_in.cpu(), other.state_in.cpu()) and _same(law_pool.state_out.cpu(), other.state_out.cpu())
    assert bool(ring_pool.state_in.any()) and bool(ring_pool.state_out.any())
    assert law_pool.to_model.last_kernel() == law_pool.to_client.last_kernel() == "fe_resample_kernel<streams,pinned,g711>"
    assert ring_pool.to_model.last_kernel() == ring_pool.to_client.last_kernel() == "fe_resample_kernel<ring,pinned,g711>"
    assert s16_pool.to_model.last_kernel() == s16_pool.to_client.last_kernel() == "fe_resample_kernel<streams,pinned>"
    return ticks, pulled


@pytest.mark.parametrize("law", go.LAWS)
@pytest.mark.parametrize("name", ["fe_b", "fspen"])
def test_the_law_pools_return_the_encoded_samples_of_the_s16_pool(name, law):
    """8 kHz clients, 3 streams, 30 ticks of 20 ms packets with jitter: seeded empty ticks, one double packet, slot 1 closed at tick 6 and reopened
    at tick 8 (the model, the engines and the schedule of test_gpu_ring_resample.py's pool test)"""
    from test_gpu_ring_resample import _oracle_pool, _signal
    from test_gpu_step_chunk import _engine
    eng = _engine(name)
    client_rate, packet = 8000, 160
    kw = dict(capacity=3, ring_hops=4, client_rate=client_rate, T_max=2, max_packet=2 * packet)
    if name == "fspen":
        oracle = _oracle_pool(FamilyPacketPool, meters=True)
        law_pool, s16_pool = oracle(eng, client_format=law, **kw), oracle(eng, client_format="s16", **kw)
        ring_pool = RingResampledPacketPool(eng, pool=FamilyPacketPool, meters=True, client_format=law, **kw)
    else:
        law_pool, s16_pool = ResampledPacketPool(eng, client_format=law, **kw), ResampledPacketPool(eng, **kw)
        ring_pool = RingResampledPacketPool(eng, client_format=law, **kw)
    assert law_pool._cin.dtype == ring_pool._cout.dtype == torch.uint8 and s16_pool._cin.dtype == torch.int16
    rng = np.random.default_rng(11)
    schedule = []
    for tick in range(30):
        actions = [("close", 1)] if tick == 6 else [("open", 1)] if tick == 8 else []
        live = [0, 2] if tick in (6, 7) else [0, 1, 2]
        pushes = [(s, 2 if (tick, s) == (12, 2) else int(rng.random() > 0.12)) for s in live]
        schedule.append((actions, pushes))
    sig = _enc(_signal(3, 32 * packet, seed=41, dtype=torch.int16, peak=0.3), law)
    for s in range(3):
        assert [p.open() for p in (law_pool, s16_pool, ring_pool)] == [s] * 3
    ticks, pulled = _drive3(law_pool, s16_pool, ring_pool, schedule, packet, sig, law)
    assert ticks >= 20 and pulled > 50 * packet


# ------------------------------------------------------------------ 6. nothing moved
def test_the_other_calls_on_a_handle_that_ran_g711_report_and_compute_what_a_fresh_handle_does():
    dev = _dev()
    used, fresh = Resampler(8000, 16000, dev), Resampler(8000, 16000, dev)
    b = _all_bytes(2, 300, seed=3)
    s16 = _dec(b, "alaw")
    f32 = s16.to(torch.float32) / 32768.0

    def pinned(t):
        return t.clone().pin_memory()

    def forms(rs, g711):
        """one call of each of the five forms; g711: bytes in and out, else int16 in / float out and float in / int16 out in turn"""
        out, names = [], []
        kw = dict(in_format="alaw", out_format="ulaw") if g711 else {}
        for x, odt in ((b, torch.uint8),) if g711 else ((s16, torch.float32), (f32, torch.int16)):
            out.append(rs(x.to(dev), None if g711 else odt, **kw).cpu())
            names.append(rs.last_kernel())
            n, p = x.shape[1], rs.produced(0, x.shape[1])
            for pin in (False, True):
                for ring in (False, True):
                    src = pinned(x.reshape(-1)) if pin else x.reshape(-1).to(dev)
                    dst = pinned(torch.zeros(2 * p, dtype=odt)) if pin else torch.zeros(2 * p, dtype=odt, device=dev)
                    desc = [(i, n, i * n, i * p, n, 0, p, 0) for i in range(2)] if ring else [(i, n, i * n, i * p) for i in range(2)]
                    call = getattr(rs, ("step_rings" if ring else "step_streams") + ("_pinned" if pin else ""))
                    call(src, rs.new_state(2), 2, desc, dst, n, **kw)
                    torch.cuda.synchronize()
                    out.append(dst.cpu().clone())
                    names.append(rs.last_kernel())
        return out, names

    _, g_names = forms(used, g711=True)
    assert g_names == ["fe_resample_kernel<whole,g711>", "fe_resample_kernel<streams,g711>", "fe_resample_kernel<ring,g711>",
                       "fe_resample_kernel<streams,pinned,g711>", "fe_resample_kernel<ring,pinned,g711>"]
    got, names = forms(used, g711=False)
    want, want_names = forms(fresh, g711=False)
    assert names == want_names == 2 * ["fe_resample_kernel<whole>", "fe_resample_kernel<streams>", "fe_resample_kernel<ring>",
                                       "fe_resample_kernel<streams,pinned>", "fe_resample_kernel<ring,pinned>"]
    for a, w in zip(got, want):
        assert bool((a != 0).any()) and _same(a, w)
