"""The resampler's ring form on the GPU (fe_resample_rings[_pinned] through Resampler.step_rings[_pinned]) and serving.RingResampledPacketPool.

The oracle of the kernel is the flat form, fe_resample_streams, fed the same packets: the ring form differs in addresses only, so its
outputs - un-wrapped on the host - its state rows and its `produced` are the flat call's, bit for bit; elements it has no business with keep
their sentinels.  The oracle of the pool is ResampledPacketPool on the same schedule: every pull, every tick() return, both state tables."""
import numpy as np
import pytest
import torch

import resample_oracle as ro
from fastenhancer_amd.resample import Resampler
from fastenhancer_amd.serving import BacklogPacketPool, FamilyPacketPool, PacketPool, ResampledPacketPool, RingResampledPacketPool

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (16000, 48000), (16000, 44100), (16000, 8000)]
OUT_LEN = {(48000, 16000): 149, (8000, 16000): 883, (44100, 16000): 163, (16000, 48000): 1327, (16000, 44100): 1217, (16000, 8000): 223}
SENT = {torch.float32: 123.25, torch.int16: 12345}
CYCLE = [1, 7, 0, 160, 441, 3, 64]
SHIFTS = [0, 3, 5]           # the streams' cycles rotated against each other
SLOTS, CAPACITY, IN_LEN, PAD = [5, 0, 2], 6, 449, 5
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


def _signal(rows, n, seed, dtype=torch.float32, peak=0.5):
    x = (2.0 * torch.rand(rows, n, generator=torch.Generator().manual_seed(seed)) - 1.0) * peak
    return x if dtype == torch.float32 else torch.round(x * 32768.0).to(torch.int16)


def _is_prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def _sizes(step):
    return [CYCLE[(step + s) % len(CYCLE)] for s in SHIFTS]


def wrap_counts(up, down, K, in_len, out_len, steps):
    """From the contract's M(N) alone: per stream, the calls whose packet wrapped in the input ring and those whose outputs wrapped in the output
    ring; and, over all streams, the packets whose last K - 1 samples straddled the input wrap"""
    ins, outs, straddles = [0] * len(SHIFTS), [0] * len(SHIFTS), 0
    for i in range(len(SHIFTS)):
        consumed = in_pos = out_pos = 0
        for t in range(steps):
            n = _sizes(t)[i]
            p = ro.emitted(consumed + n, up, down) - ro.emitted(consumed, up, down)
            ins[i] += in_pos + n > in_len
            outs[i] += out_pos + p > out_len
            straddles += in_pos + n - min(n, K - 1) < in_len < in_pos + n
            consumed, in_pos, out_pos = consumed + n, (in_pos + n) % in_len, (out_pos + p) % out_len
    return ins, outs, straddles


def _put_ring(buf, base, length, pos, x):
    idx = base + (pos + torch.arange(x.numel())) % length
    buf[idx] = x


def _ring_idx(base, length, pos, n):
    return base + (pos + torch.arange(n)) % length


def _ring_run(rs, xs, out_len, steps, dtype_in, dtype_out, pinned=False):
    """xs [3, N] through step_rings[_pinned] (rings of IN_LEN / out_len elements, PAD sentinels around each) and, packet for packet, through
    step_streams on flat device buffers - the oracle.  Checks every call; returns (ring outputs per stream, final ring state)"""
    n_streams, n_in_max = len(SLOTS), max(CYCLE)
    cap_out = rs.out_count(n_in_max) + 1
    dev = _dev()
    make = (lambda n, dtype, fill: torch.full((n,), fill, dtype=dtype).pin_memory()) if pinned else (lambda n, dtype, fill: torch.full((n,), fill, dtype=dtype, device=dev))
    in_base = [PAD + i * (IN_LEN + PAD) for i in range(n_streams)]
    out_base = [PAD + i * (out_len + PAD) for i in range(n_streams)]
    rin = make(PAD + n_streams * (IN_LEN + PAD), dtype_in, SENT[dtype_in])
    rout = make(PAD + n_streams * (out_len + PAD), dtype_out, SENT[dtype_out])
    produced = make(n_streams, torch.int32, -7)
    state, flat_state = rs.new_state(CAPACITY), rs.new_state(CAPACITY)
    for s in range(CAPACITY):
        if s not in SLOTS:
            state[s] = flat_state[s] = 777.0
    fin = torch.zeros(n_streams * n_in_max, dtype=dtype_in, device=dev)
    fout = torch.zeros(n_streams * cap_out, dtype=dtype_out, device=dev)
    fprod = torch.zeros(n_streams, dtype=torch.int32, device=dev)
    consumed, in_pos, out_pos = [0] * n_streams, [0] * n_streams, [0] * n_streams
    got = [[] for _ in range(n_streams)]
    call = rs.step_rings_pinned if pinned else rs.step_rings
    for t in range(steps):
        sizes = _sizes(t)
        # the oracle: flat buffers, the same packets
        host_in = torch.zeros(n_streams * n_in_max, dtype=dtype_in)
        ring_host = rin.cpu()
        for i, n in enumerate(sizes):
            x = xs[i, consumed[i]:consumed[i] + n]
            host_in[i * n_in_max:i * n_in_max + n] = x
            _put_ring(ring_host, in_base[i], IN_LEN, in_pos[i], x)
        fin.copy_(host_in)
        rin.copy_(ring_host)
        rs.step_streams(fin, flat_state, CAPACITY, [(SLOTS[i], n, i * n_in_max, i * cap_out) for i, n in enumerate(sizes)], fout, n_in_max, produced=fprod)
        rout.fill_(SENT[dtype_out])
        desc = [(SLOTS[i], n, in_base[i], out_base[i], IN_LEN, in_pos[i], out_len, out_pos[i]) for i, n in enumerate(sizes)]
        call(rin, state, CAPACITY, desc, rout, n_in_max, produced=produced)
        torch.cuda.synchronize()
        assert rs.last_kernel() == ("fe_resample_kernel<ring,pinned>" if pinned else "fe_resample_kernel<ring>")
        o, p, fo, fp = rout.cpu(), produced.cpu().tolist(), fout.cpu(), fprod.cpu().tolist()
        assert p == fp == [rs.produced(consumed[i], n) for i, n in enumerate(sizes)], t
        written = torch.zeros(o.numel(), dtype=torch.bool)
        for i, n in enumerate(sizes):
            idx = _ring_idx(out_base[i], out_len, out_pos[i], p[i])
            assert _same(o[idx], fo[i * cap_out:i * cap_out + p[i]]), (t, i)
            got[i].append(o[idx].clone())
            written[idx] = True
            consumed[i], in_pos[i], out_pos[i] = consumed[i] + n, (in_pos[i] + n) % IN_LEN, (out_pos[i] + p[i]) % out_len
        assert bool((o[~written] == SENT[dtype_out]).all()), "an element outside the written ranges lost its sentinel"
        assert _same(rin.cpu(), ring_host), "the input buffer changed"
        assert _same(state.cpu(), flat_state.cpu()), t
    return [torch.cat(g) for g in got], state.cpu()


CASES = [(a, b, torch.int16, torch.int16) for a, b in PAIRS] + [(48000, 16000, torch.float32, torch.int16), (48000, 16000, torch.int16, torch.float32)]


@pytest.mark.parametrize("sr_in,sr_out,dtype_in,dtype_out", CASES, ids=[f"{a}-{b}-{'s16' if di == torch.int16 else 'f32'}-{'s16' if do == torch.int16 else 'f32'}"
                                                                         for a, b, di, do in CASES])
def test_the_ring_form_equals_the_flat_form_bit_for_bit(sr_in, sr_out, dtype_in, dtype_out):
    rs = _rs(sr_in, sr_out)
    out_len = OUT_LEN[(sr_in, sr_out)]
    least = rs.out_count(max(CYCLE)) + 1
    assert _is_prime(out_len) and out_len >= least and not any(_is_prime(q) for q in range(least, out_len))      # the smallest prime >= out_count(441) + 1
    steps = 3 * len(CYCLE)
    ins, outs, straddles = wrap_counts(rs.up, rs.down, rs.taps_per_output, IN_LEN, out_len, steps)
    assert min(ins) >= 3 and min(outs) >= 3 and straddles >= 1, (ins, outs, straddles)
    xs = _signal(len(SLOTS), steps * max(CYCLE), seed=sr_in // 100 + sr_out // 1000, dtype=dtype_in, peak=0.9)
    got, _ = _ring_run(rs, xs, out_len, steps, dtype_in, dtype_out)
    for i, g in enumerate(got):
        assert g.numel() == ro.emitted(3 * sum(CYCLE), rs.up, rs.down) and bool((g != 0).any()), i


def test_a_wrap_inside_a_later_tile():
    """48 -> 16 kHz, one packet of 5000 samples = two tiles (1024 outputs, 3072 inputs each): the input ring wraps at sample 4000, the output
    ring at output 1300 - both inside the second tile"""
    rs, dev = _rs(48000, 16000), _dev()
    n, in_len, out_len, in_pos, out_pos = 5000, 5003, 1699, 1003, 399
    x = _signal(1, 100 + n, seed=31, dtype=torch.int16, peak=0.9)[0]
    state = rs.new_state(2)
    warm = torch.zeros(64, dtype=torch.int16, device=dev)
    rs.step_streams(x[:100].to(dev), state, 2, [(1, 100, 0, 0)], warm, n)             # a live stream: 100 samples consumed
    torch.cuda.synchronize()
    flat_state = state.clone()
    p = rs.produced(100, n)
    assert p > 1024 and out_pos + 1024 < out_len < out_pos + p and in_pos + 3072 < in_len < in_pos + n
    want = torch.zeros(p, dtype=torch.int16, device=dev)
    rs.step_streams(x[100:].to(dev), flat_state, 2, [(1, n, 0, 0)], want, n)
    rin = torch.full((in_len + 2 * PAD,), SENT[torch.int16], dtype=torch.int16)
    _put_ring(rin, PAD, in_len, in_pos, x[100:])
    rout = torch.full((out_len + 2 * PAD,), SENT[torch.int16], dtype=torch.int16, device=dev)
    made = torch.zeros(1, dtype=torch.int32, device=dev)
    rs.step_rings(rin.to(dev), state, 2, [(1, n, PAD, PAD, in_len, in_pos, out_len, out_pos)], rout, n, produced=made)
    torch.cuda.synchronize()
    assert made.cpu().tolist() == [p]
    o, idx = rout.cpu(), _ring_idx(PAD, out_len, out_pos, p)
    assert _same(o[idx], want.cpu())
    rest = torch.ones(o.numel(), dtype=torch.bool)
    rest[idx] = False
    assert bool((o[rest] == SENT[torch.int16]).all())
    assert _same(state.cpu(), flat_state.cpu())


def test_bad_ring_descriptors_touch_nothing():
    rs, dev = _rs(48000, 16000), _dev()
    cap, n_in_max, in_count, out_count, margin = 16, 460, 1200, 600, 100
    x = _signal(1, in_count, seed=6, dtype=torch.int16)[0]
    big_in = torch.full((in_count + 2 * margin,), SENT[torch.int16], dtype=torch.int16)
    big_in[margin:margin + in_count] = x
    big_in = big_in.to(dev)
    big_out = torch.full((out_count + 2 * margin,), SENT[torch.int16], dtype=torch.int16, device=dev)
    state = rs.new_state(cap)
    warm = torch.zeros(cap * 100, dtype=torch.int16, device=dev)
    rs.step_streams(big_in[margin:margin + 300].contiguous(), state, cap, [(s, 300, 0, s * 100) for s in range(cap)], warm, 300)      # every row a live stream
    torch.cuda.synchronize()
    before = state.clone()
    p300, p460 = rs.produced(300, 300), rs.produced(300, 460)
    assert p300 == 100 and p460 > 149
    IB, IL, IP, OB, OL, OP = 50, 449, 400, 400, 149, 100           # a ring pair every bad case would be served on, but for its one fault
    cases = [(0, 300, IB, OB, 0, 0, OL, OP),                       # in_len = 0
             (1, 300, IB, OB, IL, IL, OL, OP),                     # in_pos = in_len
             (2, 300, IB, OB, IL, -1, OL, OP),                     # in_pos = -1
             (3, IL + 1, IB, OB, IL, IP, OL, OP),                  # n_in = in_len + 1 (within n_in_max)
             (4, 300, IB, OB, IL, IP, p300 - 1, 0),                # p = out_len + 1
             (5, 300, in_count - IL + 1, OB, IL, IP, OL, OP),      # the input ring ends one element past its buffer
             (6, 300, IB, out_count - OL + 1, IL, IP, OL, OP),     # the output ring ends one element past its buffer
             (7, 300, -1, OB, IL, IP, OL, OP),                     # negative bases
             (8, 300, IB, -1, IL, IP, OL, OP),
             (-1, 300, IB, OB, IL, IP, OL, OP),                    # slot outside [0, capacity)
             (cap, 300, IB, OB, IL, IP, OL, OP),
             (9, 300, IB, OB, IL, IP, 0, 0),                       # out_len = 0
             (10, 300, IB, OB, IL, IP, OL, OL),                    # out_pos = out_len
             (11, 100000, 600, 200, 500, 450, 199, 150),           # n_in above n_in_max: runs as n_in_max, both rings wrapping
             (12, 300, IB, 10, IL, IP, OL, OP)]                    # a valid stream, both rings wrapping
    assert IL + 1 <= n_in_max
    desc = Resampler.pack_ring_desc(cases).to(dev)
    produced = torch.full((len(cases),), -7, dtype=torch.int32, device=dev)
    view_in, view_out = big_in[margin:margin + in_count], big_out[margin:margin + out_count]
    rs.step_rings(view_in, state, cap, desc, view_out, n_in_max, produced=produced)
    torch.cuda.synchronize()
    assert produced.cpu().tolist() == [0] * 13 + [p460, p300]
    rest = [s for s in range(cap) if s not in (11, 12)]
    assert _same(state[rest].cpu(), before[rest].cpu()), "the state of a skipped stream changed"
    # the two served streams ran as the flat call runs them on the samples their rings hold
    o = big_out.cpu()[margin:margin + out_count].clone()
    written = torch.zeros(out_count, dtype=torch.bool)
    for slot, n, ib, il, ip, ob, ol, op, p in ((11, n_in_max, 600, 500, 450, 200, 199, 150, p460), (12, 300, IB, IL, IP, 10, OL, OP, p300)):
        twin = before.clone()
        want = torch.zeros(p, dtype=torch.int16, device=dev)
        rs.step_streams(x[_ring_idx(ib, il, ip, n)].to(dev), twin, cap, [(slot, n, 0, 0)], want, n_in_max)
        torch.cuda.synchronize()
        idx = _ring_idx(ob, ol, op, p)
        assert _same(o[idx], want.cpu()) and _same(state[slot].cpu(), twin[slot].cpu()), slot
        written[idx] = True
    assert bool((o[~written] == SENT[torch.int16]).all()), "an element outside the two valid ranges was written"
    full = big_out.cpu()
    assert bool((full[:margin] == SENT[torch.int16]).all()) and bool((full[margin + out_count:] == SENT[torch.int16]).all())
    want_in = torch.full((in_count + 2 * margin,), SENT[torch.int16], dtype=torch.int16)
    want_in[margin:margin + in_count] = x
    assert _same(big_in.cpu(), want_in)


def test_pinned_rings_equal_device_rings_bit_for_bit():
    rs = _rs(48000, 16000)
    steps = 2 * len(CYCLE)
    xs = _signal(len(SLOTS), steps * max(CYCLE), seed=8, dtype=torch.int16, peak=0.9)
    dev = _ring_run(rs, xs, 149, steps, torch.int16, torch.int16, pinned=False)       # (names fe_resample_kernel<ring> ...
    pin = _ring_run(rs, xs, 149, steps, torch.int16, torch.int16, pinned=True)        # ... and <ring,pinned>: asserted call by call)
    for a, b in zip(dev[0], pin[0]):
        assert a.numel() > 0 and _same(a, b)
    assert _same(dev[1], pin[1])
    with pytest.raises(ValueError, match="page-locked"):
        rs.step_rings_pinned(torch.zeros(8, dtype=torch.int16), rs.new_state(1), 1, [(0, 8, 0, 0, 8, 0, 8, 0)], torch.zeros(8, dtype=torch.int16), 8)


# ------------------------------------------------------------------ the pool
def _oracle_pool(inner_cls, step_hops=None, **inner_kw):
    """ResampledPacketPool over another inner pool class, by its _make_pool hook.  Its model-rate staging towards the client is sized for T_max
    hops a tick; over an inner pool that serves backlogs of step_hops > T_max hops the oracle's two buffers on that side are made again for
    step_hops (nothing else of it changes)."""
    class _Oracle(ResampledPacketPool):
        @staticmethod
        def _make_pool(engine, capacity, ring_hops, T_max):
            return inner_cls(engine, capacity, ring_hops, T_max=T_max, **inner_kw)

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            if step_hops is not None:
                self._step = step_hops * self.inner.H
                self._client_cap = self.to_client.out_count(self._step) + 1
                self._mout = self.to_client.new_pinned(self.capacity, self._step, dtype=torch.int16)
                self._cout = self.to_client.new_pinned(self.capacity, self._client_cap, dtype=torch.int16)
    return _Oracle


def _drive(old, new, schedule, packet, sig, check_levels):
    """one schedule - per tick (close / open actions, packets per slot) - through both pools, whose first slots are open: every tick()
    return and every pull compared, the state tables at the end"""
    sent = {s: 0 for s in old.active}
    returns = []
    for tick, (actions, pushes) in enumerate(schedule):
        for act, slot in actions:
            if act == "close":
                old.close(slot), new.close(slot)
            else:
                assert (old.open(), new.open()) == (slot, slot)
                sent[slot] = 0
        for slot, count in pushes:
            for _ in range(count):
                x = sig[slot, sent[slot]:sent[slot] + packet]
                sent[slot] += packet
                old.push(slot, x), new.push(slot, x)
        want = old.tick()
        got = new.tick()
        assert got == want, tick
        returns.append(got)
        for slot in old.active:
            a, b = old.pull(slot), new.pull(slot)
            assert _same(a, b), (tick, slot, a.numel(), b.numel())
            if check_levels:
                assert old.inner.levels(slot) == new.inner.levels(slot), (tick, slot)
    torch.cuda.synchronize()
    assert _same(old.state_in.cpu(), new.state_in.cpu()) and _same(old.state_out.cpu(), new.state_out.cpu())
    assert bool(new.state_in.any()) and bool(new.state_out.any())
    assert new.to_model.last_kernel() == new.to_client.last_kernel() == "fe_resample_kernel<ring,pinned>"
    return returns


@pytest.mark.parametrize("client_rate", [48000, 8000])
@pytest.mark.parametrize("name", ["fe_b", "fspen"])
def test_the_ring_pool_equals_the_resampled_pool_bit_for_bit(name, client_rate):
    """30 ticks of 20 ms packets with jitter: seeded empty ticks, one double packet, slot 1 closed at tick 6 and reopened at tick 8"""
    from test_gpu_step_chunk import _engine
    eng = _engine(name)
    packet = client_rate // 50
    kw = dict(capacity=3, ring_hops=4, client_rate=client_rate, T_max=2, max_packet=2 * packet)
    if name == "fspen":
        old = _oracle_pool(FamilyPacketPool, meters=True)(eng, **kw)
        new = RingResampledPacketPool(eng, pool=FamilyPacketPool, meters=True, **kw)
        assert type(new.inner) is type(old.inner) is FamilyPacketPool
    else:
        old, new = ResampledPacketPool(eng, **kw), RingResampledPacketPool(eng, **kw)
        assert type(new.inner) is type(old.inner) is PacketPool
    rng = np.random.default_rng(11)
    schedule = []
    for tick in range(30):
        actions = [("close", 1)] if tick == 6 else [("open", 1)] if tick == 8 else []
        live = [0, 2] if tick in (6, 7) else [0, 1, 2]
        pushes = [(s, 2 if (tick, s) == (12, 2) else int(rng.random() > 0.12)) for s in live]
        schedule.append((actions, pushes))
    assert sum(c == 0 for _, p in schedule for _, c in p) >= 3
    sig = _signal(3, 32 * packet, seed=41, dtype=torch.int16, peak=0.3)
    for s in range(3):
        assert (old.open(), new.open()) == (s, s)
    if name == "fspen":                                 # limits, meters, banks: through the inner pool, whose slots are the same numbers
        old.inner.set_suppression_limit(2, -12.0), new.inner.set_suppression_limit(2, -12.0)
    returns = _drive(old, new, schedule, packet, sig, check_levels=name == "fspen")
    assert sum(1 for r in returns if r) >= 20
    ring = new.inner.ring
    for slot in new.active:
        assert new.inner._stepped[slot] >= 3 * ring, (slot, new.inner._stepped[slot])        # the inner rings wrapped at least 3 times
        assert new.inner._stepped == old.inner._stepped


def test_the_ring_pool_over_a_backlog_pool_serves_a_backlog():
    """bsrnn_xxt, backlog_hops = 8: six ordinary ticks, a stall of 8 ticks without a packet, then two double packets at once - 5 hops, more than
    T_max = 2: they leave in the backlog launch - and six more ticks"""
    from test_gpu_step_chunk import _engine
    eng = _engine("bsrnn_xxt")
    packet = 960
    kw = dict(capacity=2, ring_hops=16, client_rate=48000, T_max=2, max_packet=4 * packet)
    old = _oracle_pool(BacklogPacketPool, step_hops=8, backlog_hops=8)(eng, **kw)
    new = RingResampledPacketPool(eng, pool=BacklogPacketPool, backlog_hops=8, **kw)
    assert type(new.inner) is type(old.inner) is BacklogPacketPool and new.inner.backlog_hops == 8 and new._step == old._step == 8 * 256
    for s in range(2):
        assert (old.open(), new.open()) == (s, s)
    schedule = [([], [(0, 1), (1, 1)]) for _ in range(6)] + [([], [(1, 1)]) for _ in range(8)] + [([], [(0, 4), (1, 1)])] + [([], [(0, 1), (1, 1)]) for _ in range(6)]
    sig = _signal(2, 24 * packet, seed=43, dtype=torch.int16, peak=0.3)
    returns = _drive(old, new, schedule, packet, sig, check_levels=False)
    burst = [d for d in returns[14] if d[0] == 0]
    assert len(burst) == 1 and 2 < burst[0][1] <= 8, returns[14]          # slot 0's backlog: one launch of more than T_max hops
    assert all(hops <= 2 for t, r in enumerate(returns) if t != 14 for _, hops, _, _ in r)
