"""fe_step_pool_streams[_pinned] on the GPU: the packet step of BSRNN, FSPEN and LiSenNet (Engine.step_pool_streams*, PacketPool).

Every stream of a call advances its own number of hops at its own offsets, in float32 or int16 PCM.  Each stream's rows and state must be those
of fe_step_pool(T = its hops) on the same slot - bit for bit wherever that call dispatches the same kernel functions (decided here by comparing
the two fe_last_step_kernel strings with the words `streams`, `pinned`, `s16` taken out of the brackets), else within TIGHT_REL["bsrnn"] (a
BSRNN stream with one hop inside a T_max > 1 call: the generic walk against the per-hop kernels).  Nothing else may change: no state of a
stream without a hop or of a slot not named, no sample outside the ranges the descriptors name - also when the descriptors point outside the
buffers.  Models: bsrnn_xxt (both PART 1 kernels), bsrnn_s (64 channels), fspen, lisennet; states seeded non-zero by four fe_step hops."""
import re

import numpy as np
import pytest
import torch

from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool
from test_gpu_parity import TIGHT_REL, _assert_close
from test_gpu_step_chunk import _dev, _engine, _same, _seeded_state
from test_gpu_step_pool import MODELS, _dense
from test_gpu_stream_packets import _audio, _desc, _kernel, _quantise

pytestmark = pytest.mark.gpu

CASES = [("bsrnn_xxt", "wg8"), ("bsrnn_xxt", "waves4"), ("bsrnn_s", "wg8"), ("fspen", "wg8"), ("lisennet", "wg8")]
SENT = {torch.float32: 123.25, torch.int16: 12345}


def _strip(k):
    """a kernel list with the packet step's words taken out of the brackets: what fe_step_pool names the same kernel functions"""
    return re.sub(r", (streams|pinned|s16)\b", "", k)


def _packet(eng, pinned):
    return eng.step_pool_streams_pinned if pinned else eng.step_pool_streams


def _sized(eng, cap):
    """fe_state_init for `cap` streams: the scratch of BSRNN's three-launch step holds every call of the test (the steps allocate nothing)"""
    eng.init_state(eng.new_state(cap), cap)


def _twin(eng, full, cap, slot, x_rows):
    """fe_step_pool(T = hops) of one stream on a dense twin holding the record of `slot`: (rows [1, hops*H], record, kernel names)"""
    hops = x_rows.numel() // eng.cfg.hop_size
    dense = _dense(eng, full, cap, [slot])
    y = eng.step_pool(x_rows.reshape(1, -1).to(_dev()).contiguous(), dense, 1, [0], T=hops)
    k = eng.last_step_kernel()
    torch.cuda.synchronize()
    return y, eng.export_slots(dense, 1, [0]), k


def _check_stream(eng, name, what, y, rec, k, twin):
    """the equality rule of the header: equal bits where fe_step_pool ran the same kernel functions, else BSRNN's bound"""
    ty, trec, tk = twin
    if _strip(k) == tk:
        assert _same(y.reshape(1, -1), ty), f"{what}: output differs from fe_step_pool ({k})"
        assert _same(rec, trec), f"{what}: record differs from fe_step_pool ({k})"
        return True
    assert name.startswith("bsrnn") and y.numel() == eng.cfg.hop_size and "generic" in k and "generic" not in tk, (what, k, tk)
    _assert_close(y.reshape(1, -1).cpu().numpy(), ty.cpu().numpy(), f"{what} wav_out", tight=TIGHT_REL["bsrnn"])
    _assert_close(rec.cpu().numpy(), trec.cpu().numpy(), f"{what} record", tight=TIGHT_REL["bsrnn"])
    return False


def _names_ok(k):
    assert "slots" in k and "streams" in k, k
    for bad in ("_sb_", "fused", "time-pipelined"):
        assert bad not in k, k


# ------------------------------------------------------------------ 1. ragged hop counts
@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("name,kern", CASES)
def test_ragged_hop_counts_equal_fe_step_pool_of_each_count(name, kern, pinned):
    eng = _engine(name)
    cap, slots, hops, TM, H = 6, [4, 0, 5, 2], [2, 0, 3, 1], 3, _engine(name).cfg.hop_size
    in_off, out_off, total = [5000, 20, 9000, 13000], [11000, 3000, 40, 7000], 16000
    with _kernel(eng, kern):
        _sized(eng, cap)
        full = _seeded_state(eng, cap, 4, seed=11)
        x = 0.1 * torch.randn(4, TM * H, generator=torch.Generator().manual_seed(12))
        big_in = _audio((total,), torch.float32, pinned, fill=SENT[torch.float32])
        for i in range(4):
            big_in[in_off[i]:in_off[i] + TM * H] = x[i]
        big_out = _audio((total,), torch.float32, pinned, fill=SENT[torch.float32])
        st = full.clone()
        _packet(eng, pinned)(big_in, st, cap, _desc([(slots[i], hops[i], in_off[i], out_off[i]) for i in range(4)]), big_out, T_max=TM)
        k = eng.last_step_kernel()
        torch.cuda.synchronize()
        _names_ok(k)
        assert ("pinned" in k) == pinned and "s16" not in k and ("generic" in k or not name.startswith("bsrnn")), k
        exact = []
        for i in range(4):
            if hops[i]:
                twin = _twin(eng, full, cap, slots[i], x[i, :hops[i] * H])
                y = big_out[out_off[i]:out_off[i] + hops[i] * H].to(_dev())
                exact.append(_check_stream(eng, name, f"stream {i} ({hops[i]} hops)", y, eng.export_slots(st, cap, [slots[i]]), k, twin))
    assert exact == ([True, True, False] if name.startswith("bsrnn") else [True] * 3), exact      # only BSRNN's 1-hop stream runs another kernel
    keep = [0, 1, 3]                                                     # the 0-hop slot and the two slots not named
    assert _same(eng.export_slots(st, cap, keep), eng.export_slots(full, cap, keep)), "a slot the call does not advance changed"
    written = torch.zeros(total, dtype=torch.bool)
    for i in range(4):
        written[out_off[i]:out_off[i] + hops[i] * H] = True
    assert bool((big_out.cpu()[~written] == SENT[torch.float32]).all()), "an output element outside the written ranges lost the sentinel"
    assert bool((big_out.cpu()[written] != SENT[torch.float32]).all())


# ------------------------------------------------------------------ 2. T_max = 1, hops in {0, 1}: BSRNN's three launches
def _three_launches(name, kern, k):
    if not name.startswith("bsrnn"):
        return
    parts = k.split(" + ")
    first = "bsrnn_ov_kernel<slots, streams" if (name == "bsrnn_xxt" and kern == "wg8") else "bsrnn_frame_kernel<PART 1, slots, streams"
    assert len(parts) == 3 and parts[0].startswith(first) and parts[1].startswith("bsrnn_mlp_kernel") and \
        parts[2].startswith("bsrnn_frame_kernel<PART 2, slots, streams"), k


def _ticks_of_zero_and_one_hop(name, kern, ticks, poison=False, dtype=torch.float32):
    """capacity 5, four descriptors, two of them without a hop, changing from tick to tick; every tick checked against the twins"""
    eng = _engine(name)
    cap, slots, H = 5, [3, 0, 4, 1], eng.cfg.hop_size
    results = []
    with _kernel(eng, kern):
        _sized(eng, cap)
        full = _seeded_state(eng, cap, 4, seed=13)
        x = 0.1 * torch.randn(ticks, 4, H, generator=torch.Generator().manual_seed(14))
        for t in range(ticks):
            hops = [1 if (i + t) % 4 in (0, 3) else 0 for i in range(4)] if t % 3 != 2 else [1 if (i + t) % 2 else 0 for i in range(4)]
            assert sum(hops) == 2
            before = full.clone()
            xin = x[t].to(_dev()).contiguous()
            out = torch.full((4, H), SENT[torch.float32], device=_dev())
            if poison:
                eng.poison_lds()
            eng.step_pool_streams(xin.view(-1), full, cap, _desc([(slots[i], hops[i], i * H, i * H) for i in range(4)]), out.view(-1), T_max=1)
            k = eng.last_step_kernel()
            torch.cuda.synchronize()
            _names_ok(k)
            _three_launches(name, kern, k)
            for i in range(4):
                rec = eng.export_slots(full, cap, [slots[i]])
                if hops[i]:
                    assert _check_stream(eng, name, f"tick {t} stream {i}", out[i], rec, k, _twin(eng, before, cap, slots[i], x[t, i])), "T_max = 1: equal bits"
                else:
                    assert _same(rec, eng.export_slots(before, cap, [slots[i]])), f"tick {t}: the state of stream {i} (0 hops) changed"
                    assert bool((out[i] == SENT[torch.float32]).all()), f"tick {t}: the output range of stream {i} (0 hops) was written"
            assert _same(eng.export_slots(full, cap, [2]), eng.export_slots(before, cap, [2])), f"tick {t}: the slot not named changed"
            results.append((out.clone(), full.clone()))
    return results


@pytest.mark.parametrize("name,kern", CASES)
def test_zero_and_one_hop_ticks_run_the_per_hop_kernels(name, kern):
    _ticks_of_zero_and_one_hop(name, kern, 6)


# ------------------------------------------------------------------ 3. offsets
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("TM", [1, 2])
@pytest.mark.parametrize("name", MODELS)
def test_unaligned_offsets_give_the_bits_of_the_aligned_dense_layout(name, TM, dtype):
    eng = _engine(name)
    cap, slots, H = 8, [6, 1, 7, 3], eng.cfg.hop_size
    row, n, total = TM * H, 4, 16000
    in_off, out_off = [10001, 7, 5003, 2481], [6001, 9003, 13, 3001]        # odd element offsets: no multiple of 4 (f32) or 8 (s16)
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=15)
    x = _audio((n, row), dtype, False, gen=torch.Generator().manual_seed(16))
    big_in = _audio((total,), dtype, False, fill=SENT[dtype])
    for i in range(n):
        big_in[in_off[i]:in_off[i] + row] = x[i]
    big_in0 = big_in.clone()
    big_out = _audio((total,), dtype, False, fill=SENT[dtype])
    ref_st, st = full.clone(), full.clone()
    ref = _audio((n, row), dtype, False, fill=SENT[dtype])
    eng.step_pool_streams(x.view(-1), ref_st, cap, _desc([(slots[i], TM, i * row, i * row) for i in range(n)]), ref.view(-1), T_max=TM)
    k_ref = eng.last_step_kernel()
    eng.step_pool_streams(big_in, st, cap, _desc([(slots[i], TM, in_off[i], out_off[i]) for i in range(n)]), big_out, T_max=TM)
    assert eng.last_step_kernel() == k_ref and ("s16" in k_ref) == (dtype == torch.int16)
    torch.cuda.synchronize()
    want = _audio((total,), dtype, False, fill=SENT[dtype])
    for i in range(n):
        want[out_off[i]:out_off[i] + row] = ref[i]
    assert torch.equal(big_out.view(torch.int16), want.view(torch.int16)), "output rows or the sentinels around them differ"
    assert torch.equal(big_in.view(torch.int16), big_in0.view(torch.int16)), "the input buffer was written"
    assert _same(st, ref_st)
    assert float(ref.float().abs().max()) > 0 and not _same(st, full)


# ------------------------------------------------------------------ 4. int16 PCM
@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("name,TM", [("bsrnn_xxt", 1), ("bsrnn_xxt", 2), ("bsrnn_s", 1), ("fspen", 2), ("lisennet", 1)])
def test_int16_pcm_is_the_float_call_on_s_over_32768_quantised_on_the_way_out(name, TM, pinned):
    eng = _engine(name)
    cap, slots, H = 6, [5, 0, 2, 3], eng.cfg.hop_size
    n, hops = 4, [TM, max(TM - 1, 1), TM, TM]
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=17)
    s = _audio((n, TM * H), torch.int16, pinned, gen=torch.Generator().manual_seed(18), scale=0.25)
    s.view(-1)[:8] = torch.tensor([32767, -32768, 0, 1, -1, 16384, -16384, 12345], dtype=torch.int16)
    xf = _audio((n, TM * H), torch.float32, pinned, fill=0.0)
    xf.copy_(s.float() / 32768.0)
    d = _desc([(slots[i], hops[i], i * TM * H, i * TM * H) for i in range(n)])
    st_f, st_s = full.clone(), full.clone()
    yf = _audio((n, TM * H), torch.float32, pinned, fill=0.0)
    ys = _audio((n, TM * H), torch.int16, pinned, fill=-999)
    _packet(eng, pinned)(xf.view(-1), st_f, cap, d, yf.view(-1), T_max=TM)
    k_f = eng.last_step_kernel()
    _packet(eng, pinned)(s.view(-1), st_s, cap, d, ys.view(-1), T_max=TM)
    k_s = eng.last_step_kernel()
    torch.cuda.synchronize()
    assert "s16" in k_s and ("pinned" in k_s) == pinned and re.sub(r", s16\b", "", k_s) == k_f, (k_s, k_f)
    assert _same(st_f, st_s), "the state after the int16 call is not the float call's"
    want = torch.full_like(ys, -999)
    for i in range(n):
        want[i, :hops[i] * H] = _quantise(yf[i, :hops[i] * H])
    bad = (want != ys).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} samples differ, first at {bad[0].tolist()}: {int(ys[tuple(bad[0])])} vs {int(want[tuple(bad[0])])}"
    assert float(torch.cat([want[i, :hops[i] * H] for i in range(n)]).float().abs().mean()) > 10, "the streams should not be silent"


# ------------------------------------------------------------------ 5. descriptors that point outside
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("name,kern,TM", [("bsrnn_xxt", "wg8", 1), ("bsrnn_xxt", "waves4", 1), ("bsrnn_xxt", "wg8", 3), ("bsrnn_s", "wg8", 1),
                                          ("fspen", "wg8", 1), ("fspen", "wg8", 3), ("lisennet", "wg8", 1), ("lisennet", "wg8", 3)])
def test_bad_descriptors_touch_nothing_outside_the_buffers(name, kern, TM, dtype):
    """the call is told a count smaller than the allocation, whose base pointers sit G elements inside it, and every bad offset is smaller
    than G in size: taken unchecked it would still land in memory this test owns - a missing check shows as a changed sentinel, not as a fault"""
    eng = _engine(name)
    H, cap = eng.cfg.hop_size, 16
    row = TM * H
    count, G = 12 * row, 2 * (TM + 5) * H + 64
    with _kernel(eng, kern):
        _sized(eng, cap)
        full = _seeded_state(eng, cap, 4, seed=19)
        alloc_in = _audio((count + 2 * G,), dtype, False, gen=torch.Generator().manual_seed(20))
        alloc_out = _audio((count + 2 * G,), dtype, False, fill=SENT[dtype])
        win, wout = alloc_in[G:G + count], alloc_out[G:G + count]
        in0 = alloc_in.clone()
        rows = [
            (3, TM, 0, 0),                                  # 0: good
            (4, 1, count - H + 1, 1 * row),                 # 1: input range ends one element past count
            (5, 1, 1 * row, count - H + 1),                 # 2: output range ends one element past count
            (6, 1, -7, 2 * row),                            # 3: negative input offset
            (7, 1, 2 * row, -1),                            # 4: negative output offset
            (8, -3, 3 * row, 3 * row),                      # 5: negative hop count: none
            (9, TM + 5, 4 * row, 4 * row),                  # 6: too many hops: T_max of them
            (cap + 2, 1, 5 * row, 5 * row),                 # 7: slot out of range: one zero row
            (-1, TM, 6 * row, 6 * row),                     # 8: slot out of range: T_max zero rows
            (10, TM, count - row + 1, 7 * row),             # 9: T_max hops whose input range ends one element past count
            (11, TM, 8 * row, count - row + 1),             # 10: ... whose output range does
            (14, TM, count - row, count - row),             # 11: good: the last rows of both buffers
        ]
        assert all(-G < r[2] and r[2] + (TM + 5) * H <= count + G and -G < r[3] and r[3] + (TM + 5) * H <= count + G for r in rows)
        st = full.clone()
        eng.step_pool_streams(win, st, cap, _desc(rows), wout, T_max=TM)
        k = eng.last_step_kernel()
        ref_st = full.clone()
        ref_alloc = _audio((count + 2 * G,), dtype, False, fill=SENT[dtype])
        good = [(3, TM, 0, 0), (9, TM, 4 * row, 4 * row), (14, TM, count - row, count - row)]
        eng.step_pool_streams(win, ref_st, cap, _desc(good), ref_alloc[G:G + count], T_max=TM)
        assert eng.last_step_kernel() == k
        torch.cuda.synchronize()
    ref_alloc[G + 5 * row:G + 5 * row + H] = 0
    ref_alloc[G + 6 * row:G + 7 * row] = 0
    assert torch.equal(alloc_out.view(torch.int16), ref_alloc.view(torch.int16)), "output: a row, a skipped stream's place or a guard region differs"
    assert torch.equal(alloc_in.view(torch.int16), in0.view(torch.int16))
    assert _same(st, ref_st), "a skipped stream or an out-of-range slot touched the state"
    untouched = [s for s in range(cap) if s not in (3, 9, 14)]
    assert _same(eng.export_slots(st, cap, untouched), eng.export_slots(full, cap, untouched)) and not _same(st, full)


# ------------------------------------------------------------------ 6. above the streams resident at once
@pytest.mark.parametrize("name", ["bsrnn_xxt", "lisennet"])
def test_the_persistent_walk_above_the_resident_count(name):
    eng = _engine(name)
    n = 2 * torch.cuda.get_device_properties(_dev()).multi_processor_count + 5
    cap, H = n + 3, eng.cfg.hop_size
    rng = np.random.default_rng(21)
    slots = [int(s) for s in rng.permutation(cap)[:n]]
    idle = set(int(i) for i in rng.permutation(n)[:5])
    hops = [0 if i in idle else 1 for i in range(n)]
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=22)
    x = (0.1 * torch.randn(n, H, generator=torch.Generator().manual_seed(23))).to(_dev())
    out = torch.full((n, H), SENT[torch.float32], device=_dev())
    st = full.clone()
    eng.step_pool_streams(x.view(-1), st, cap, _desc([(slots[i], hops[i], i * H, i * H) for i in range(n)]), out.view(-1), T_max=1)
    k = eng.last_step_kernel()
    act = [i for i in range(n) if hops[i]]
    ref_st = full.clone()
    ref = eng.step_pool(x[act].contiguous(), ref_st, cap, [slots[i] for i in act])
    k_ref = eng.last_step_kernel()
    torch.cuda.synchronize()
    _names_ok(k)
    assert _strip(k) == k_ref and ("two workgroups per CU" in k or name == "lisennet"), (k, k_ref)
    assert _same(out[act], ref), f"output differs (max {float((out[act] - ref).abs().max()):.3e})"
    assert bool((out[sorted(idle)] == SENT[torch.float32]).all()), "a stream without a hop was written"
    assert _same(st, ref_st), "the state differs from fe_step_pool on the streams that advanced"
    assert not _same(st, full)


# ------------------------------------------------------------------ 7. graph capture
def test_pinned_int16_in_a_captured_graph_follows_descriptors_and_rings():
    """bsrnn_xxt, T_max = 1: a linear chain of three kernels, replayed with descriptors and rings rewritten between replays"""
    eng = _engine("bsrnn_xxt")
    dev = _dev()
    cap, n, H, R = 8, 5, eng.cfg.hop_size, 4 * eng.cfg.hop_size
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=24)
    twin = full.clone()
    ring_in, ring_out = _audio((cap, R), torch.int16, True, fill=0), _audio((cap, R), torch.int16, True, fill=0)
    e_in, e_out = _audio((cap, R), torch.int16, True, fill=0), _audio((cap, R), torch.int16, True, fill=0)
    d = _desc([(i, 1, i * R, i * R) for i in range(n)])
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):                                           # warm-up: function attributes - nothing allocates in the capture
            eng.step_pool_streams_pinned(ring_in, twin.clone(), cap, d, ring_out, T_max=1)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step_pool_streams_pinned(ring_in, full, cap, d, ring_out, T_max=1)
    k = eng.last_step_kernel()
    _three_launches("bsrnn_xxt", "wg8", k)
    assert "pinned, s16" in k, k
    rng = np.random.default_rng(25)
    gen = torch.Generator().manual_seed(26)
    for r in range(3):
        sl = [int(v) for v in rng.permutation(cap)[:n]]
        rows = [(sl[i], int(rng.integers(0, 2)) if i else 1, sl[i] * R + int(rng.integers(0, 4)) * H, sl[i] * R + int(rng.integers(0, 4)) * H) for i in range(n)]
        d.copy_(Engine.pack_stream_desc(rows))
        ring_in.copy_((0.1 * torch.randn(cap, R, generator=gen) * 32768).round().to(torch.int16))
        ring_out.fill_(r)
        e_in.copy_(ring_in)
        e_out.fill_(r)
        graph.replay()
        eng.step_pool_streams_pinned(e_in, twin, cap, rows, e_out, T_max=1)
        torch.cuda.synchronize()
        assert torch.equal(ring_out, e_out), f"replay {r}"
        assert _same(full, twin), f"replay {r}: state"
        assert int((ring_out != r).sum()) > 0


# ------------------------------------------------------------------ 8. end to end: PacketPool
@pytest.mark.parametrize("name", ["fspen", "bsrnn_xxt"])
def test_packet_pool_with_jittered_20ms_packets_equals_each_stream_run_alone(name):
    """three streams, T_max = 1 (every launched stream runs the per-hop kernels fe_step runs), moved to a second pool in the middle"""
    eng = _engine(name)
    dev, H = _dev(), eng.cfg.hop_size
    n_streams, ticks, packet = 3, 40, 320                            # 20 ms at 16 kHz against a hop of 256 samples
    rng = np.random.default_rng(27)
    arrivals = rng.choice([0, 1, 1, 1, 2], size=(ticks, n_streams))  # packets per stream and tick: none, one, or a burst
    total = int(arrivals.sum(0).max()) * packet
    pcm = (0.2 * torch.randn(n_streams, total, generator=torch.Generator().manual_seed(28)) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    pool = PacketPool(eng, 4, ring_hops=16, T_max=1)
    other = PacketPool(eng, 5, ring_hops=24, T_max=1)
    home = [(pool, pool.open()) for _ in range(n_streams)]
    sent, got = [0] * n_streams, [[] for _ in range(n_streams)]
    for t in range(ticks):
        if t == ticks // 2:                                          # streams 0 and 2 move, in flight samples and all
            for i in (2, 0):
                home[i] = (other, pool.move(home[i][1], other))
        for i in rng.permutation(n_streams):
            for _ in range(int(arrivals[t, i])):
                p, s = home[i]
                p.push(s, pcm[i, sent[i]:sent[i] + packet])
                sent[i] += packet
        for p in (pool, other):
            if p.tick():
                k = eng.last_step_kernel()
                assert "slots, streams, pinned, s16" in k and "_sb_" not in k, k
        for i, (p, s) in enumerate(home):
            got[i].append(p.pull(s))
    for i in range(n_streams):
        y = torch.cat(got[i])
        hops = y.numel() // H
        assert y.numel() % H == 0 and hops > 20 and y.numel() <= sent[i]
        solo = eng.new_state(1)
        x = (pcm[i, :hops * H].float() / 32768.0).to(dev)
        ref = torch.cat([eng.step(x[k * H:(k + 1) * H].reshape(1, H), solo)[0] for k in range(hops)])
        want = _quantise(ref).cpu()
        bad = (want != y).nonzero()
        assert bad.numel() == 0, f"stream {i}: {bad.shape[0]} of {y.numel()} samples differ, first at {int(bad[0])}"


# ------------------------------------------------------------------ 9. LDS poison
@pytest.mark.parametrize("name,kern", CASES)
def test_what_lds_held_before_does_not_matter(name, kern):
    plain = _ticks_of_zero_and_one_hop(name, kern, 1)
    poisoned = _ticks_of_zero_and_one_hop(name, kern, 1, poison=True)
    assert _same(plain[0][0], poisoned[0][0]) and _same(plain[0][1], poisoned[0][1]), "the result depends on what was in LDS before the launch"
    assert bool(torch.isfinite(poisoned[0][1]).all())
