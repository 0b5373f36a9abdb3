"""The packet step's time-pipelined form on the GPU (fe_step_streams_chunk[_pinned] through Engine.step_streams_chunk* and
PacketPool(backlog_hops=)).

The call means fe_step_streams_banked[_pinned] with the same arguments: on the pipeline each stream's hops run on co-resident workgroups
and stream_ola_streams_kernel overlap-adds them, which agrees with the serial packet step to fp32 rounding - output rows and every state
tensor of the stepped slots - leaves cache_stft (a copy of input samples) bit-identical and touches nothing else: no slot it does not
advance, no sample outside the rows its descriptors name.  Where nothing is pipelined it is the serial step bit for bit.

Bounds.  PIPE_REL = 3e-5 of the reference's largest magnitude: the bound of tests/test_gpu_step_chunk.py and the pipelined-vs-serial tests
of tests/test_gpu_parity.py.  int16 rows: |q_chunk - q_serial| <= 1 + ceil(PIPE_REL * max|y| * 32768) LSB (one for the rounding of either
side, the rest the float bound in LSB).

The core case names seven descriptors, so its state has seven slots (a call takes at most `capacity` descriptors): (slot, hops) = (5, 9),
(0, 1), (3, 0), (2, 4), (1, 2), (7, 3) - slot 7 has no state - and (6, 2) whose input range ends past in_count, which is skipped; slot 4 is
not named.  1 and 2 hops of fe_m (hop 160, N - H = 352 > 2 H) do not cover the overlap: the new caches hold shifted old cache values."""
import math

import numpy as np
import pytest
import torch

from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool
from test_gpu_stream_packets import _audio, _desc
from test_gpu_stream_slots import _dev, _engine, _same, _seeded_state, _views

pytestmark = pytest.mark.gpu

PIPE_REL = 3e-5
MODELS = ["fe_t", "fe_b", "fe_ln_b", "fe_dprnn_b", "fe_m", "fe48_b_h480"]
SENTINEL = -77.0
TM = 9
CAP = 7
ROWS = [(5, 9), (0, 1), (3, 0), (2, 4), (1, 2), (7, 3), (6, 2)]      # (slot, hops); the last one is skipped by the bounds check
PADS = [1, 0, 3, 8, 5, 2, 7]                                           # element offsets of the rows inside their strides: odd, and 16-byte aligned ones
SKIPPED, STATELESS = 6, 5                                              # indices into ROWS
LIVE = [0, 1, 3, 4]                                                    # ... of the streams that advance


def _chunk(eng, pinned):
    return eng.step_streams_chunk_pinned if pinned else eng.step_streams_chunk


def _serial(eng, pinned):
    return eng.step_streams_pinned if pinned else eng.step_streams


def _lsb_bound(ref_q):
    """1 + ceil(PIPE_REL * max|y| * 32768) with max|y| = max|q| / 32768"""
    return 1 + math.ceil(PIPE_REL * float(ref_q.abs().max()))


def _assert_rows_close(got, ref, dtype, what):
    """output samples of one row: the float bound, or the int16 bound in LSB"""
    if dtype == torch.int16:
        diff, bound = int((got.int() - ref.int()).abs().max()), _lsb_bound(ref.float())
        print(f"{what}: max |q_chunk - q_serial| {diff} LSB, bound {bound}")
        assert diff <= bound, f"{what}: {diff} LSB > {bound}"
    else:
        diff, scale = float((got - ref).abs().max()), float(ref.abs().max())
        print(f"{what}: max abs diff {diff:.3e}, scale {scale:.3e}, ratio {diff / max(scale, 1e-30):.3e}")
        assert torch.isfinite(got).all() and diff <= PIPE_REL * scale, f"{what}: {diff:.3e} > {PIPE_REL:.0e} x {scale:.3e}"


def _assert_state_close(eng, cap, got, ref, slots, what):
    """cache_stft of the stepped slots bit for bit, every other state tensor of them within PIPE_REL of the reference's largest magnitude"""
    idx = torch.tensor(slots, device=got.device)
    vg, vr = _views(eng, got, cap), _views(eng, ref, cap)
    assert _same(vg[0][idx], vr[0][idx]), f"{what}: cache_stft differs"
    for j, (a, b) in enumerate(zip(vg[1:], vr[1:]), 1):
        a, b = a[idx], b[idx]
        diff, scale = float((a - b).abs().max()), float(b.abs().max())
        print(f"{what}: state tensor {j}: max abs diff {diff:.3e}, scale {scale:.3e}")
        assert torch.isfinite(a).all() and diff <= PIPE_REL * scale, f"{what}: state tensor {j}: {diff:.3e} > {PIPE_REL:.0e} x {scale:.3e}"


def _core_layout(eng, dtype, pinned, seed=11):
    """the core case's buffers and descriptors: rows of TM * H samples at stride TM * H + 40 with a pad of their own in front"""
    H = eng.cfg.hop_size
    stride = TM * H + 40
    count = len(ROWS) * stride
    x = _audio((count,), dtype, pinned, gen=torch.Generator().manual_seed(seed))
    offs = [i * stride + PADS[i] for i in range(len(ROWS))]
    rows = [(s, h, offs[i], offs[i]) for i, (s, h) in enumerate(ROWS)]
    rows[SKIPPED] = (ROWS[SKIPPED][0], ROWS[SKIPPED][1], count - H, offs[SKIPPED])         # two hops from count - H: past the input's end
    return x, rows, offs, count


def _fill(dtype):
    return 7.0 if dtype == torch.float32 else 777


def _run_core(eng, full, dtype, pinned, fn, levels=None, rows_override=None):
    x, rows, offs, count = _core_layout(eng, dtype, pinned)
    st, y = full.clone(), _audio((count,), dtype, pinned, fill=_fill(dtype))
    kw = {} if levels is None else dict(levels=levels)
    fn(x, st, CAP, _desc(rows_override or rows), y, T_max=TM, **kw)
    k = eng.last_step_kernel()
    torch.cuda.synchronize()
    return x, rows, offs, st, y, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("name", MODELS)
def test_chunk_equals_the_serial_packet_step_and_leaves_a_valid_state(name, pinned, dtype):
    eng = _engine(name)
    H = eng.cfg.hop_size
    full = _seeded_state(eng, CAP, hops=4)
    x, rows, offs, st, y, k = _run_core(eng, full, dtype, pinned, _chunk(eng, pinned))
    _, _, _, st_ref, y_ref, k_ref = _run_core(eng, full, dtype, pinned, _serial(eng, pinned))
    assert "time-pipelined" in k and "streams" in k and "stream_ola_streams_kernel" in k, k
    assert ("pinned" in k) == pinned and ("s16" in k) == (dtype == torch.int16) and "banks" not in k, k
    assert "time-pipelined" not in k_ref
    # rows: the live streams within the bound, the stateless stream's exact zeros, every other byte untouched
    y, y_ref = y.cpu(), y_ref.cpu()
    written = torch.zeros(y.numel(), dtype=torch.bool)
    for i in LIVE + [STATELESS]:
        lo, n = offs[i], ROWS[i][1] * H
        written[lo:lo + n] = True
        if i == STATELESS:
            assert int((y[lo:lo + n] != 0).sum()) == 0 and int((y_ref[lo:lo + n] != 0).sum()) == 0, "a stream without state gets zero rows"
        else:
            _assert_rows_close(y[lo:lo + n], y_ref[lo:lo + n], dtype, f"{name} stream {i} ({ROWS[i][1]} hops)")
    assert bool((y[~written] == _fill(dtype)).all()), "a sample outside the rows of the streams that advanced was written"
    assert bool((y_ref[~written] == _fill(dtype)).all())
    # state: stepped slots close, everything else bit for bit
    live_slots = [ROWS[i][0] for i in LIVE]
    _assert_state_close(eng, CAP, st, st_ref, live_slots, name)
    still = torch.tensor([4, 3, ROWS[SKIPPED][0]], device=st.device)
    for j, (a, b) in enumerate(zip(_views(eng, st, CAP), _views(eng, full, CAP))):
        assert _same(a[still], b[still]), f"state tensor {j} of a slot the call does not advance changed"
    assert not _same(st, full)
    # continuation: two ordinary one-hop ticks on both states
    g = torch.Generator().manual_seed(12)
    d1 = _desc([(s, 1, i * H, i * H) for i, s in enumerate(live_slots)])
    for t in range(2):
        x1 = _audio((len(live_slots) * H,), dtype, pinned, gen=g)
        outs = []
        for state in (st, st_ref):
            y1 = _audio((len(live_slots) * H,), dtype, pinned, fill=_fill(dtype))
            _serial(eng, pinned)(x1, state, CAP, d1, y1, T_max=1)
            torch.cuda.synchronize()
            outs.append(y1.cpu())
        _assert_rows_close(outs[0], outs[1], dtype, f"{name} continuation hop {t}")
        _assert_state_close(eng, CAP, st, st_ref, live_slots, f"{name} after continuation hop {t}")


def test_chunk_is_reproducible_bit_for_bit():
    eng = _engine("fe_b")
    full = _seeded_state(eng, CAP, hops=4)
    runs = []
    for _ in range(2):
        lv = torch.full((CAP, 4), SENTINEL, device=_dev())
        _, _, _, st, y, k = _run_core(eng, full, torch.int16, False, eng.step_streams_chunk, levels=lv)
        assert "time-pipelined" in k
        runs.append((y, st, lv))
    assert torch.equal(runs[0][0], runs[1][0]), "output bytes differ between two runs"
    assert _same(runs[0][1], runs[1][1]), "state floats differ between two runs"
    assert _same(runs[0][2], runs[1][2]), "level rows differ between two runs"
    assert int((runs[0][2] != SENTINEL).all(dim=1).sum()) == len(LIVE)


# ------------------------------------------------------------------ controls: the suppression limit and the level meters
def test_chunk_applies_the_limit_to_the_output_path_only_and_meters_like_the_serial_step():
    eng = _engine("fe_b")
    H, cap, T = eng.cfg.hop_size, 8, 6
    gains = [0.0, 0.25, 1.0]
    full = _seeded_state(eng, cap, hops=4)
    n_in = 6 * T * H
    s = _audio((n_in,), torch.int16, False, gen=torch.Generator().manual_seed(21), scale=0.2)
    # three live streams of six hops on slots 2, 0, 5; a 0-hop stream (slot 1), a skipped one (slot 3: input past the end), a stateless one (slot 9)
    rows = [(2, T, 0, 0), (0, T, T * H, T * H), (5, T, 2 * T * H, 2 * T * H), (1, 0, 3 * T * H, 3 * T * H), (3, T, n_in - H, 4 * T * H), (9, T, 5 * T * H, 5 * T * H)]
    d = _desc(rows)
    table = torch.zeros(cap)
    for (slot, *_), gain in zip(rows[:3], gains):
        table[slot] = gain
    table = table.to(_dev())

    def run(fn, gain):
        st, y, lv = full.clone(), _audio((n_in,), torch.int16, False, fill=777), torch.full((cap, 4), SENTINEL, device=_dev())
        fn(s, st, cap, d, y, T_max=T, min_gain=gain, levels=lv)
        k = eng.last_step_kernel()
        torch.cuda.synchronize()
        return st, y.cpu(), lv.cpu(), k

    st_lim, y_lim, lv_lim, k = run(eng.step_streams_chunk, table)
    assert "time-pipelined" in k
    st_off, y_off, lv_off, _ = run(eng.step_streams_chunk, None)
    st_ser, y_ser, lv_ser, k_ser = run(eng.step_streams, table)
    assert "time-pipelined" not in k_ser
    vl, vo = _views(eng, st_lim, cap), _views(eng, st_off, cap)
    for i, ((slot, *_), gain) in enumerate(zip(rows[:3], gains)):
        row = slice(i * T * H, (i + 1) * T * H)
        for j, (a, b) in enumerate(zip(vl, vo)):
            if j == 1:        # cache_istft: the output path
                assert _same(a[slot], b[slot]) == (gain == 0.0), f"gain {gain}: cache_istft"
            else:             # cache_stft and the model's own state: untouched by the limit
                assert _same(a[slot], b[slot]), f"gain {gain}: state tensor {j} differs from the unlimited chunk"
        assert torch.equal(y_lim[row], y_off[row]) == (gain == 0.0), f"gain {gain}: wav_out"
        _assert_rows_close(y_lim[row], y_ser[row], torch.int16, f"gain {gain} against the serial step")
        # the level row
        x = s[row].cpu().double() / 32768.0
        got, ser = lv_lim[slot], lv_ser[slot]
        assert _same(got[1], ser[1]) and float(got[1]) == float(x.abs().max()), "in_peak is exact"
        ss = float((x * x).sum())
        print(f"gain {gain}: in_sumsq {float(got[0]):.9e} against {ss:.9e} (fp64), relative {abs(float(got[0]) - ss) / ss:.3e}")
        assert abs(float(got[0]) - ss) <= 1e-5 * ss          # (n eps for n = 1536 samples, with margin)
        q = y_lim[row].double() / 32768.0                    # the output is metered before its quantisation: half an int16 step per sample
        assert abs(float(got[3]) - float(q.abs().max())) <= 0.5 / 32768 + 1e-7
        assert abs(math.sqrt(float(got[2]) / (T * H)) - math.sqrt(float((q * q).mean()))) <= 0.5 / 32768 + 1e-7
        scale = float(q.abs().max())
        assert abs(float(got[3]) - float(ser[3])) <= PIPE_REL * scale
        assert abs(math.sqrt(float(got[2]) / (T * H)) - math.sqrt(float(ser[2]) / (T * H))) <= PIPE_REL * scale
    for slot in (1, 3, 4, 6, 7):                              # 0 hops, skipped, not named: no row
        assert bool((lv_lim[slot] == SENTINEL).all()) and bool((lv_ser[slot] == SENTINEL).all()), f"slot {slot}: a level row was written"
    assert int((y_lim[5 * T * H:] != 0).sum()) == 0, "the stateless stream's rows are zero"


# ------------------------------------------------------------------ banks
def test_chunk_serves_each_stream_on_its_own_bank():
    from test_gpu_weight_banks import _banked, _refs
    name = "fe_t"
    eng, refs = _banked(name), _refs(name)
    H, cap, T = eng.cfg.hop_size, 5, 5
    rows = [(3, 5, 2), (0, 3, 0), (1, 4, 1), (4, 2, 9)]                # (slot, hops, bank); bank 9 is out of range
    table = torch.zeros(cap, dtype=torch.int32)
    for slot, _, bank in rows:
        table[slot] = bank
    table = table.to(_dev())
    full = _seeded_state(refs[0], cap, hops=4)
    x = _audio((len(rows) * T * H,), torch.float32, False, gen=torch.Generator().manual_seed(31))
    d = _desc([(slot, hops, i * T * H, i * T * H) for i, (slot, hops, _) in enumerate(rows)])
    st, y = full.clone(), _audio((len(rows) * T * H,), torch.float32, False, fill=7.0)
    eng.step_streams_chunk(x, st, cap, d, y, T_max=T, bank=table)
    k = eng.last_step_kernel()
    torch.cuda.synchronize()
    assert "time-pipelined" in k and "banks" in k, k
    st_ref, y_ref = full.clone(), _audio((len(rows) * T * H,), torch.float32, False, fill=7.0)
    for b, ref in enumerate(refs):                                     # every checkpoint's one-bank engine serves its own streams, serially
        d_b = _desc([(slot, hops if bank == b else 0, i * T * H, i * T * H) for i, (slot, hops, bank) in enumerate(rows)])
        ref.step_streams(x, st_ref, cap, d_b, y_ref, T_max=T)
        torch.cuda.synchronize()
    for i, (slot, hops, bank) in enumerate(rows[:3]):
        _assert_rows_close(y[i * T * H:i * T * H + hops * H], y_ref[i * T * H:i * T * H + hops * H], torch.float32, f"stream {i} on bank {bank}")
        assert bool((y[i * T * H + hops * H:(i + 1) * T * H] == 7.0).all())
    _assert_state_close(eng, cap, st, st_ref, [r[0] for r in rows[:3]], name)
    assert int((y[3 * T * H:3 * T * H + 2 * H] != 0).sum()) == 0, "a bank out of range gives zero rows"
    for j, (a, b) in enumerate(zip(_views(eng, st, cap), _views(eng, full, cap))):
        assert _same(a[torch.tensor([4, 2])], b[torch.tensor([4, 2])]), f"state tensor {j} of a stream without a bank, or of a slot not named, changed"


# ------------------------------------------------------------------ fallbacks: the serial step, bit for bit, under its own name
def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


@pytest.mark.parametrize("case", ["T_max=3", "pipeline off", "2n > CUs", "fe_tk_b", "fe_dpt_t"])
def test_what_is_not_pipelined_is_the_serial_step_bit_for_bit(case):
    name = case if case.startswith("fe_") else "fe_b"
    eng = _engine(name)
    H = eng.cfg.hop_size
    T = 3 if case == "T_max=3" else 5
    if case == "2n > CUs":
        n = _cus() // 2 + 1
        rows = [(n - 1 - i, 1, i * H, i * H) for i in range(n)]        # a capacity-sized batch, one hop each
    else:
        n = 4
        rows = [(2, T, 0, 0), (0, 1, T * H, T * H), (3, 2, 2 * T * H, 2 * T * H), (1, 0, 3 * T * H, 3 * T * H)]
    cap, count = n, n * T * H
    full = _seeded_state(eng, cap, hops=4)
    x = _audio((count,), torch.int16, False, gen=torch.Generator().manual_seed(41))
    lv = [torch.full((cap, 4), SENTINEL, device=_dev()) for _ in range(2)]
    out = []
    try:
        if case == "pipeline off":
            eng.set_time_pipeline(0)
        for i, fn in enumerate((eng.step_streams_chunk, eng.step_streams)):
            st, y = full.clone(), _audio((count,), torch.int16, False, fill=777)
            fn(x, st, cap, _desc(rows), y, T_max=T, levels=lv[i])
            out.append((st, y, eng.last_step_kernel()))
            torch.cuda.synchronize()
    finally:
        eng.set_time_pipeline(-1)
    assert out[0][2] == out[1][2] and "time-pipelined" not in out[0][2], out[0][2]
    assert torch.equal(out[0][1], out[1][1]) and _same(out[0][0], out[1][0]) and _same(lv[0], lv[1])
    assert not _same(out[0][0], full)
    if case in ("T_max=3", "fe_tk_b", "fe_dpt_t"):
        assert eng.streams_chunk_work_floats(n, T) == 0


# ------------------------------------------------------------------ a captured graph follows the descriptors
def test_a_captured_chunk_follows_rewritten_descriptors():
    eng = _engine("fe_b")
    dev, H, cap, n, T = _dev(), eng.cfg.hop_size, 6, 3, 8
    full = _seeded_state(eng, cap, hops=4)
    count = n * T * H
    x = _audio((count,), torch.float32, False, gen=torch.Generator().manual_seed(51))
    y, st = torch.zeros(count, device=dev), full.clone()
    work = torch.empty(eng.streams_chunk_work_floats(n, T), dtype=torch.float32, device=dev)
    descs = [[(4, 8, 0, 0), (1, 2, T * H, T * H), (0, 5, 2 * T * H, 2 * T * H)],
             [(2, 1, 0, 0), (4, 0, T * H, T * H), (5, 7, 2 * T * H, 2 * T * H)],
             [(0, 3, 5, 3), (9, 4, T * H, T * H), (1, 6, 2 * T * H, 2 * T * H)]]
    d = _desc(descs[0])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                             # warm-up: nothing allocates in the capture
            eng.step_streams_chunk(x, full.clone(), cap, d, y, T_max=T, work=work)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    # nothing is allocated: not from torch's allocator (counted around a warm call - the capture context itself takes two blocks of its
    # own), and not from the runtime's (an allocation inside a capture is an error, and the capture below succeeds)
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    eng.step_streams_chunk(x, st, cap, d, y, T_max=T, work=work)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before, "the call allocated"
    torch.cuda.synchronize()
    st.copy_(full)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eng.step_streams_chunk(x, st, cap, d, y, T_max=T, work=work)
    assert "time-pipelined" in eng.last_step_kernel()
    st_e, work_e = full.clone(), torch.empty_like(work)
    for r, rows in enumerate(descs):
        d.copy_(Engine.pack_stream_desc(rows))
        y.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        y_e = torch.full((count,), 7.0, device=dev)
        eng.step_streams_chunk(x, st_e, cap, _desc(rows), y_e, T_max=T, work=work_e)
        torch.cuda.synchronize()
        assert _same(y, y_e), f"replay {r}: rows differ from the eager call"
        assert _same(st, st_e), f"replay {r}: state differs from the eager call"
    assert not _same(st, full)


# ------------------------------------------------------------------ end to end: PacketPool(backlog_hops=)
def test_packet_pool_serves_a_backlog_in_a_second_launch():
    from test_gpu_weight_banks import _banked
    eng = _banked("fe_b")
    H = eng.cfg.hop_size
    g = torch.Generator().manual_seed(61)
    pcm = (0.2 * torch.randn(4, 15 * H, generator=g) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    packets = [700, 123, 1501, 64]                                     # uneven; the rest of the 13.5 hops in one piece

    def run(T_max, backlog_hops):
        pool = PacketPool(eng, 4, ring_hops=32, T_max=T_max, meters=True, backlog_hops=backlog_hops)
        late = pool.open(bank=1)
        pool.set_suppression_limit(late, -12.0)
        others = [pool.open() for _ in range(3)]
        sent = 0
        for p in packets + [13 * H + H // 2 - sum(packets)]:
            pool.push(late, pcm[0, sent:sent + p])
            sent += p
        for i, slot in enumerate(others):
            pool.push(slot, pcm[1 + i, :H])
        launched = pool.tick()
        k = eng.last_step_kernel()
        first = [pool.pull(s) for s in [late] + others]
        lv = [pool.levels(s) for s in [late] + others]
        pool.push(late, pcm[0, sent:sent + H // 2])                    # the leftover half hop completed: an ordinary tick
        for i, slot in enumerate(others):
            pool.push(slot, pcm[1 + i, H:2 * H])
        launched2 = pool.tick()
        second = [pool.pull(s) for s in [late] + others]
        return late, others, launched, k, first, lv, launched2, second

    late, others, launched, k, first, lv, launched2, second = run(1, 16)
    assert "time-pipelined" in k and "pinned, s16, banks" in k, k
    assert launched[:3] == [(s, 1, s * 32 * H, s * 32 * H) for s in others] and launched[3] == (late, 13, late * 32 * H, late * 32 * H), launched
    assert sorted(launched2) == sorted((s, 1, s * 32 * H + (13 if s == late else 1) * H, s * 32 * H + (13 if s == late else 1) * H) for s in [late] + others)
    _, _, t_launched, t_k, t_first, t_lv, _, t_second = run(16, 0)
    assert "time-pipelined" not in t_k and sorted(t_launched) == sorted(launched)
    assert first[0].numel() == 13 * H and second[0].numel() == H
    for i in range(4):
        _assert_rows_close(first[i], t_first[i], torch.int16, f"stream {i}, first tick")
        _assert_rows_close(second[i], t_second[i], torch.int16, f"stream {i}, next tick")
        a, b = lv[i], t_lv[i]
        assert a.samples == b.samples == (13 * H if i == 0 else H)
        assert a.in_peak == b.in_peak
        assert abs(a.in_sumsq - b.in_sumsq) <= 1e-5 * b.in_sumsq
        scale = float(t_first[i].abs().max()) / 32768.0
        assert abs(a.out_peak - b.out_peak) <= PIPE_REL * scale
        assert abs(math.sqrt(a.out_sumsq / a.samples) - math.sqrt(b.out_sumsq / b.samples)) <= PIPE_REL * scale
    assert not torch.equal(first[0], torch.zeros_like(first[0]))
