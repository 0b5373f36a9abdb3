"""The packet step's time-pipelined form for BSRNN and FSPEN pools on the GPU (fe_step_pool_streams_chunk[_pinned] through
Engine.step_pool_streams_chunk* and serving.BacklogPacketPool).

The call means fe_step_pool_streams_ctl[_pinned] with the same arguments: on the pipeline each stream's hops run on co-resident workgroups - the
PIPE + SLOT + STRM instantiation of the family's frame kernel, the state handed from frame to frame in place at the stream's slot - and
stream_ola_streams_kernel overlap-adds them, which agrees with the serial packet step to fp32 rounding (output rows and every model-state tensor
of the stepped slots), leaves cache_stft (a copy of input samples) bit-identical and touches nothing else: no slot it does not advance, no sample
outside the rows its descriptors name.  Where nothing is pipelined it is the serial step bit for bit.  Every pipelined case asserts the kernel
string: a silent fall-back to the serial step fails the test instead of passing it.

Models: the smallest that reach every state path - bsrnn_xxt (register-resident weights), bsrnn_t (streamed weights), bsrnn_s (C = 64: the
band-LSTM projections in global scratch) and fspen (the inter-GRU states).

Bounds.  PIPE_REL = 3e-5 of the reference's largest magnitude for pipelined against serial (tests/test_gpu_step_chunk.py); int16 rows
|q_chunk - q_serial| <= 1 + ceil(PIPE_REL * max|q|) LSB (tests/test_gpu_streams_chunk.py); TIGHT_REL[family] against the fp32 oracle
(tests/test_gpu_parity.py).  Level rows against the serial step's: in_peak equal; in_sumsq - the same samples summed in another order - within
PIPE_REL of itself; out_peak and the output's rms, which move by no more than the largest sample difference, within PIPE_REL of the largest
output magnitude.

The core case is that of tests/test_gpu_streams_chunk.py: capacity 7, T_max 9, (slot, hops) = (5, 9), (0, 1), (3, 0), (2, 4), (1, 2), (7, 3) -
slot 7 has no state - and (6, 2) whose input range ends past in_count, which is skipped; slot 4 is not named.  1, 2 and 3 hops are below what the
pipeline's width needs: workgroups beyond the stream's hops leave, and the last frame is hops - 1."""
import math

import numpy as np
import pytest
import torch

from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import BacklogPacketPool, FamilyPacketPool
from oracle.weightgen import make_input
from test_gpu_parity import TIGHT_REL, _assert_close
from test_gpu_step_backlog import SEED_HOPS, _fam
from test_gpu_step_chunk import _cached, _dev, _engine, _same, _seed_audio, _seeded_state
from test_gpu_stream_packets import _audio, _desc
from test_gpu_streams_chunk import CAP, LIVE, PIPE_REL, ROWS, SENTINEL, SKIPPED, STATELESS, TM, _assert_rows_close, _fill, _run_core

pytestmark = pytest.mark.gpu

MODELS = ["bsrnn_xxt", "bsrnn_t", "bsrnn_s", "fspen"]
AUDIO = {"device-f32": (False, torch.float32), "pinned-s16": (True, torch.int16), "device-s16": (False, torch.int16), "pinned-f32": (True, torch.float32)}
CORE_CASES = [(m, a) for m in MODELS for a in ("device-f32", "pinned-s16")] + [(m, a) for m in ("bsrnn_xxt", "fspen") for a in ("device-s16", "pinned-f32")]


def _chunk(eng, pinned):
    return eng.step_pool_streams_chunk_pinned if pinned else eng.step_pool_streams_chunk


def _serial(eng, pinned):
    return eng.step_pool_streams_ctl_pinned if pinned else eng.step_pool_streams_ctl


def _piped(k, name):
    kernel = "fspen_frame_kernel" if name == "fspen" else "bsrnn_frame_kernel"
    return f"{kernel}<time-pipelined, streams" in k and "time-pipelined" in k and "+ stream_ola_streams_kernel" in k


def _width(eng, width):
    """a context that runs under fe_set_time_pipeline(width) and restores the default (the engines are shared between test modules)"""
    class W:
        def __enter__(self):
            eng.set_time_pipeline(width)

        def __exit__(self, *exc):
            eng.set_time_pipeline(-1)
    return W()


def _slot_tensors(eng, state, cap, slots):
    """per named slot, the reference's cache list of its state record (a record is the stream's state as a capacity-1 state)"""
    recs = eng.export_slots(state, cap, list(slots))
    torch.cuda.synchronize()
    return [eng.split_state(recs[i], 1) for i in range(len(slots))]


def _assert_slots_close(eng, cap, got, ref, slots, what):
    """cache_stft of the stepped slots bit for bit, every other state tensor of them within PIPE_REL of the reference's largest magnitude"""
    a, b = _slot_tensors(eng, got, cap, slots), _slot_tensors(eng, ref, cap, slots)
    for j in range(len(a[0])):
        u, v = torch.stack([s[j].reshape(-1) for s in a]), torch.stack([s[j].reshape(-1) for s in b])
        if j == 0:
            assert _same(u, v), f"{what}: cache_stft differs"
            continue
        diff, scale = float((u - v).abs().max()), float(v.abs().max())
        print(f"{what}: state tensor {j}: max abs diff {diff:.3e}, scale {scale:.3e}")
        assert torch.isfinite(u).all() and diff <= PIPE_REL * scale, f"{what}: state tensor {j}: {diff:.3e} > {PIPE_REL:.0e} x {scale:.3e}"


def _tensors(eng, state, cap):
    """(cache_stft [cap, N - H], cache_istft [cap, N - H], the model's own state) of a state sized for cap streams"""
    n = cap * eng.cfg.cache_len
    return state[:n].view(cap, -1), state[n:2 * n].view(cap, -1), state[2 * n:]


def _check_core(name, pinned, dtype):
    eng = _engine(name)
    H = eng.cfg.hop_size
    full = _seeded_state(eng, CAP, SEED_HOPS)
    x, rows, offs, st, y, k = _run_core(eng, full, dtype, pinned, _chunk(eng, pinned))
    _, _, _, st_ref, y_ref, k_ref = _run_core(eng, full, dtype, pinned, _serial(eng, pinned))
    assert _piped(k, name), k
    assert ("pinned" in k) == pinned and ("s16" in k) == (dtype == torch.int16), k
    assert "time-pipelined" not in k_ref and "slots, streams" in k_ref, k_ref
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
            assert int((y_ref[lo:lo + n] != 0).sum()) > 0
    assert bool((y[~written] == _fill(dtype)).all()), "a sample outside the rows of the streams that advanced was written"
    assert bool((y_ref[~written] == _fill(dtype)).all())
    # state: stepped slots close (cache_stft bit for bit), everything else bit for bit
    live_slots = [ROWS[i][0] for i in LIVE]
    _assert_slots_close(eng, CAP, st, st_ref, live_slots, name)
    still = [3, 4, ROWS[SKIPPED][0]]
    assert _same(eng.export_slots(st, CAP, still), eng.export_slots(full, CAP, still)), "a slot the call does not advance changed"
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
        _assert_slots_close(eng, CAP, st, st_ref, live_slots, f"{name} after continuation hop {t}")


@pytest.mark.parametrize("name,audio", CORE_CASES)
def test_chunk_equals_the_serial_packet_step_and_leaves_a_valid_state(name, audio):
    _check_core(name, *AUDIO[audio])


@pytest.mark.parametrize("width", [2, 3, -1])
@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen"])
def test_chunk_at_other_pipeline_widths(name, width):
    """width 2: a workgroup runs several frames of the nine-hop stream; 3; the default"""
    with _width(_engine(name), width):
        _check_core(name, False, torch.float32)


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen"])
def test_packet_chunks_match_the_oracle_stepping_hop_by_hop(name):
    """from a state seeded by four hops: two consecutive pipelined packet chunks of 13 hops, then three one-hop ticks on the state they leave -
    the outputs of all three parts and the caches after each against the fp32 oracle, within the family's own bound"""
    m, orc, cfg, sr = _cached(name)
    eng = m.engine
    B, T, H, tight = 3, 13, cfg.hop_size, TIGHT_REL[_fam(name)]
    x0 = _seed_audio(eng, B, SEED_HOPS).numpy()
    x = make_input(B, (2 * T + 3) * H, 4243, sr)
    caches = orc.initialize_cache(B)
    for t in range(SEED_HOPS):
        _, *caches = orc.step(x0[:, t * H:(t + 1) * H], *caches)
    refs, ref_caches = [], []
    for t in range(2 * T + 3):
        o, *caches = orc.step(x[:, t * H:(t + 1) * H], *caches)
        refs.append(o)
        if t + 1 in (T, 2 * T, 2 * T + 3):
            ref_caches.append([np.array(c) for c in caches])
    ref = np.concatenate(refs, axis=1)

    state = _seeded_state(eng, B, SEED_HOPS)
    xd = torch.from_numpy(x).to(_dev())
    for i, (t0, t1) in enumerate([(0, T), (T, 2 * T), (2 * T, 2 * T + 3)]):
        if i < 2:
            xin = xd[:, t0 * H:t1 * H].contiguous().view(-1)
            y = torch.zeros(B * T * H, device=_dev())
            eng.step_pool_streams_chunk(xin, state, B, [(b, T, b * T * H, b * T * H) for b in range(B)], y, T_max=T)
            assert _piped(eng.last_step_kernel(), name), eng.last_step_kernel()
            torch.cuda.synchronize()
            y = y.view(B, T * H)
        else:
            ys = []
            for t in range(t0, t1):
                y1 = torch.zeros(B * H, device=_dev())
                eng.step_pool_streams_ctl(xd[:, t * H:(t + 1) * H].contiguous().view(-1), state, B, [(b, 1, b * H, b * H) for b in range(B)], y1, T_max=1)
                ys.append(y1.view(B, H))
            torch.cuda.synchronize()
            y = torch.cat(ys, dim=1)
        _assert_close(y.cpu().numpy(), ref[:, t0 * H:t1 * H], f"{name} part {i} wav_out", tight=tight)
        for j, (a, b) in enumerate(zip(eng.split_state(state, B), ref_caches[i])):
            _assert_close(a.cpu().numpy(), b, f"{name} cache {j} after part {i}", tight=tight)


# ------------------------------------------------------------------ controls: the suppression limit and the level meters
@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen"])
def test_chunk_applies_the_limit_to_the_output_path_only_and_meters_like_the_serial_step(name):
    eng = _engine(name)
    H, cap, T = eng.cfg.hop_size, 8, 6
    gains = [0.0, 0.25, 1.0]
    full = _seeded_state(eng, cap, SEED_HOPS)
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

    st_lim, y_lim, lv_lim, k = run(eng.step_pool_streams_chunk, table)
    assert _piped(k, name), k
    st_off, y_off, lv_off, k_off = run(eng.step_pool_streams_chunk, None)
    assert _piped(k_off, name), k_off
    st_ser, y_ser, lv_ser, k_ser = run(eng.step_pool_streams_ctl, table)
    assert "time-pipelined" not in k_ser
    st_two, y_two, lv_two, _ = run(eng.step_pool_streams_chunk, table)
    assert torch.equal(y_lim, y_two) and _same(st_lim, st_two) and _same(lv_lim, lv_two), "two identical runs differ"
    (cs_l, ci_l, m_l), (cs_o, ci_o, m_o) = _tensors(eng, st_lim, cap), _tensors(eng, st_off, cap)
    assert _same(m_l, m_o), "the limit changed the model's own state"
    assert _same(cs_l, cs_o), "the limit changed cache_stft"
    for i, ((slot, *_), gain) in enumerate(zip(rows[:3], gains)):
        row = slice(i * T * H, (i + 1) * T * H)
        assert _same(ci_l[slot], ci_o[slot]) == (gain == 0.0), f"gain {gain}: cache_istft"
        assert torch.equal(y_lim[row], y_off[row]) == (gain == 0.0), f"gain {gain}: wav_out"
        _assert_rows_close(y_lim[row], y_ser[row], torch.int16, f"{name} gain {gain} against the serial step")
        got, ser = lv_lim[slot], lv_ser[slot]
        x = s[row].cpu().double() / 32768.0
        assert _same(got[1], ser[1]) and float(got[1]) == float(x.abs().max()), "in_peak is exact"
        print(f"{name} gain {gain}: in_sumsq {float(got[0]):.9e} (serial {float(ser[0]):.9e}), out_sumsq {float(got[2]):.9e} ({float(ser[2]):.9e}), "
              f"out_peak {float(got[3]):.9e} ({float(ser[3]):.9e})")
        assert abs(float(got[0]) - float(ser[0])) <= PIPE_REL * float(ser[0])
        scale = float(y_ser[row].abs().max()) / 32768.0
        assert abs(float(got[3]) - float(ser[3])) <= PIPE_REL * scale
        assert abs(math.sqrt(float(got[2]) / (T * H)) - math.sqrt(float(ser[2]) / (T * H))) <= PIPE_REL * scale
    _assert_slots_close(eng, cap, st_lim, st_ser, [r[0] for r in rows[:3]], f"{name} limited, against the serial step")
    for slot in (1, 3, 4, 6, 7):                              # 0 hops, skipped, not named: no row
        assert bool((lv_lim[slot] == SENTINEL).all()) and bool((lv_ser[slot] == SENTINEL).all()), f"slot {slot}: a level row was written"
    assert int((y_lim[5 * T * H:] != 0).sum()) == 0, "the stateless stream's rows are zero"
    assert bool((y_lim[3 * T * H:5 * T * H] == 777).all()), "the rows of the 0-hop and the skipped stream were written"
    keep = [1, 3, 4, 6, 7]
    assert _same(eng.export_slots(st_lim, cap, keep), eng.export_slots(full, cap, keep))


# ------------------------------------------------------------------ fallbacks: the serial step, bit for bit, under its own name
@pytest.mark.parametrize("name,case", [(m, c) for m in ("bsrnn_xxt", "fspen") for c in ("T_max=3", "pipeline 0", "pipeline 1")] + [("lisennet", "T_max=9")])
def test_what_is_not_pipelined_is_the_serial_step_bit_for_bit(name, case):
    eng = _engine(name)
    H, cap = eng.cfg.hop_size, 4
    T = 3 if case == "T_max=3" else 9
    rows = [(2, T, 0, 0), (0, 1, T * H, T * H), (3, 2, 2 * T * H, 2 * T * H), (1, 0, 3 * T * H, 3 * T * H)]
    count = cap * T * H
    full = _seeded_state(eng, cap, SEED_HOPS)
    x = _audio((count,), torch.int16, False, gen=torch.Generator().manual_seed(41))
    lv = [torch.full((cap, 4), SENTINEL, device=_dev()) for _ in range(2)]
    out = []
    with _width(eng, int(case[-1]) if case.startswith("pipeline") else -1):
        for i, fn in enumerate((eng.step_pool_streams_chunk, eng.step_pool_streams_ctl)):
            st, y = full.clone(), _audio((count,), torch.int16, False, fill=777)
            kw = dict(work=None) if i == 0 else {}
            fn(x, st, cap, _desc(rows), y, T_max=T, levels=lv[i], **kw)
            out.append((st, y, eng.last_step_kernel()))
            torch.cuda.synchronize()
    assert out[0][2] == out[1][2] and "time-pipelined" not in out[0][2], out[0][2]
    assert torch.equal(out[0][1], out[1][1]) and _same(out[0][0], out[1][0]) and _same(lv[0], lv[1])
    assert not _same(out[0][0], full)
    if case.startswith("T_max") :
        assert eng.pool_streams_chunk_work_floats(cap, T) == 0


# ------------------------------------------------------------------ the work buffer
@pytest.mark.parametrize("name,width", [("bsrnn_xxt", -1), ("bsrnn_s", 2), ("fspen", 3)])
def test_pool_streams_chunk_work_floats_cover_the_call(name, width):
    """exactly pool_streams_chunk_work_floats(n, T_max) floats, NaN-filled, with a sentinel region behind them: the sentinels keep their bits
    and the results are those of a run with a roomy zero-filled buffer, bit for bit (the method of tests/test_gpu_work_bounds.py)"""
    eng = _engine(name)
    H, guard, mark = eng.cfg.hop_size, 4096, 7.5
    need = eng.pool_streams_chunk_work_floats(len(ROWS), TM)
    assert need >= len(ROWS) * TM * eng.cfg.n_fft
    full = _seeded_state(eng, CAP, SEED_HOPS)
    results = []
    with _width(eng, width):
        for tight in (True, False):
            if tight:
                buf = torch.full((need + guard,), float("nan"), device=_dev())
                buf[need:] = mark
            else:
                buf = torch.zeros(4 * need + guard, device=_dev())
            fn = lambda *a, **kw: eng.step_pool_streams_chunk(*a, work=buf[:need] if tight else buf, **kw)
            _, _, _, st, y, k = _run_core(eng, full, torch.float32, False, fn)
            assert _piped(k, name), k
            if tight:
                assert bool((buf[need:] == mark).all()), f"{name}: floats behind pool_streams_chunk_work_floats({len(ROWS)}, {TM}) were written"
            results.append((y.clone(), st))
    assert torch.isfinite(results[0][0]).all() and torch.isfinite(results[0][1]).all()
    assert _same(results[0][0], results[1][0]) and _same(results[0][1], results[1][1])


# ------------------------------------------------------------------ a captured graph follows the descriptors
def test_a_captured_chunk_follows_rewritten_descriptors():
    name = "bsrnn_xxt"
    eng = _engine(name)
    dev, H, cap, n, T = _dev(), eng.cfg.hop_size, 6, 3, 8
    full = _seeded_state(eng, cap, SEED_HOPS)
    count = n * T * H
    g = torch.Generator().manual_seed(51)
    audio = [_audio((count,), torch.float32, False, gen=g) for _ in range(3)]
    x = audio[0].clone()
    y, st = torch.zeros(count, device=dev), full.clone()
    work = torch.empty(eng.pool_streams_chunk_work_floats(n, T), dtype=torch.float32, device=dev)
    descs = [[(4, 8, 0, 0), (1, 2, T * H, T * H), (0, 5, 2 * T * H, 2 * T * H)],
             [(2, 1, 0, 0), (4, 0, T * H, T * H), (5, 7, 2 * T * H, 2 * T * H)],
             [(0, 3, 5, 3), (9, 4, T * H, T * H), (1, 6, 2 * T * H, 2 * T * H)]]
    d = _desc(descs[0])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                             # warm-up: nothing allocates in the capture
            eng.step_pool_streams_chunk(x, full.clone(), cap, d, y, T_max=T, work=work)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    eng.step_pool_streams_chunk(x, st, cap, d, y, T_max=T, work=work)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before, "the call allocated"
    torch.cuda.synchronize()
    st.copy_(full)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eng.step_pool_streams_chunk(x, st, cap, d, y, T_max=T, work=work)
    assert _piped(eng.last_step_kernel(), name)
    st_e, work_e = full.clone(), torch.empty_like(work)
    for r, rows in enumerate(descs):
        d.copy_(Engine.pack_stream_desc(rows))
        x.copy_(audio[r])
        y.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        y_e = torch.full((count,), 7.0, device=dev)
        eng.step_pool_streams_chunk(audio[r], st_e, cap, _desc(rows), y_e, T_max=T, work=work_e)
        torch.cuda.synchronize()
        for (slot, hops, i0, o0) in rows:
            if hops and slot < cap:
                _assert_rows_close(y[o0:o0 + hops * H], y_e[o0:o0 + hops * H], torch.float32, f"replay {r} slot {slot}")
        untouched = torch.ones(count, dtype=torch.bool, device=dev)
        for (slot, hops, i0, o0) in rows:
            untouched[o0:o0 + hops * H] = False
        assert bool((y[untouched] == 7.0).all()) and bool((y_e[untouched] == 7.0).all())
        _assert_slots_close(eng, cap, st, st_e, [s for s, h, _, _ in rows if h and s < cap], f"replay {r}")
    assert not _same(st, full)


# ------------------------------------------------------------------ end to end: BacklogPacketPool
def test_backlog_packet_pool_serves_an_fspen_backlog_in_a_second_launch():
    eng = _engine("fspen")
    H, K = eng.cfg.hop_size, 8
    g = torch.Generator().manual_seed(61)
    pcm = (0.2 * torch.randn(3, 11 * H, generator=g) * 32768).round().clamp(-32768, 32767).to(torch.int16)

    def run(cls, **kw):
        pool = cls(eng, 4, ring_hops=16, T_max=1, meters=True, **kw)
        late = pool.open()
        pool.set_suppression_limit(late, -12.0)
        others = [pool.open() for _ in range(2)]
        pool.push(late, pcm[0])                                          # eleven hops at once
        launched, kernels, pulled = [], [], [[], [], []]
        for t in range(11):
            for i, slot in enumerate(others):
                if t < 2:
                    pool.push(slot, pcm[1 + i, t * H:(t + 1) * H])          # ... next to two streams with a hop per tick
            got = pool.tick()
            if not got:
                break
            launched.append(got)
            kernels.append(eng.last_step_kernel())
            for i, slot in enumerate([late] + others):
                pulled[i].append(pool.pull(slot))
        counters = [(pool._pushed[s], pool._stepped[s], pool._pulled[s]) for s in [late] + others]
        return late, others, launched, kernels, [torch.cat(p) for p in pulled], counters, pool.levels(late)

    late, others, launched, kernels, pulled, counters, lv = run(BacklogPacketPool, backlog_hops=K)
    R = 16 * H
    assert launched[0] == [(s, 1, s * R, s * R) for s in others] + [(late, K, late * R, late * R)], launched[0]      # the backlog after the ordinary ones
    assert launched[1] == [(s, 1, s * R + H, s * R + H) for s in others] + [(late, 3, late * R + K * H, late * R + K * H)], launched[1]
    assert len(launched) == 2
    assert all("fspen_frame_kernel<time-pipelined, streams, pinned, s16>" in k and "stream_ola_streams_kernel" in k for k in kernels), kernels
    _, _, t_launched, t_kernels, t_pulled, t_counters, t_lv = run(FamilyPacketPool)
    assert len(t_launched) == 11 and not any("time-pipelined" in k for k in t_kernels)
    assert counters == t_counters == [(11 * H, 11 * H, 11 * H), (2 * H, 2 * H, 2 * H), (2 * H, 2 * H, 2 * H)]
    for i in range(3):
        assert pulled[i].numel() == t_pulled[i].numel() == (11 if i == 0 else 2) * H
        _assert_rows_close(pulled[i], t_pulled[i], torch.int16, f"stream {i}")
    assert int((pulled[0] != 0).sum()) > 0
    assert lv.samples == 3 * H and t_lv.samples == H                     # the last tick that advanced the stream: three hops here, one there
