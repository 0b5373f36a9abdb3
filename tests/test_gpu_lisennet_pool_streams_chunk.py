"""LiSenNet pools: a packet stream's backlog on the time pipeline (fe_step_pool_streams_chunk[_pinned] under an explicit
fe_set_time_pipeline(P >= 2) with a work buffer of fe_lisennet_pool_streams_chunk_work_floats, through Engine.step_pool_streams_chunk* and
serving.BacklogPacketPool).

The pipelined call is zero_counters_kernel, lisennet_frame_kernel<time-pipelined, streams[, pinned][, s16]> - the CARRY + PIPE + SLOT + STRM
instantiation: frame 0 of a stream takes the nine caches from the stream's slot, its last frames leave theirs there, in place - and
stream_ola_streams_kernel.  It means fe_step_pool_streams_ctl[_pinned] with the same arguments: output rows and every model-state tensor of
the stepped slots agree to fp32 rounding, cache_stft bit for bit, nothing else is touched; at every other setting it is that launch bit for
bit.  Every pipelined case asserts the kernel string: a silent fall-back to the serial step fails the test instead of passing it.

Bounds, the project's own: PIPE_REL = 3e-5 of the reference's largest magnitude for pipelined against serial (tests/test_gpu_step_chunk.py);
int16 rows |q_chunk - q_serial| <= 1 + ceil(PIPE_REL * max|q|) LSB (tests/test_gpu_streams_chunk.py); TIGHT_REL["lisennet"] against the fp32
oracle (tests/test_gpu_parity.py).  Every state is seeded non-zero by four hops.

Any hop count 0 .. T_max is served on the pipeline: a one-hop stream's frame is the reader of the old state and the last frame at every site
(and moves the ConvGLU's newer half to the older), a two-hop stream's frame 0 is also the ConvGLU's frame T - 2 - the in-place edge case runs
1, 2, 3, 4 and 5 hops in one call and compares the ConvGLU halves one by one."""
import math

import numpy as np
import pytest
import torch

from fastenhancer_amd import _lib
from fastenhancer_amd.engine import Engine, _ptr, _stream
from fastenhancer_amd.serving import BacklogPacketPool, FamilyPacketPool
from oracle.weightgen import make_input
from test_gpu_lisennet_backlog import N_CACHES, SEED_HOPS, _assert_seeded
from test_gpu_parity import TIGHT_REL, _assert_close
from test_gpu_pool_streams_chunk import AUDIO, _assert_slots_close, _chunk, _serial, _slot_tensors, _tensors, _width
from test_gpu_step_chunk import _cached, _dev, _same, _seed_audio, _seeded_state
from test_gpu_stream_packets import _audio, _desc
from test_gpu_streams_chunk import CAP, LIVE, PIPE_REL, ROWS, SENTINEL, SKIPPED, STATELESS, TM, _assert_rows_close, _fill, _run_core

pytestmark = pytest.mark.gpu

NAME = "lisennet"
GLU = (2 + 5, 2 + 7)            # the two ConvGLU caches in the reference's cache list [cache_stft, cache_istft, pha, e2, e3, e4, h, glu, h, glu, dec]


def _eng():
    return _cached(NAME)[0].engine


def _piped(k):
    return "lisennet_frame_kernel<time-pipelined, streams" in k and "+ stream_ola_streams_kernel" in k


def _serial_name(k):
    return "time-pipelined" not in k and "lisennet_frame_kernel<slots, streams" in k and "stream_ola" not in k


def _seeded(eng, cap):
    full = _seeded_state(eng, cap, SEED_HOPS)
    _assert_seeded(eng, cap, full)
    return full


def _continue(eng, cap, st, st_ref, slots, dtype, pinned, what):
    """two ordinary one-hop ticks on both states: a ConvGLU half or a cache left in the wrong place shows here"""
    H = eng.cfg.hop_size
    g = torch.Generator().manual_seed(12)
    d1 = _desc([(s, 1, i * H, i * H) for i, s in enumerate(slots)])
    for t in range(2):
        x1 = _audio((len(slots) * H,), dtype, pinned, gen=g)
        outs = []
        for state in (st, st_ref):
            y1 = _audio((len(slots) * H,), dtype, pinned, fill=_fill(dtype))
            _serial(eng, pinned)(x1, state, cap, d1, y1, T_max=1)
            assert _serial_name(eng.last_step_kernel())
            torch.cuda.synchronize()
            outs.append(y1.cpu())
        _assert_rows_close(outs[0], outs[1], dtype, f"{what} continuation hop {t}")
        _assert_slots_close(eng, cap, st, st_ref, slots, f"{what} after continuation hop {t}")


# ------------------------------------------------------------------ 1. the core case
@pytest.mark.parametrize("audio", list(AUDIO))
@pytest.mark.parametrize("width", [2, 3, 8])
def test_chunk_equals_the_serial_packet_step_and_leaves_a_valid_state(width, audio):
    pinned, dtype = AUDIO[audio]
    eng = _eng()
    H = eng.cfg.hop_size
    full = _seeded(eng, CAP)
    what = f"lisennet width {width} {audio}"
    with _width(eng, width):
        x, rows, offs, st, y, k = _run_core(eng, full, dtype, pinned, _chunk(eng, pinned))
        _, _, _, st2, y2, k2 = _run_core(eng, full, dtype, pinned, _chunk(eng, pinned))
        _, _, _, st_ref, y_ref, k_ref = _run_core(eng, full, dtype, pinned, _serial(eng, pinned))
    assert _piped(k) and _piped(k2), k
    assert ("pinned" in k) == pinned and ("s16" in k) == (dtype == torch.int16), k
    assert _serial_name(k_ref), k_ref
    assert torch.equal(y.cpu(), y2.cpu()) and _same(st, st2), "two identical runs differ"
    y, y_ref = y.cpu(), y_ref.cpu()
    written = torch.zeros(y.numel(), dtype=torch.bool)
    for i in LIVE + [STATELESS]:
        lo, n = offs[i], ROWS[i][1] * H
        written[lo:lo + n] = True
        if i == STATELESS:
            assert int((y[lo:lo + n] != 0).sum()) == 0 and int((y_ref[lo:lo + n] != 0).sum()) == 0, "a stream without state gets zero rows"
        else:
            _assert_rows_close(y[lo:lo + n], y_ref[lo:lo + n], dtype, f"{what} stream {i} ({ROWS[i][1]} hops)")
            assert int((y_ref[lo:lo + n] != 0).sum()) > 0
    assert bool((y[~written] == _fill(dtype)).all()), "a sample outside the rows of the streams that advanced was written"
    assert bool((y_ref[~written] == _fill(dtype)).all())
    live_slots = [ROWS[i][0] for i in LIVE]
    _assert_slots_close(eng, CAP, st, st_ref, live_slots, what)
    still = [3, 4, ROWS[SKIPPED][0]]
    assert _same(eng.export_slots(st, CAP, still), eng.export_slots(full, CAP, still)), "a slot the call does not advance changed"
    assert not _same(st, full)
    _continue(eng, CAP, st, st_ref, live_slots, dtype, pinned, what)


# ------------------------------------------------------------------ 2. the in-place edge: 1, 2 and 3 hops next to 4 and 5
@pytest.mark.parametrize("width", [2, 3])
def test_one_two_and_three_hop_streams_update_every_cache_in_place(width):
    eng = _eng()
    H, cap, T = eng.cfg.hop_size, 6, 5
    hops = [5, 1, 2, 3, 4]
    slots = [4, 0, 3, 5, 1]                                  # slot 2 is not named
    rows = [(s, h, i * T * H, i * T * H) for i, (s, h) in enumerate(zip(slots, hops))]
    count = len(rows) * T * H
    full = _seeded(eng, cap)
    x = _audio((count,), torch.float32, False, gen=torch.Generator().manual_seed(31))
    out = []
    with _width(eng, width):
        for fn in (eng.step_pool_streams_chunk, eng.step_pool_streams_ctl):
            st, y = full.clone(), _audio((count,), torch.float32, False, fill=7.0)
            fn(x, st, cap, _desc(rows), y, T_max=T)
            out.append((st, y.cpu(), eng.last_step_kernel()))
            torch.cuda.synchronize()
    (st, y, k), (st_ref, y_ref, k_ref) = out
    assert _piped(k) and _serial_name(k_ref), (k, k_ref)
    for (slot, h, i0, o0) in rows:
        _assert_rows_close(y[o0:o0 + h * H], y_ref[o0:o0 + h * H], torch.float32, f"width {width}: {h}-hop stream")
        assert bool((y[o0 + h * H:o0 + T * H] == 7.0).all())
    _assert_slots_close(eng, cap, st, st_ref, slots, f"width {width}")
    # each slot's ConvGLU caches, half by half, against the serial step's (and the halves moved: the seeded ones are gone)
    got, ref, old = (_slot_tensors(eng, s, cap, slots) for s in (st, st_ref, full))
    for i, h in enumerate(hops):
        for j in GLU:
            a, b, o = (t[i][j].reshape(32, 2, 32) for t in (got, ref, old))
            for half in (0, 1):
                diff, scale = float((a[:, half] - b[:, half]).abs().max()), float(b[:, half].abs().max())
                print(f"width {width}: {h}-hop stream, cache {j}, half {half}: max abs diff {diff:.3e}, scale {scale:.3e}")
                assert scale > 0 and diff <= PIPE_REL * scale, f"{h}-hop stream: ConvGLU cache {j} half {half}: {diff:.3e} > {PIPE_REL:.0e} x {scale:.3e}"
            if h == 1:
                assert _same(a[:, 0], o[:, 1]), "a one-hop stream: the older half is the newer half the call found"
            assert not _same(a[:, 0], o[:, 0]) and not _same(a[:, 1], o[:, 1])
    assert _same(eng.export_slots(st, cap, [2]), eng.export_slots(full, cap, [2])), "a slot the call does not advance changed"
    _continue(eng, cap, st, st_ref, slots, torch.float32, False, f"width {width}")


# ------------------------------------------------------------------ 3. against the oracle
def test_packet_chunks_match_the_oracle_stepping_hop_by_hop():
    """from a state seeded by four hops: two consecutive pipelined packet chunks of 13 hops, then three serial one-hop ticks on the state
    they leave - the outputs of all three parts and all eleven caches after each against the fp32 oracle, within the family's own bound"""
    m, orc, cfg, sr = _cached(NAME)
    eng = m.engine
    B, T, H, tight = 3, 13, cfg.hop_size, TIGHT_REL["lisennet"]
    x0 = _seed_audio(eng, B, SEED_HOPS).numpy()
    x = make_input(B, (2 * T + 3) * H, 4243, sr)
    caches = orc.initialize_cache(B)
    for t in range(SEED_HOPS):
        _, *caches = orc.step(x0[:, t * H:(t + 1) * H], *caches)
    assert len(caches) == 2 + N_CACHES
    refs, ref_caches = [], []
    for t in range(2 * T + 3):
        o, *caches = orc.step(x[:, t * H:(t + 1) * H], *caches)
        refs.append(o)
        if t + 1 in (T, 2 * T, 2 * T + 3):
            ref_caches.append([np.array(c) for c in caches])
    ref = np.concatenate(refs, axis=1)

    state = _seeded(eng, B)
    xd = torch.from_numpy(x).to(_dev())
    for i, (t0, t1) in enumerate([(0, T), (T, 2 * T), (2 * T, 2 * T + 3)]):
        if i < 2:
            xin = xd[:, t0 * H:t1 * H].contiguous().view(-1)
            y = torch.zeros(B * T * H, device=_dev())
            with _width(eng, 8):
                eng.step_pool_streams_chunk(xin, state, B, [(b, T, b * T * H, b * T * H) for b in range(B)], y, T_max=T)
            assert _piped(eng.last_step_kernel()), eng.last_step_kernel()
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
        _assert_close(y.cpu().numpy(), ref[:, t0 * H:t1 * H], f"lisennet part {i} wav_out", tight=tight)
        parts = eng.split_state(state, B)
        assert len(parts) == 2 + N_CACHES
        for j, (a, b) in enumerate(zip(parts, ref_caches[i])):
            _assert_close(a.cpu().numpy(), b, f"lisennet cache {j} after part {i}", tight=tight)


# ------------------------------------------------------------------ 4. controls: the suppression limit and the level meters
def test_chunk_applies_the_limit_to_the_output_path_only_and_meters_like_the_serial_step():
    eng = _eng()
    H, cap, T = eng.cfg.hop_size, 8, 6
    gains = [0.0, 0.25, 1.0]
    full = _seeded(eng, cap)
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

    with _width(eng, 8):
        st_lim, y_lim, lv_lim, k = run(eng.step_pool_streams_chunk, table)
        st_off, y_off, lv_off, k_off = run(eng.step_pool_streams_chunk, None)
        st_ser, y_ser, lv_ser, k_ser = run(eng.step_pool_streams_ctl, table)
        st_two, y_two, lv_two, _ = run(eng.step_pool_streams_chunk, table)
    assert _piped(k) and _piped(k_off), (k, k_off)
    assert _serial_name(k_ser), k_ser
    assert torch.equal(y_lim, y_two) and _same(st_lim, st_two) and _same(lv_lim, lv_two), "two identical runs differ"
    (cs_l, ci_l, m_l), (cs_o, ci_o, m_o) = _tensors(eng, st_lim, cap), _tensors(eng, st_off, cap)
    assert _same(m_l, m_o), "the limit changed the model's own state"
    assert _same(cs_l, cs_o), "the limit changed cache_stft"
    for i, ((slot, *_), gain) in enumerate(zip(rows[:3], gains)):
        row = slice(i * T * H, (i + 1) * T * H)
        assert _same(ci_l[slot], ci_o[slot]) == (gain == 0.0), f"gain {gain}: cache_istft"
        assert torch.equal(y_lim[row], y_off[row]) == (gain == 0.0), f"gain {gain}: wav_out"
        _assert_rows_close(y_lim[row], y_ser[row], torch.int16, f"lisennet gain {gain} against the serial step")
        got, ser = lv_lim[slot], lv_ser[slot]
        x = s[row].cpu().double() / 32768.0
        assert _same(got[1], ser[1]) and float(got[1]) == float(x.abs().max()), "in_peak is exact"
        print(f"lisennet gain {gain}: in_sumsq {float(got[0]):.9e} (serial {float(ser[0]):.9e}), out_sumsq {float(got[2]):.9e} ({float(ser[2]):.9e}), "
              f"out_peak {float(got[3]):.9e} ({float(ser[3]):.9e})")
        assert abs(float(got[0]) - float(ser[0])) <= PIPE_REL * float(ser[0])
        scale = float(y_ser[row].abs().max()) / 32768.0
        assert abs(float(got[3]) - float(ser[3])) <= PIPE_REL * scale
        assert abs(math.sqrt(float(got[2]) / (T * H)) - math.sqrt(float(ser[2]) / (T * H))) <= PIPE_REL * scale
    _assert_slots_close(eng, cap, st_lim, st_ser, [r[0] for r in rows[:3]], "lisennet limited, against the serial step")
    for slot in (1, 3, 4, 6, 7):                              # 0 hops, skipped, not named: no row
        assert bool((lv_lim[slot] == SENTINEL).all()) and bool((lv_ser[slot] == SENTINEL).all()), f"slot {slot}: a level row was written"
    assert int((y_lim[5 * T * H:] != 0).sum()) == 0, "the stateless stream's rows are zero"
    assert bool((y_lim[3 * T * H:5 * T * H] == 777).all()), "the rows of the 0-hop and the skipped stream were written"
    keep = [1, 3, 4, 6, 7]
    assert _same(eng.export_slots(st_lim, cap, keep), eng.export_slots(full, cap, keep))


# ------------------------------------------------------------------ 5. fall-backs: the serial step, bit for bit, under its own name
@pytest.mark.parametrize("case", ["default width, work", "width 8, NULL work", "width 0, work", "width 1, work", "width 8, T_max=3"])
def test_what_is_not_pipelined_is_the_serial_step_bit_for_bit(case):
    eng = _eng()
    H, cap = eng.cfg.hop_size, 4
    T = 3 if "T_max=3" in case else 9
    width = -1 if case.startswith("default") else int(case.split(",")[0].split()[1])
    rows = [(2, T, 0, 0), (0, 1, T * H, T * H), (3, 2, 2 * T * H, 2 * T * H), (1, 0, 3 * T * H, 3 * T * H)]
    count = cap * T * H
    full = _seeded(eng, cap)
    x = _audio((count,), torch.int16, False, gen=torch.Generator().manual_seed(41))
    lv = [torch.full((cap, 4), SENTINEL, device=_dev()) for _ in range(2)]
    work = torch.zeros(eng.lisennet_pool_streams_chunk_work_floats(cap, 9), device=_dev())
    d = _desc(rows)
    out = []
    with _width(eng, width):
        for i in range(2):
            st, y = full.clone(), _audio((count,), torch.int16, False, fill=777)
            if i == 1:
                eng.step_pool_streams_ctl(x, st, cap, d, y, T_max=T, levels=lv[i])
            elif "NULL" in case:        # (Engine.step_pool_streams_chunk(work=None) hands its scratch at this width: the C call, with a null work buffer)
                with torch.cuda.device(eng.device):
                    _lib.check(eng.lib.fe_step_pool_streams_chunk(eng._h, _ptr(x), x.numel(), _ptr(st), cap, _ptr(d), _ptr(y), y.numel(), len(rows), T,
                                                                  _lib.FE_AUDIO_S16, _ptr(None), _ptr(lv[i]), _ptr(None), _stream(eng.device)), "fe_step_pool_streams_chunk")
            else:
                eng.step_pool_streams_chunk(x, st, cap, d, y, T_max=T, levels=lv[i], work=work)
            out.append((st, y, eng.last_step_kernel()))
            torch.cuda.synchronize()
    assert out[0][2] == out[1][2] and _serial_name(out[0][2]), out[0][2]
    assert torch.equal(out[0][1], out[1][1]) and _same(out[0][0], out[1][0]) and _same(lv[0], lv[1])
    assert not _same(out[0][0], full)
    assert eng.pool_streams_chunk_work_floats(cap, T) == 0


# ------------------------------------------------------------------ 6. the work buffer
def test_lisennet_pool_streams_chunk_work_floats_cover_the_call():
    """exactly the queried floats, NaN-filled, with a sentinel region behind them: the sentinels keep their bits and the results are those of a
    run with a roomy zero-filled buffer, bit for bit (the method of tests/test_gpu_work_bounds.py) - and once more with every CU's LDS poisoned"""
    eng = _eng()
    guard, mark = 4096, 7.5
    need = eng.lisennet_pool_streams_chunk_work_floats(len(ROWS), TM)
    assert need > len(ROWS) * TM * eng.cfg.n_fft
    full = _seeded(eng, CAP)
    results = []
    with _width(eng, 8):
        for mode in ("tight", "roomy", "poisoned"):
            if mode == "roomy":
                buf = torch.zeros(2 * need + guard, device=_dev())
            else:
                buf = torch.full((need + guard,), float("nan"), device=_dev())
                buf[need:] = mark
            if mode == "poisoned":
                eng.poison_lds()
            fn = lambda *a, **kw: eng.step_pool_streams_chunk(*a, work=buf if mode == "roomy" else buf[:need], **kw)
            _, _, _, st, y, k = _run_core(eng, full, torch.float32, False, fn)
            assert _piped(k), k
            if mode != "roomy":
                assert bool((buf[need:] == mark).all()), f"floats behind lisennet_pool_streams_chunk_work_floats({len(ROWS)}, {TM}) were written"
            results.append((y.clone(), st))
    assert torch.isfinite(results[0][0]).all() and torch.isfinite(results[0][1]).all()
    for y, st in results[1:]:
        assert _same(results[0][0], y) and _same(results[0][1], st)


# ------------------------------------------------------------------ 7. a captured graph follows the descriptors
def test_a_captured_chunk_follows_rewritten_descriptors():
    eng = _eng()
    dev, H, cap, n, T = _dev(), eng.cfg.hop_size, 6, 3, 8
    full = _seeded(eng, cap)
    count = n * T * H
    g = torch.Generator().manual_seed(51)
    audio = [_audio((count,), torch.float32, False, gen=g) for _ in range(3)]
    x = audio[0].clone()
    y, st = torch.zeros(count, device=dev), full.clone()
    work = torch.empty(eng.lisennet_pool_streams_chunk_work_floats(n, T), dtype=torch.float32, device=dev)
    descs = [[(4, 8, 0, 0), (1, 2, T * H, T * H), (0, 5, 2 * T * H, 2 * T * H)],
             [(2, 1, 0, 0), (4, 0, T * H, T * H), (5, 7, 2 * T * H, 2 * T * H)],
             [(0, 3, 5, 3), (9, 4, T * H, T * H), (1, 6, 2 * T * H, 2 * T * H)]]
    d = _desc(descs[0])
    with _width(eng, 8):
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
        assert _piped(eng.last_step_kernel()), eng.last_step_kernel()
        st_e, work_e = full.clone(), torch.empty_like(work)
        for r, rows in enumerate(descs):
            d.copy_(Engine.pack_stream_desc(rows))
            x.copy_(audio[r])
            y.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            y_e = torch.full((count,), 7.0, device=dev)
            eng.step_pool_streams_chunk(audio[r], st_e, cap, _desc(rows), y_e, T_max=T, work=work_e)
            assert _piped(eng.last_step_kernel())
            torch.cuda.synchronize()
            for (slot, hops, i0, o0) in rows:
                if hops and slot < cap:
                    _assert_rows_close(y[o0:o0 + hops * H], y_e[o0:o0 + hops * H], torch.float32, f"replay {r} slot {slot}")
                elif hops:
                    assert int((y[o0:o0 + hops * H] != 0).sum()) == 0, "a stream without state gets zero rows"
            untouched = torch.ones(count, dtype=torch.bool, device=dev)
            for (slot, hops, i0, o0) in rows:
                untouched[o0:o0 + hops * H] = False
            assert bool((y[untouched] == 7.0).all()) and bool((y_e[untouched] == 7.0).all())
            _assert_slots_close(eng, cap, st, st_e, [s for s, h, _, _ in rows if h and s < cap], f"replay {r}")
    assert not _same(st, full)


# ------------------------------------------------------------------ 8. end to end: BacklogPacketPool (and the resampled pool over it)
def _pool_run(eng, cls, pcm, **kw):
    H = eng.cfg.hop_size
    pool = cls(eng, 4, ring_hops=16, T_max=1, meters=True, **kw)
    late = pool.open()
    pool.set_suppression_limit(late, -12.0)
    others = [pool.open() for _ in range(2)]
    pool.push(late, pcm[0])                                              # eleven hops at once
    launched, kernels, pulled = [], [], [[], [], []]
    for t in range(11):
        for i, slot in enumerate(others):
            if t < 2:
                pool.push(slot, pcm[1 + i, t * H:(t + 1) * H])              # ... next to two streams with a hop per tick
        got = pool.tick()
        if not got:
            break
        launched.append(got)
        kernels.append(eng.last_step_kernel())
        for i, slot in enumerate([late] + others):
            pulled[i].append(pool.pull(slot))
    counters = [(pool._pushed[s], pool._stepped[s], pool._pulled[s]) for s in [late] + others]
    return late, others, launched, kernels, [torch.cat(p) for p in pulled], counters, pool.levels(late)


def test_backlog_packet_pool_serves_a_lisennet_backlog_on_the_time_pipeline_when_asked():
    eng = _eng()
    H, K = eng.cfg.hop_size, 8
    g = torch.Generator().manual_seed(61)
    pcm = (0.2 * torch.randn(3, 11 * H, generator=g) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    R = 16 * H
    try:
        eng.set_time_pipeline(8)
        late, others, launched, kernels, pulled, counters, lv = _pool_run(eng, BacklogPacketPool, pcm, backlog_hops=K)
    finally:
        eng.set_time_pipeline(-1)
    assert launched[0] == [(s, 1, s * R, s * R) for s in others] + [(late, K, late * R, late * R)], launched[0]      # the backlog after the ordinary ones
    assert launched[1] == [(s, 1, s * R + H, s * R + H) for s in others] + [(late, 3, late * R + K * H, late * R + K * H)], launched[1]
    assert len(launched) == 2
    # (the last launch of a tick is the backlog's: K = 8 hops, then three hops at T_max = 8)
    assert all("lisennet_frame_kernel<time-pipelined, streams, pinned, s16>" in k and "stream_ola_streams_kernel" in k for k in kernels), kernels
    _, _, t_launched, t_kernels, t_pulled, t_counters, t_lv = _pool_run(eng, FamilyPacketPool, pcm)
    assert len(t_launched) == 11 and not any("time-pipelined" in k for k in t_kernels)
    assert counters == t_counters == [(11 * H, 11 * H, 11 * H), (2 * H, 2 * H, 2 * H), (2 * H, 2 * H, 2 * H)]
    for i in range(3):
        assert pulled[i].numel() == t_pulled[i].numel() == (11 if i == 0 else 2) * H
        _assert_rows_close(pulled[i], t_pulled[i], torch.int16, f"stream {i}")
    assert int((pulled[0] != 0).sum()) > 0
    assert lv.samples == 3 * H and t_lv.samples == H
    # at the default width the pool launches what it launches today: the serial packet step, the same bits as without the new scratch rule
    _, _, d_launched, d_kernels, d_pulled, d_counters, _ = _pool_run(eng, BacklogPacketPool, pcm, backlog_hops=K)
    assert d_launched == launched and d_counters == counters
    assert all(_serial_name(k) for k in d_kernels), d_kernels
    for i in range(3):
        _assert_rows_close(d_pulled[i], t_pulled[i], torch.int16, f"default width, stream {i}")


def test_the_resampled_pools_over_a_backlog_pool_need_no_change(monkeypatch):
    """tests/test_gpu_ring_resample.py's backlog case on LiSenNet under an explicit width: six ordinary ticks, a stall of 8 ticks without a
    packet, then two double packets at once - 5 hops, more than T_max = 2: they leave in the backlog launch, which is the pipelined one in
    ResampledPacketPool and in RingResampledPacketPool alike - and the two pools return the same bits"""
    from fastenhancer_amd.serving import RingResampledPacketPool
    from test_gpu_ring_resample import _drive, _oracle_pool, _signal
    eng = _eng()
    seen = []
    call = eng.step_pool_streams_chunk_pinned

    def recorded(*a, **kw):
        out = call(*a, **kw)
        seen.append(eng.last_step_kernel())
        return out
    monkeypatch.setattr(eng, "step_pool_streams_chunk_pinned", recorded)
    packet = 960
    kw = dict(capacity=2, ring_hops=16, client_rate=48000, T_max=2, max_packet=4 * packet)
    try:
        eng.set_time_pipeline(8)
        old = _oracle_pool(BacklogPacketPool, step_hops=8, backlog_hops=8)(eng, **kw)
        new = RingResampledPacketPool(eng, pool=BacklogPacketPool, backlog_hops=8, **kw)
        assert type(new.inner) is type(old.inner) is BacklogPacketPool
        for s in range(2):
            assert (old.open(), new.open()) == (s, s)
        schedule = [([], [(0, 1), (1, 1)]) for _ in range(6)] + [([], [(1, 1)]) for _ in range(8)] + [([], [(0, 4), (1, 1)])] + [([], [(0, 1), (1, 1)]) for _ in range(6)]
        sig = _signal(2, 24 * packet, seed=43, dtype=torch.int16, peak=0.3)
        returns = _drive(old, new, schedule, packet, sig, check_levels=False)
    finally:
        eng.set_time_pipeline(-1)
    burst = [d for d in returns[14] if d[0] == 0]
    assert len(burst) == 1 and 2 < burst[0][1] <= 8, returns[14]          # slot 0's backlog: one launch of more than T_max hops
    assert len(seen) == 2 and all("lisennet_frame_kernel<time-pipelined, streams, pinned, s16>" in k for k in seen), seen      # one per pool
