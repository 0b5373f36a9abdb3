"""The packet step's per-stream controls on the GPU (fe_step_streams_ctl / fe_step_streams_ctl_pinned through Engine.step_streams*(min_gain=,
levels=) and PacketPool): a limit on how far a stream may be attenuated, and input / output level meters.

Off must be off - null tables, zeros and NaN give the bits of fe_step_streams; the limit must be the floor formula of the header applied to
the oracle's mask, and touch nothing but the output path; the level rows must be exact peaks and fp32 sums, bitwise reproducible, and written
for the streams that advanced only."""
import functools
import math

import numpy as np
import pytest
import torch

from common import build_oracle, rms
from fastenhancer_amd.serving import PacketPool
from test_gpu_stream_packets import _audio, _desc, _kernel, _step
from test_gpu_stream_slots import _dev, _engine, _same, _seeded_state, _views

pytestmark = pytest.mark.gpu

FAMILY_REL = 2e-5          # tests/test_gpu_parity.py TIGHT_REL["fastenhancer"]: ~5x the largest error of tests/golden/parity_observed_r5.json
NORTH_STAR = 1e-4
SENTINEL = -77.0


def _table(values, pinned=False):
    t = torch.tensor(values, dtype=torch.float32)
    return t.pin_memory() if pinned else t.to(_dev())


def _levels(cap, pinned=False):
    t = torch.full((cap, 4), SENTINEL)
    return t.pin_memory() if pinned else t.to(_dev())


# ------------------------------------------------------------------ 1. off is off
OFF_CASES = [("fe_b", "wg8", 1, 5), ("fe_b", "waves4", 3, 7), ("fe_t", "wg8", 1, 5), ("fe_tk_b", "wg8", 1, 5), ("fe_dpt_b", "wg8", 1, 5)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("name,kernel,TM,n", OFF_CASES)
def test_null_zero_and_nan_gain_tables_give_the_bits_of_the_plain_step(name, kernel, TM, n, pinned, dtype):
    eng = _engine(name)
    H, cap = eng.cfg.hop_size, n + 4
    slots = [int(s) for s in np.random.default_rng(n + TM).permutation(cap)[:n]]
    hops = [TM] * n if TM == 1 else [(i % TM) + 1 for i in range(n)]                  # ragged where the kernel allows it
    with _kernel(eng, kernel):
        full = _seeded_state(eng, cap)
        x = _audio((n, TM * H), dtype, pinned, gen=torch.Generator().manual_seed(21))
        d = _desc([(slots[i], hops[i], i * TM * H, i * TM * H) for i in range(n)])
        fill = 7.0 if dtype == torch.float32 else 777
        st0, y0 = full.clone(), _audio((n, TM * H), dtype, pinned, fill=fill)
        _step(eng, pinned)(x.view(-1), st0, cap, d, y0.view(-1), T_max=TM)
        k0 = eng.last_step_kernel()
        torch.cuda.synchronize()
        for what, gain in (("null", None), ("zeros", _table([0.0] * cap)), ("nan", _table([float("nan")] * cap))):
            st, y, lv = full.clone(), _audio((n, TM * H), dtype, pinned, fill=fill), _levels(cap)
            _step(eng, pinned)(x.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=gain, levels=lv)
            assert eng.last_step_kernel() == k0, "the ctl entry points pick the kernels of fe_step_streams, under their names"
            torch.cuda.synchronize()
            assert torch.equal(y.view(torch.int16), y0.view(torch.int16)), f"{what}: output differs from fe_step_streams"
            for j, (a, b) in enumerate(zip(_views(eng, st, cap), _views(eng, st0, cap))):
                assert _same(a, b), f"{what}: state tensor {j} differs from fe_step_streams"
            assert bool((lv[torch.tensor(slots)] != SENTINEL).all()), f"{what}: the level rows were not written"
    assert not _same(st0, full)


# ------------------------------------------------------------------ 2. the limit against the reference
GAINS = [0.0, 0.01, 0.1]
HOPS = 6


def _oracle_step_with_floor(orc, x, caches, gains):
    """FEOracle.step with the floor of the header between model_forward and the complex multiply, in fp64; gains [B].  Returns the step's
    outputs and, per stream, the fraction of bins the floor lifted."""
    c, dt = orc.cfg, orc.dtype
    spec_in, cache_stft = orc.stft_step(x, caches[0])
    s = spec_in[:, :-1].astype(dt)
    mag = np.maximum(np.sqrt(s[..., 0:1] ** 2 + s[..., 1:2] ** 2), dt(1e-5))
    s = s * mag ** dt(c.input_compression - 1.0)
    mask, h_out = orc.model_forward(s, list(caches[2:]))
    m = mask.astype(np.float64)                                                      # [B, F0, 1, 2]
    m_min = (np.asarray(gains, np.float64) ** float(c.input_compression)).reshape(-1, 1, 1)
    mabs = np.sqrt(m[..., 0] ** 2 + m[..., 1] ** 2)
    lift = np.maximum(1.0, m_min / np.where(mabs > 0, mabs, 1.0))
    floored = np.stack([np.where(mabs > 0, m[..., 0] * lift, m_min), np.where(mabs > 0, m[..., 1] * lift, 0.0)], axis=-1).astype(dt)
    frac = (mabs < m_min).mean(axis=(1, 2))
    y = np.stack([s[..., 0] * floored[..., 0] - s[..., 1] * floored[..., 1], s[..., 0] * floored[..., 1] + s[..., 1] * floored[..., 0]], axis=3)
    mag2 = np.sqrt(y[..., 0:1] ** 2 + y[..., 1:2] ** 2)
    y = y * mag2 ** dt(1.0 / c.input_compression - 1.0)
    y = np.pad(y, ((0, 0), (0, 1), (0, 0), (0, 0))).astype(dt)
    wav_out, cache_istft = orc.istft_step(y, caches[1])
    return (wav_out, cache_stft, cache_istft, *h_out), frac


@functools.lru_cache(maxsize=None)
def _floor_reference(name):
    """six hops of three streams from zero state: the input, the composed oracle's output and overlap tail with GAINS, the same with no
    limit; the oracle-side checks that the comparison is not vacuous are made here, once per shape"""
    cfg, sd, fused, orc = build_oracle(name)
    H, B = cfg.hop_size, len(GAINS)
    x = (0.1 * torch.randn(B, HOPS * H, generator=torch.Generator().manual_seed(77))).numpy()
    lim, off, plain = orc.initialize_cache(B), orc.initialize_cache(B), orc.initialize_cache(B)
    out_lim, out_off, out_plain = [], [], []
    for t in range(HOPS):
        xt = x[:, t * H:(t + 1) * H]
        (o, *lim), frac = _oracle_step_with_floor(orc, xt, lim, GAINS)
        assert 0.10 < frac[1] < 0.90, f"{name} hop {t}: {frac[1]:.0%} of the 0.01 stream's bins are floored - the case does not exercise the floor"
        assert frac[0] == 0.0
        out_lim.append(o)
        (o, *off), _ = _oracle_step_with_floor(orc, xt, off, [0.0] * B)
        out_off.append(o)
        o, *plain = orc.step(xt, *plain)
        out_plain.append(o)
    out_lim, out_off, out_plain = (np.concatenate(v, axis=1) for v in (out_lim, out_off, out_plain))
    # with no limit the composition is FEOracle.step
    assert rms(out_off - out_plain) <= 2e-7 * rms(out_plain)
    for i in (1, 2):
        assert rms(out_lim[i] - out_plain[i]) > 1e-3 * rms(out_plain[i]), f"{name}: the floor of stream {i} changes nothing"
    return x, out_lim, np.asarray(lim[1]), out_plain


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return rms(got - ref) / max(rms(ref), 1e-3)


@pytest.mark.parametrize("name,kernel,TM", [("fe_t", "wg8", 1), ("fe_b", "wg8", 1), ("fe_b", "waves4", 2), ("fe48_b_h480", "wg8", 1), ("fe_tk_b", "wg8", 1),
                                            ("fe_dpt_b", "wg8", 1)])
def test_the_limit_is_the_floor_formula_on_the_oracle_mask_and_touches_the_output_path_only(name, kernel, TM):
    x, ref_out, ref_tail, ref_plain = _floor_reference(name)
    eng = _engine(name)
    H, cap, B = eng.cfg.hop_size, 8, len(GAINS)
    slots = [5, 2, 6]
    gains = [0.0] * cap
    for s, g in zip(slots, GAINS):
        gains[s] = g
    xd = torch.from_numpy(x).to(_dev())
    runs = {}
    with _kernel(eng, kernel):
        for what, table in (("limit", _table(gains)), ("plain", None)):
            st = eng.new_state(cap)
            y = torch.zeros(B, HOPS * H, device=_dev())
            for t in range(0, HOPS, TM):
                d = _desc([(slots[i], TM, i * HOPS * H + t * H, i * HOPS * H + t * H) for i in range(B)])
                eng.step_streams(xd.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=table)
                if name == "fe_b":                                               # both kernels: the 512-thread per-hop one and the four-wave one
                    assert ("fe_frame8_kernel" in eng.last_step_kernel()) == (kernel == "wg8"), eng.last_step_kernel()
            torch.cuda.synchronize()
            runs[what] = (y.cpu().numpy(), st)
    y, st = runs["limit"]
    y_plain, st_plain = runs["plain"]
    sl = torch.tensor(slots, device=_dev())
    tail = _views(eng, st, cap)[1][sl].cpu().numpy()
    for i, g in enumerate(GAINS):
        for what, got, ref in (("output", y[i], ref_out[i]), ("cache_istft", tail[i], ref_tail[i])):
            rel = _rel(got, ref)
            print(f"stream_ctl parity {name} {kernel} T_max {TM} min_gain {g}: {what} relative rms {rel:.3e}")
            assert rel <= NORTH_STAR, f"{what} of the stream with min_gain {g}: relative rms {rel:.3e} (north_star bound 1e-4)"
            # (the family's regression bound holds for the floored streams as it stands: 1.6e-6 at most on the MI355X, all shapes, output and tail)
            assert rel <= FAMILY_REL, f"{what} of the stream with min_gain {g}: relative rms {rel:.3e} > {FAMILY_REL:.1e}"
    assert _rel(y_plain, ref_plain) <= FAMILY_REL
    assert np.array_equal(y[0], y_plain[0]), "the stream without a limit is not the plain run's"
    for i in (1, 2):
        assert rms(y[i] - y_plain[i]) > 1e-3 * rms(y_plain[i]), "the limit changed nothing on the GPU"
    for j, (a, b) in enumerate(zip(_views(eng, st, cap), _views(eng, st_plain, cap))):
        if j != 1:                                                                   # (1: cache_istft, the output path's overlap tail)
            assert _same(a, b), f"state tensor {j}: the limit reached beyond the output path"
    assert not _same(_views(eng, st, cap)[1][sl[1:]], _views(eng, st_plain, cap)[1][sl[1:]])


# ------------------------------------------------------------------ 3. clamping
@pytest.mark.parametrize("name,kernel,TM", [("fe_b", "wg8", 1), ("fe_b", "waves4", 2)])
def test_min_gain_is_clamped_to_0_1(name, kernel, TM):
    eng = _engine(name)
    H, cap, n = eng.cfg.hop_size, 6, 4
    with _kernel(eng, kernel):
        full = _seeded_state(eng, cap)
        x = _audio((n, TM * H), torch.float32, False, gen=torch.Generator().manual_seed(5))
        d = _desc([(i + 1, TM, i * TM * H, i * TM * H) for i in range(n)])
        res = []
        for g in ([0.0, 2.0, -1.0, 1.0, 1e9, 0.0], [0.0, 1.0, 0.0, 1.0, 1.0, 0.0]):
            st, y = full.clone(), _audio((n, TM * H), torch.float32, False, fill=0.0)
            eng.step_streams(x.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=_table(g))
            torch.cuda.synchronize()
            res.append((y, st))
        st, y = full.clone(), _audio((n, TM * H), torch.float32, False, fill=0.0)
        eng.step_streams(x.view(-1), st, cap, d, y.view(-1), T_max=TM)
        torch.cuda.synchronize()
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1]), "2.0 / 1e9 are not 1.0, or -1 is not 0"
    assert _same(res[0][0][1], y[1]), "min_gain -1 is not the plain step"
    assert not _same(res[0][0][0], y[0]), "min_gain 1 changed nothing"


# ------------------------------------------------------------------ 4. levels
def _expected_levels(x, y):
    """fp64 sums and exact float peaks of float32 rows"""
    x, y = x.double().reshape(-1), y.double().reshape(-1)
    return float((x * x).sum()), float(x.abs().max()), float((y * y).sum()), float(y.abs().max())


@pytest.mark.parametrize("name,kernel,TM,n", [("fe_b", "wg8", 1, 1), ("fe_b", "wg8", 1, 300), ("fe_b", "waves4", 3, 1), ("fe_b", "waves4", 3, 300),
                                              ("fe48_b_h480", "wg8", 2, 7), ("fe_t", "wg8", 1, 7)])
def test_level_rows_are_exact_peaks_and_fp32_sums_and_do_not_depend_on_how_the_audio_comes(name, kernel, TM, n):
    eng = _engine(name)
    H, cap = eng.cfg.hop_size, n + 5
    rng = np.random.default_rng(n)
    slots = [int(s) for s in rng.permutation(cap)[:n]]
    hops = [TM] if n == 1 else [(i % (TM + 1)) for i in range(n)]                    # 0 .. TM hops
    row = TM * H
    with _kernel(eng, kernel):
        full = _seeded_state(eng, cap)
        s16 = _audio((n, row), torch.int16, False, gen=torch.Generator().manual_seed(n + 9), scale=0.2)
        xf = (s16.float() / 32768.0).contiguous()
        d = _desc([(slots[i], hops[i], i * row, i * row) for i in range(n)])
        rows = {}
        for what, x, pinned in (("f32", xf, False), ("f32 again", xf, False), ("s16", s16, False), ("f32 pinned", xf.cpu().pin_memory(), True),
                                ("s16 pinned", s16.cpu().pin_memory(), True)):
            st = full.clone()
            y = _audio((n, row), x.dtype, pinned, fill=0)
            lv = _levels(cap, pinned=pinned)
            _step(eng, pinned)(x.view(-1), st, cap, d, y.view(-1), T_max=TM, levels=lv)
            torch.cuda.synchronize()
            rows[what] = (lv.cpu().clone(), y.cpu().clone())
        # another place in the batch: the streams in reverse order
        st = full.clone()
        y = _audio((n, row), torch.float32, False, fill=0)
        lv = _levels(cap)
        back = list(range(n))[::-1]
        eng.step_streams(xf.view(-1), st, cap, _desc([(slots[i], hops[i], i * row, i * row) for i in back]), y.view(-1), T_max=TM, levels=lv)
        torch.cuda.synchronize()
        rows["f32 reversed"] = (lv.cpu().clone(), y.cpu().clone())
    lv, y = rows["f32"]
    for what, (other, _) in rows.items():
        assert torch.equal(other.view(torch.int32), lv.view(torch.int32)), f"the level rows of the {what} call are not those of the f32 call"
    named = torch.zeros(cap, dtype=torch.bool)
    for i in range(n):
        named[slots[i]] = hops[i] > 0
    assert bool((lv[~named] == SENTINEL).all()), "a row of a stream without a hop, or of a slot not named, was written"
    for i in range(n):
        h = hops[i]
        if h == 0:
            continue
        cnt = h * H
        want = _expected_levels(xf[i, :cnt].cpu(), y[i, :cnt])
        got = [float(v) for v in lv[slots[i]]]
        assert got[1] == want[1] and got[3] == want[3], f"stream {i}: peaks {got[1]}, {got[3]} are not {want[1]}, {want[3]}"
        tol = 2.0 * cnt * 2.0 ** -24
        assert abs(got[0] - want[0]) <= tol * want[0], f"stream {i}: in_sumsq {got[0]} vs {want[0]}"
        assert abs(got[2] - want[2]) <= tol * want[2], f"stream {i}: out_sumsq {got[2]} vs {want[2]}"
        assert want[0] > 0 and want[2] > 0


@pytest.mark.parametrize("TM", [1, 3])
def test_level_rows_of_bad_descriptors_keep_the_sentinel(TM):
    eng = _engine("fe_b")
    H, cap = eng.cfg.hop_size, 16
    row = TM * H
    count = 12 * row
    rows = [
        (3, TM, 0, 0),                                  # good
        (4, 1, count + 5, 1 * row),                     # input past the end
        (5, 1, 1 * row, count),                         # output past the end
        (6, 1, -7, 2 * row),                            # negative input offset
        (7, 1, 2 * row, -1),                            # negative output offset
        (8, -3, 3 * row, 3 * row),                      # negative hop count: none
        (9, TM + 5, 4 * row, 4 * row),                  # too many hops: T_max of them
        (cap + 2, 1, 5 * row, 5 * row),                 # slot out of range
        (-1, TM, 6 * row, 6 * row),                     # slot out of range
        (10, TM, count - row + 1, 7 * row),             # input range straddles the end
        (11, TM, 8 * row, count - row + 1),             # output range straddles the end
        (12, 1, 2 ** 62, 9 * row),                      # an offset that would overflow
        (13, 1, 9 * row, -2 ** 63),
        (14, TM, count - row, count - row),             # good: the last rows of both buffers
        (15, 0, 10 * row, 10 * row),                    # no hop
    ]
    with _kernel(eng, "wg8" if TM == 1 else "waves4"):
        full = _seeded_state(eng, cap)
        x = _audio((count,), torch.float32, False, gen=torch.Generator().manual_seed(2))
        y = _audio((count,), torch.float32, False, fill=0.0)
        guard = torch.full((cap + 2, 4), SENTINEL, device=_dev())         # a row before and a row after the table
        lv = guard[1:cap + 1]
        eng.step_streams(x, full, cap, _desc(rows), y, T_max=TM, levels=lv)
        torch.cuda.synchronize()
    written = (guard != SENTINEL).any(dim=1).nonzero().flatten().tolist()
    assert written == [1 + 3, 1 + 9, 1 + 14], f"rows written: table slots {[w - 1 for w in written]}"
    for slot, off in ((3, 0), (9, 4 * row), (14, count - row)):
        want = _expected_levels(x[off:off + row].cpu(), y[off:off + row].cpu())
        got = [float(v) for v in lv[slot]]
        assert got[1] == want[1] and got[3] == want[3]


# ------------------------------------------------------------------ 5. graph capture
def test_a_captured_graph_follows_a_rewritten_gain_table():
    eng = _engine("fe_b")
    dev, H, cap, n = _dev(), eng.cfg.hop_size, 8, 4
    full = _seeded_state(eng, cap)
    x = _audio((n, H), torch.float32, False, gen=torch.Generator().manual_seed(3))
    d = _desc([(i, 1, i * H, i * H) for i in range(n)])
    gain, lv = _table([0.0] * cap), _levels(cap)
    y = _audio((n, H), torch.float32, False, fill=0.0)
    st = full.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                           # warm-up: nothing allocates in the capture
            eng.step_streams(x.view(-1), full.clone(), cap, d, y.view(-1), T_max=1, min_gain=gain, levels=lv)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step_streams(x.view(-1), st, cap, d, y.view(-1), T_max=1, min_gain=gain, levels=lv)
    for r, table in enumerate(([0.0] * cap, [0.5, 0.0, 0.05, 1.0] + [0.0] * (cap - n))):
        gain.copy_(torch.tensor(table))
        st.copy_(full)
        lv.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        e_st, e_y, e_lv = full.clone(), torch.zeros_like(y), _levels(cap)
        eng.step_streams(x.view(-1), e_st, cap, d, e_y.view(-1), T_max=1, min_gain=_table(table), levels=e_lv)
        torch.cuda.synchronize()
        assert _same(y, e_y) and _same(st, e_st) and _same(lv, e_lv), f"replay {r}"
        if r == 0:
            first = y.clone()
    assert not _same(y[0], first[0]) and _same(y[1], first[1]), "the second replay did not follow the new table"


# ------------------------------------------------------------------ 6. LDS poison
@pytest.mark.parametrize("kernel,TM,n", [("wg8", 1, 7), ("wg8", 1, 300), ("waves4", 2, 7)])
def test_ctl_step_from_poisoned_lds_gives_the_bits_of_the_plain_run(kernel, TM, n):
    eng = _engine("fe_b")
    H, cap = eng.cfg.hop_size, n
    with _kernel(eng, kernel):
        full = _seeded_state(eng, cap)
        s = _audio((n, TM * H), torch.int16, False, gen=torch.Generator().manual_seed(14))
        d = _desc([(n - 1 - i, 0 if i % 5 == 2 else TM, i * TM * H, i * TM * H) for i in range(n)])
        gain = _table([0.0 if i % 2 else 0.05 for i in range(cap)])
        runs = []
        for poison in (False, True):
            st, y, lv = full.clone(), _audio((n, TM * H), torch.int16, False, fill=-999), _levels(cap)
            if poison:
                eng.poison_lds()
            eng.step_streams(s.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=gain, levels=lv)
            torch.cuda.synchronize()
            runs.append((y, st, lv))
    assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]) and _same(runs[0][2], runs[1][2])
    assert int((runs[0][2] == SENTINEL).all(dim=1).sum()) == len([i for i in range(n) if i % 5 == 2])


# ------------------------------------------------------------------ 7. end to end: PacketPool
def test_packet_pool_limits_equal_each_stream_run_alone_and_levels_match_the_audio_pulled():
    eng = _engine("fe_b")
    dev, H = _dev(), eng.cfg.hop_size
    limits = [None, -40.0, -20.0]
    n_streams, ticks, packet = len(limits), 40, 320                  # 20 ms at 16 kHz against a hop of 256 samples
    rng = np.random.default_rng(41)
    arrivals = rng.choice([0, 1, 1, 1, 2, 3], size=(ticks, n_streams))
    total = int(arrivals.sum(0).max()) * packet
    pcm = (0.2 * torch.randn(n_streams, total, generator=torch.Generator().manual_seed(42)) * 32768).round().clamp(-32768, 32767).to(torch.int16)

    def run(pool, members):
        """members: {stream index: slot}; pushes the recorded arrivals of those streams, ticks, pulls, checks levels() against the audio"""
        sent = {i: 0 for i in members}
        got = {i: [] for i in members}
        for t in range(ticks):
            for i, slot in members.items():
                for _ in range(int(arrivals[t, i])):
                    pool.push(slot, pcm[i, sent[i]:sent[i] + packet])
                    sent[i] += packet
            launched = {slot: hops for slot, hops, _, _ in pool.tick()}
            for i, slot in members.items():
                before = sum(v.numel() for v in got[i])
                out = pool.pull(slot)
                got[i].append(out)
                if slot in launched:
                    cnt = launched[slot] * H
                    assert out.numel() == cnt
                    lv = pool.levels(slot)
                    xin = pcm[i, before:before + cnt].double() / 32768.0
                    assert lv.samples == cnt and lv.in_peak == float(xin.abs().max())
                    assert abs(lv.in_sumsq - float((xin * xin).sum())) <= 2 * cnt * 2.0 ** -24 * float((xin * xin).sum())
                    # the output is metered before its quantisation: half an int16 step per sample
                    q = out.double() / 32768.0
                    assert abs(lv.out_peak - float(q.abs().max())) <= 0.5 / 32768 + 1e-7
                    assert abs(math.sqrt(lv.out_sumsq / cnt) - math.sqrt(float((q * q).mean()))) <= 0.5 / 32768 + 1e-7
                    assert lv.out_rms_dbfs == pytest.approx(10 * math.log10(lv.out_sumsq / cnt))
        return {i: torch.cat(v) for i, v in got.items()}

    with _kernel(eng, "waves4"):
        pool = PacketPool(eng, 5, ring_hops=16, T_max=3, meters=True)
        members = {}
        for i, db in enumerate(limits):
            members[i] = pool.open()
            pool.set_suppression_limit(members[i], db)
        together = run(pool, members)
        assert "streams, pinned, s16>" in eng.last_step_kernel()
        for i, db in enumerate(limits):
            solo = PacketPool(eng, 1, ring_hops=16, T_max=3, meters=True)
            slot = solo.open()
            solo.set_suppression_limit(slot, db)
            alone = run(solo, {i: slot})[i]
            assert alone.numel() > 20 * H and torch.equal(alone, together[i]), f"stream {i} (limit {db} dB) differs from the same stream run alone"
    assert not torch.equal(together[1], together[2])
    # the stream without a limit is the plain pool's
    plain = PacketPool(eng, 1, ring_hops=16, T_max=3)
    with _kernel(eng, "waves4"):
        slot = plain.open()
        sent, got = 0, []
        for t in range(ticks):
            for _ in range(int(arrivals[t, 0])):
                plain.push(slot, pcm[0, sent:sent + packet])
                sent += packet
            plain.tick()
            got.append(plain.pull(slot))
    assert torch.equal(torch.cat(got), together[0])

