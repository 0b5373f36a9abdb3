"""fe_step_pool_streams_ctl[_pinned] on the GPU: the packet step's suppression limit and level meters for BSRNN, FSPEN and LiSenNet
(Engine.step_pool_streams_ctl*, serving.FamilyPacketPool).

Off must be off - null tables, zeros and NaN give the bits, the state and the kernel strings of fe_step_pool_streams; the limit must be the
contract's formula on the output bin against the input bin (tests/pool_ctl_oracle.py: the oracle's step with the floor in float64) and touch nothing but the output path; the level
rows must be exact peaks and fp32 sums, bitwise reproducible, and written for the streams that advanced only.  Models and kernels: CASES of
tests/test_gpu_pool_streams.py (bsrnn_xxt with both PART 1 kernels, bsrnn_s, fspen, lisennet)."""
import math

import numpy as np
import pytest
import torch

import pool_ctl_oracle as pco
from common import rms
from fastenhancer_amd.serving import FamilyPacketPool, PacketPool
from test_gpu_parity import TIGHT_REL
from test_gpu_pool_streams import CASES, _names_ok, _packet, _sized, _three_launches
from test_gpu_step_chunk import _dev, _engine, _same, _seeded_state
from test_gpu_stream_ctl import SENTINEL, _expected_levels, _levels, _table
from test_gpu_stream_packets import _audio, _desc, _kernel

pytestmark = pytest.mark.gpu

NORTH_STAR = 1e-4
# Relative rms of output and overlap tail against the oracle's composed step, measured on the MI355X (profiles/pool_stream_ctl_parity.txt), all
# cases, T_max 1 and 2, limited and unlimited streams: see MEASURED below.  The regression bound is 5x the largest value measured, not below
# the family's TIGHT_REL of tests/test_gpu_parity.py.
MEASURED = {"bsrnn": 1.79e-6, "fspen": 1.16e-6, "lisennet": 4.1e-7}       # the largest of each family (bsrnn: xxt, T_max 2, gain 0.25, cache_istft)
REGRESSION_REL = {fam: max(TIGHT_REL[fam], 5.0 * (MEASURED[fam] or 0.0)) for fam in MEASURED}


def _family(name):
    return name.split("_")[0]


def _ctl(eng, pinned):
    return eng.step_pool_streams_ctl_pinned if pinned else eng.step_pool_streams_ctl


def _tensors(eng, state, cap):
    """(cache_stft, cache_istft, everything else) of a state sized for cap streams: the first two tensors of every family's layout"""
    n = cap * eng.cfg.cache_len
    return state[:n].view(cap, -1), state[n:2 * n].view(cap, -1), state[2 * n:]


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("TM,n", [(1, 5), (3, 7)])
@pytest.mark.parametrize("name,kern", CASES)
def test_null_zero_and_nan_gain_tables_give_the_bits_of_the_plain_packet_step(name, kern, TM, n, pinned, dtype):
    eng = _engine(name)
    H, cap = eng.cfg.hop_size, n + 4
    slots = [int(s) for s in np.random.default_rng(n + TM).permutation(cap)[:n]]
    hops = [TM] * n if TM == 1 else [(i % TM) + 1 for i in range(n)]                  # ragged where one kernel walks the frames
    with _kernel(eng, kern):
        _sized(eng, cap)
        full = _seeded_state(eng, cap, 4, seed=31)
        x = _audio((n, TM * H), dtype, pinned, gen=torch.Generator().manual_seed(32))
        d = _desc([(slots[i], hops[i], i * TM * H, i * TM * H) for i in range(n)])
        fill = 7.0 if dtype == torch.float32 else 777
        st0, y0 = full.clone(), _audio((n, TM * H), dtype, pinned, fill=fill)
        _packet(eng, pinned)(x.view(-1), st0, cap, d, y0.view(-1), T_max=TM)
        k0 = eng.last_step_kernel()
        torch.cuda.synchronize()
        _names_ok(k0)
        if TM == 1:
            _three_launches(name, kern, k0)
        st, y = full.clone(), _audio((n, TM * H), dtype, pinned, fill=fill)
        _ctl(eng, pinned)(x.view(-1), st, cap, d, y.view(-1), T_max=TM)                # both tables NULL: the same code path
        assert eng.last_step_kernel() == k0
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), y0.view(torch.int16)) and _same(st, st0), "both tables NULL: not fe_step_pool_streams"
        for what, gain in (("null", None), ("zeros", _table([0.0] * cap)), ("nan", _table([float("nan")] * cap))):
            st, y, lv = full.clone(), _audio((n, TM * H), dtype, pinned, fill=fill), _levels(cap)
            _ctl(eng, pinned)(x.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=gain, levels=lv)
            assert eng.last_step_kernel() == k0, "the ctl entry points pick the kernels of fe_step_pool_streams, under their names"
            torch.cuda.synchronize()
            assert torch.equal(y.view(torch.int16), y0.view(torch.int16)), f"{what}: output differs from fe_step_pool_streams"
            for j, (a, b) in enumerate(zip(_tensors(eng, st, cap), _tensors(eng, st0, cap))):
                assert _same(a, b), f"{what}: state tensor {j} differs from fe_step_pool_streams"
            assert bool((lv[torch.tensor(slots)] != SENTINEL).all()), f"{what}: the level rows were not written"
            assert int((lv != SENTINEL).any(dim=1).sum()) == n
    assert not _same(st0, full)


# ------------------------------------------------------------------ 2. the limit against the reference
@pytest.mark.parametrize("TM", [1, 2])
@pytest.mark.parametrize("name,kern", CASES)
def test_the_limit_is_the_contracts_formula_and_touches_the_output_path_only(name, kern, TM):
    ref = pco.reference(name)
    GAINS, HOPS = pco.GAINS, pco.HOPS
    eng = _engine(name)
    H, cap, B = eng.cfg.hop_size, 8, len(GAINS)
    slots = [5, 2, 6]
    gains = [0.0] * cap
    for s, g in zip(slots, GAINS):
        gains[s] = g
    xd = torch.from_numpy(ref["x"]).to(_dev())
    runs = {}
    with _kernel(eng, kern):
        _sized(eng, cap)
        for what in ("limit", "plain"):
            st = eng.new_state(cap)
            y = torch.zeros(B, HOPS * H, device=_dev())
            for t in range(0, HOPS, TM):
                d = _desc([(slots[i], TM, i * HOPS * H + t * H, i * HOPS * H + t * H) for i in range(B)])
                if what == "limit":
                    eng.step_pool_streams_ctl(xd.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=_table(gains))
                else:
                    eng.step_pool_streams(xd.view(-1), st, cap, d, y.view(-1), T_max=TM)
                k = eng.last_step_kernel()
                _names_ok(k)
                if TM == 1:
                    _three_launches(name, kern, k)
            torch.cuda.synchronize()
            runs[what] = (y.cpu().numpy(), st)
    y, st = runs["limit"]
    y_plain, st_plain = runs["plain"]
    sl = torch.tensor(slots, device=_dev())
    tail = _tensors(eng, st, cap)[1][sl].cpu().numpy()
    fam = _family(name)
    for i, g in enumerate(GAINS):
        for what, got, want in (("output", y[i], ref["out"][i]), ("cache_istft", tail[i], ref["tail"][i])):
            rel = pco.rel_rms(got, want)
            print(f"pool_stream_ctl parity {name} {kern} T_max {TM} min_gain {g}: {what} relative rms {rel:.3e}")
            assert rel <= NORTH_STAR, f"{what} of the stream with min_gain {g}: relative rms {rel:.3e} (north_star bound 1e-4)"
            assert rel <= REGRESSION_REL[fam], f"{what} of the stream with min_gain {g}: relative rms {rel:.3e} > {REGRESSION_REL[fam]:.1e}"
    assert pco.rel_rms(y_plain, ref["plain"]) <= TIGHT_REL[fam]
    assert np.array_equal(y[0], y_plain[0]), "the stream without a limit is not the plain call's"
    for i in (1, 2):
        assert rms(y[i] - y_plain[i]) > 1e-3 * rms(y_plain[i]), "the limit changed nothing on the GPU"
    for j, (a, b) in enumerate(zip(_tensors(eng, st, cap), _tensors(eng, st_plain, cap))):
        if j != 1:                                                                   # (1: cache_istft, the output path's overlap tail)
            assert _same(a, b), f"state tensor {j}: the limit reached beyond the output path"
    assert _same(_tensors(eng, st, cap)[1][sl[:1]], _tensors(eng, st_plain, cap)[1][sl[:1]])
    assert not _same(_tensors(eng, st, cap)[1][sl[1:]], _tensors(eng, st_plain, cap)[1][sl[1:]])


# ------------------------------------------------------------------ 3. clamping
@pytest.mark.parametrize("name,TM", [("fspen", 2), ("bsrnn_xxt", 1)])
def test_min_gain_is_clamped_to_0_1(name, TM):
    eng = _engine(name)
    H, cap, n = eng.cfg.hop_size, 6, 4
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=33)
    x = _audio((n, TM * H), torch.float32, False, gen=torch.Generator().manual_seed(5))
    d = _desc([(i + 1, TM, i * TM * H, i * TM * H) for i in range(n)])
    res = []
    for g in ([0.0, 2.0, -1.0, 1.0, 1e9, 0.0], [0.0, 1.0, 0.0, 1.0, 1.0, 0.0]):
        st, y = full.clone(), _audio((n, TM * H), torch.float32, False, fill=0.0)
        eng.step_pool_streams_ctl(x.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=_table(g))
        torch.cuda.synchronize()
        res.append((y, st))
    st, y = full.clone(), _audio((n, TM * H), torch.float32, False, fill=0.0)
    eng.step_pool_streams(x.view(-1), st, cap, d, y.view(-1), T_max=TM)
    torch.cuda.synchronize()
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1]), "2.0 / 1e9 are not 1.0, or -1 is not 0"
    assert _same(res[0][0][1], y[1]), "min_gain -1 is not the plain step"
    assert not _same(res[0][0][0], y[0]), "min_gain 1 changed nothing"


# ------------------------------------------------------------------ 4. levels
def _check_level_rows(name, kern, TM, n):
    eng = _engine(name)
    H, cap = eng.cfg.hop_size, n + 5
    rng = np.random.default_rng(n)
    slots = [int(s) for s in rng.permutation(cap)[:n]]
    hops = [TM] if n == 1 else [(i % (TM + 1)) for i in range(n)]                    # 0 .. TM hops
    row = TM * H
    with _kernel(eng, kern):
        _sized(eng, cap)
        full = _seeded_state(eng, cap, 4, seed=34)
        s16 = _audio((n, row), torch.int16, False, gen=torch.Generator().manual_seed(n + 9), scale=0.2)
        xf = (s16.float() / 32768.0).contiguous()
        d = _desc([(slots[i], hops[i], i * row, i * row) for i in range(n)])
        rows = {}
        for what, x, pinned in (("f32", xf, False), ("f32 again", xf, False), ("s16", s16, False), ("f32 pinned", xf.cpu().pin_memory(), True),
                                ("s16 pinned", s16.cpu().pin_memory(), True)):
            st = full.clone()
            y = _audio((n, row), x.dtype, pinned, fill=0)
            lv = _levels(cap, pinned=pinned)
            _ctl(eng, pinned)(x.view(-1), st, cap, d, y.view(-1), T_max=TM, levels=lv)
            torch.cuda.synchronize()
            rows[what] = (lv.cpu().clone(), y.cpu().clone())
        k = eng.last_step_kernel()
        # another place in the batch: the streams in reverse order
        st = full.clone()
        y = _audio((n, row), torch.float32, False, fill=0)
        lv = _levels(cap)
        back = list(range(n))[::-1]
        eng.step_pool_streams_ctl(xf.view(-1), st, cap, _desc([(slots[i], hops[i], i * row, i * row) for i in back]), y.view(-1), T_max=TM, levels=lv)
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
    return k


@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("TM", [1, 3])
@pytest.mark.parametrize("name,kern", CASES)
def test_level_rows_are_exact_peaks_and_fp32_sums_and_do_not_depend_on_how_the_audio_comes(name, kern, TM, n):
    k = _check_level_rows(name, kern, TM, n)
    if TM == 1:
        _three_launches(name, kern, k)


@pytest.mark.parametrize("name", ["fspen", "bsrnn_xxt"])
def test_level_rows_of_the_persistent_forms(name):
    """300 streams: more than the workgroups resident at once, so a workgroup walks several streams and starts each with fresh accumulators"""
    _check_level_rows(name, "wg8", 1, 300)


@pytest.mark.parametrize("name,TM", [("lisennet", 3), ("bsrnn_xxt", 1)])
def test_level_rows_of_bad_descriptors_keep_the_sentinel(name, TM):
    eng = _engine(name)
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
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=35)
    x = _audio((count,), torch.float32, False, gen=torch.Generator().manual_seed(2))
    y = _audio((count,), torch.float32, False, fill=0.0)
    guard = torch.full((cap + 2, 4), SENTINEL, device=_dev())         # a row before and a row after the table
    lv = guard[1:cap + 1]
    eng.step_pool_streams_ctl(x, full, cap, _desc(rows), y, T_max=TM, min_gain=_table([0.2] * cap), levels=lv)
    torch.cuda.synchronize()
    written = (guard != SENTINEL).any(dim=1).nonzero().flatten().tolist()
    assert written == [1 + 3, 1 + 9, 1 + 14], f"rows written: table slots {[w - 1 for w in written]}"
    for slot, off in ((3, 0), (9, 4 * row), (14, count - row)):
        want = _expected_levels(x[off:off + row].cpu(), y[off:off + row].cpu())
        got = [float(v) for v in lv[slot]]
        assert got[1] == want[1] and got[3] == want[3]


# ------------------------------------------------------------------ 5. graph capture
def test_a_captured_graph_follows_a_rewritten_gain_table():
    """bsrnn_xxt, T_max = 1: the three launches as a linear chain; gains and level rows are read and written when the kernels run"""
    eng = _engine("bsrnn_xxt")
    dev, H, cap, n = _dev(), eng.cfg.hop_size, 8, 4
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=36)
    x = _audio((n, H), torch.float32, False, gen=torch.Generator().manual_seed(3))
    d = _desc([(i, 1, i * H, i * H) for i in range(n)])
    gain, lv = _table([0.0] * cap), _levels(cap)
    y = _audio((n, H), torch.float32, False, fill=0.0)
    st = full.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                           # warm-up: nothing allocates in the capture
            eng.step_pool_streams_ctl(x.view(-1), full.clone(), cap, d, y.view(-1), T_max=1, min_gain=gain, levels=lv)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step_pool_streams_ctl(x.view(-1), st, cap, d, y.view(-1), T_max=1, min_gain=gain, levels=lv)
    _three_launches("bsrnn_xxt", "wg8", eng.last_step_kernel())
    for r, table in enumerate(([0.0] * cap, [0.5, 0.0, 0.2, 1.0] + [0.0] * (cap - n))):
        gain.copy_(torch.tensor(table))
        st.copy_(full)
        lv.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        e_st, e_y, e_lv = full.clone(), torch.zeros_like(y), _levels(cap)
        eng.step_pool_streams_ctl(x.view(-1), e_st, cap, d, e_y.view(-1), T_max=1, min_gain=_table(table), levels=e_lv)
        torch.cuda.synchronize()
        assert _same(y, e_y) and _same(st, e_st) and _same(lv, e_lv), f"replay {r}"
        assert bool((lv[:n] != SENTINEL).all()) and bool((lv[n:] == SENTINEL).all())
        if r == 0:
            first = y.clone()
    assert not _same(y[0], first[0]) and _same(y[1], first[1]), "the second replay did not follow the new table"


# ------------------------------------------------------------------ 6. LDS poison
@pytest.mark.parametrize("name,TM,n", [("fspen", 2, 7), ("lisennet", 2, 7), ("bsrnn_s", 1, 7)])
def test_ctl_step_from_poisoned_lds_gives_the_bits_of_the_unpoisoned_run(name, TM, n):
    eng = _engine(name)
    H, cap = eng.cfg.hop_size, n
    _sized(eng, cap)
    full = _seeded_state(eng, cap, 4, seed=37)
    s = _audio((n, TM * H), torch.int16, False, gen=torch.Generator().manual_seed(14))
    d = _desc([(n - 1 - i, 0 if i % 5 == 2 else TM, i * TM * H, i * TM * H) for i in range(n)])
    gain = _table([0.0 if i % 2 else 0.2 for i in range(cap)])
    runs = []
    for poison in (False, True):
        st, y, lv = full.clone(), _audio((n, TM * H), torch.int16, False, fill=-999), _levels(cap)
        if poison:
            eng.poison_lds()
        eng.step_pool_streams_ctl(s.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=gain, levels=lv)
        torch.cuda.synchronize()
        runs.append((y, st, lv))
    assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]) and _same(runs[0][2], runs[1][2])
    assert bool(torch.isfinite(runs[1][1]).all()) and bool(torch.isfinite(runs[1][2]).all())
    assert int((runs[0][2] == SENTINEL).all(dim=1).sum()) == len([i for i in range(n) if i % 5 == 2])


# ------------------------------------------------------------------ 7. end to end: FamilyPacketPool
@pytest.mark.parametrize("name,TM", [("fspen", 3), ("bsrnn_xxt", 1)])
def test_family_packet_pool_limits_equal_each_stream_run_alone_and_levels_match_the_audio_pulled(name, TM):
    eng = _engine(name)
    H = eng.cfg.hop_size
    limits = [None, -40.0, -20.0]
    n_streams, ticks, packet = len(limits), 40, 320                  # 20 ms at 16 kHz against a hop of 256 samples
    rng = np.random.default_rng(41)
    arrivals = rng.choice([0, 1, 1, 1, 2, 3] if TM > 1 else [0, 1, 1, 1, 2], size=(ticks, n_streams))
    total = int(arrivals.sum(0).max()) * packet
    # (0.02: these models' seeded weights amplify - at 0.2 most of FSPEN's hops pass full scale)
    pcm = (0.02 * torch.randn(n_streams, total, generator=torch.Generator().manual_seed(42)) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    RING = 32                                                        # hops: at T_max = 1 a tick takes 256 samples where 320 arrive on average

    unclipped = [0]

    def run(pool, members, metered=True):
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
                if slot in launched and metered:
                    cnt = launched[slot] * H
                    assert out.numel() == cnt
                    lv = pool.levels(slot)
                    xin = pcm[i, before:before + cnt].double() / 32768.0
                    assert lv.samples == cnt and lv.in_peak == float(xin.abs().max())
                    assert abs(lv.in_sumsq - float((xin * xin).sum())) <= 2 * cnt * 2.0 ** -24 * float((xin * xin).sum())
                    # the output is metered before its quantisation: half an int16 step per sample - where the hop stays inside full scale; a hop
                    # that passes it (FSPEN's seeded weights give output near 1 whatever the input level) is clamped on its way out, the meter is not
                    q = out.double() / 32768.0
                    if lv.out_peak < 1.0 - 1.0 / 32768:
                        unclipped[0] += 1
                        assert abs(lv.out_peak - float(q.abs().max())) <= 0.5 / 32768 + 1e-7
                        assert abs(math.sqrt(lv.out_sumsq / cnt) - math.sqrt(float((q * q).mean()))) <= 0.5 / 32768 + 1e-7
                    else:
                        assert float(q.abs().max()) >= 32767.0 / 32768
                    assert lv.out_rms_dbfs == pytest.approx(10 * math.log10(lv.out_sumsq / cnt))
        return {i: torch.cat(v) for i, v in got.items()}

    pool = FamilyPacketPool(eng, 5, ring_hops=RING, T_max=TM, meters=True)
    members = {}
    for i, db in enumerate(limits):
        members[i] = pool.open()
        pool.set_suppression_limit(members[i], db)
    together = run(pool, members)
    assert unclipped[0] > 40, "the precise comparison of the output meter needs hops inside full scale"
    assert "slots, streams, pinned, s16" in eng.last_step_kernel()
    for i, db in enumerate(limits):
        solo = FamilyPacketPool(eng, 1, ring_hops=RING, T_max=TM, meters=True)
        slot = solo.open()
        solo.set_suppression_limit(slot, db)
        alone = run(solo, {i: slot})[i]
        assert alone.numel() > 20 * H and torch.equal(alone, together[i]), f"stream {i} (limit {db} dB) differs from the same stream run alone"
    assert not torch.equal(together[1], together[2])
    # the stream without a limit is the plain pool's
    plain = PacketPool(eng, 1, ring_hops=RING, T_max=TM)
    assert torch.equal(run(plain, {0: plain.open()}, metered=False)[0], together[0])
