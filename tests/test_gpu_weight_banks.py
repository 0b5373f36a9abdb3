"""Weight banks on the GPU (fe_set_weight_banks / fe_load_weights_bank / fe_step_streams_banked[_pinned] through Engine and PacketPool): the
streams of one packet batch on different checkpoints of a shape.

Bank k of the banked engine holds make_training_state_dict(cfg, seed + k); the references are one-bank engines of the same checkpoints -
code paths the goldens already pin.  Every stream of a banked call must be, bit for bit, what fe_step_streams_ctl gives it on the one-bank
engine of its bank under the same kernel: the reference launch of bank k is the banked launch's own descriptor list with the hop counts of
the other banks' streams set to 0, so that grid, instantiation and the walk of every workgroup are the same."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from common import MODEL_KWARGS, MODEL_MODULE, hip_model, product_config, rms
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool
from oracle.fe_oracle import FEConfig, FEOracle, fold_state_dict
from oracle.weightgen import make_training_state_dict
from test_gpu_stream_packets import _audio, _desc, _step
from test_gpu_stream_slots import _dev, _engine, _same, _seeded_state, _views

pytestmark = pytest.mark.gpu

BANKS = 3
SHAPES = ["fe_t", "fe_b", "fe48_b_h480", "fe_tk_b", "fe_dpt_b", "fe_m"]      # (fe_m: conv weights not staged in LDS)
# every streaming shape the library ships (fe_shapes.def): each has banked per-hop, persistent, generic and companion instantiations of its own
ALL_SHAPES = ["fe_t", "fe_b", "fe_s", "fe_m", "fe_l", "fe48_t", "fe48_b", "fe48_s", "fe48_m", "fe48_l", "fe48_b_h480", "fe_tk_b", "fe_dprnn_t", "fe_dprnn_b",
              "fe_dprnn_s", "fe_dprnn_m", "fe_dprnn_l", "fe_dpt_t", "fe_dpt_b", "fe_dpt_s", "fe_dpt_m", "fe_ln_b"]
TIGHT = 2e-5               # tests/test_gpu_parity.py TIGHT_REL["fastenhancer"], tests/test_gpu_model_options.py
SENTINEL = -77.0
FILL = 7.0


@functools.lru_cache(maxsize=None)
def _checkpoints(name):
    """(oracle config, [training-form state dict of bank k])"""
    kw, _, seed = MODEL_KWARGS[name]
    cfg = FEConfig.from_model_kwargs(kw, variant=MODEL_MODULE[name].split(".")[-1])
    return cfg, [make_training_state_dict(cfg, seed + k) for k in range(BANKS + 1)]     # (the last one: test 6's second checkpoint of bank 1)


def _torch_sd(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    """the one-bank engine of checkpoint k (checkpoint 0's is the engine the other test modules share)"""
    return _engine(name) if k == 0 else hip_model(name, device=_dev(), sd=_checkpoints(name)[1][k]).engine


def _refs(name):
    return [_ref(name, k) for k in range(BANKS)]


def _new_banked(name, n_banks=BANKS):
    _, sds = _checkpoints(name)
    eng = hip_model(name, device=_dev(), load=False).engine
    eng.set_weight_banks(n_banks)
    assert eng.weight_banks == n_banks
    for k in range(n_banks):
        eng.load_state_dict(_torch_sd(sds[k]), bank=k)
    return eng


@functools.lru_cache(maxsize=None)
def _banked(name):
    return _new_banked(name)


@contextlib.contextmanager
def _setup(engines, kernel, low=None):
    """step kernel (and low_lds_companion) on every engine of a comparison; put back afterwards - the engines are shared"""
    for e in engines:
        e.set_step_kernel(kernel)
        if low is not None:
            e.set_option("low_lds_companion", low)
    try:
        yield
    finally:
        for e in engines:
            e.set_step_kernel("wg8")
            e.set_option("low_lds_companion", 1)


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


def _strip_banks(k):
    return k.replace(", banks>", ">")


def _bank_table(cap, rows, pinned=False):
    t = torch.zeros(cap, dtype=torch.int32)
    for slot, _, bank in rows:
        if 0 <= slot < cap:
            t[slot] = bank
    return t.pin_memory() if pinned else t.to(_dev())


def _check_banked(name, kernel, TM, rows, cap, low=None, dtype=torch.float32, seed=5):
    """rows: (slot, hops, bank) per stream of the call.  The banked launch against, per bank, the one-bank engine's launch of the same list with
    the other streams' hops at 0: rows, state, level rows; streams that are skipped - 0 hops, a slot or a bank out of range - change nothing
    (zero rows for the last two)."""
    eng, refs = _banked(name), _refs(name)
    H, n = eng.cfg.hop_size, len(rows)
    row = TM * H
    fill = FILL if dtype == torch.float32 else 777
    with _setup([eng] + refs, kernel, low):
        full = _seeded_state(refs[0], cap)
        x = _audio((n, row), dtype, False, gen=torch.Generator().manual_seed(seed))
        live = [0 <= s < cap and 0 <= b < BANKS and h > 0 for s, h, b in rows]
        st, y, lv = full.clone(), _audio((n, row), dtype, False, fill=fill), torch.full((cap, 4), SENTINEL, device=_dev())
        eng.step_streams(x.view(-1), st, cap, _desc([(s, h, i * row, i * row) for i, (s, h, _) in enumerate(rows)]), y.view(-1), T_max=TM, levels=lv,
                         bank=_bank_table(cap, rows))
        k_banked = eng.last_step_kernel()
        torch.cuda.synchronize()
        ref = {}
        for k in sorted({b for (s, h, b), ok in zip(rows, live) if ok}):
            st_k, y_k, lv_k = full.clone(), _audio((n, row), dtype, False, fill=fill), torch.full((cap, 4), SENTINEL, device=_dev())
            d_k = _desc([(s, h if b == k else 0, i * row, i * row) for i, (s, h, b) in enumerate(rows)])
            refs[k].step_streams(x.view(-1), st_k, cap, d_k, y_k.view(-1), T_max=TM, levels=lv_k)
            k_ref = refs[k].last_step_kernel()
            torch.cuda.synchronize()
            assert ", banks>" in k_banked and _strip_banks(k_banked) == k_ref, (k_banked, k_ref)
            ref[k] = (y_k, _views(refs[0], st_k, cap), lv_k)
    vs, v0 = _views(refs[0], st, cap), _views(refs[0], full, cap)
    zero, untouched = torch.zeros_like(y[0]), torch.full_like(y[0], fill)
    named = torch.zeros(cap, dtype=torch.bool, device=_dev())
    for i, ((s, h, b), ok) in enumerate(zip(rows, live)):
        hh = min(max(h, 0), TM)
        if not ok:
            assert torch.equal(y[i, :hh * H], zero[:hh * H]), f"stream {i} (slot {s}, bank {b}): the rows of a stream without state or bank are not zero"
            assert torch.equal(y[i, hh * H:], untouched[hh * H:]), f"stream {i}: rows past its hops were written"
            continue
        named[s] = True
        y_k, v_k, lv_k = ref[b]
        assert torch.equal(y[i], y_k[i]), f"stream {i} (slot {s}, {h} hops, bank {b}): rows differ from the one-bank engine of its checkpoint"
        for j, (a, r) in enumerate(zip(vs, v_k)):
            assert _same(a[s], r[s]), f"stream {i} (slot {s}, {h} hops, bank {b}): state tensor {j} differs from the one-bank engine's"
        assert _same(lv[s], lv_k[s]) and float(lv[s, 0]) != SENTINEL, f"stream {i}: level row"
    for j, (a, r) in enumerate(zip(vs, v0)):
        assert _same(a[~named], r[~named]), f"state tensor {j} of a slot that is not named, has no hop or no bank changed"
    assert bool((lv[~named] == SENTINEL).all()), "a level row of a skipped stream or of a slot not named was written"
    # the checkpoints differ: a stream on the wrong bank would not pass
    banks_live = sorted(ref)
    if len(banks_live) > 1:
        i = next(i for i, ((s, h, b), ok) in enumerate(zip(rows, live)) if ok and b == banks_live[1])
        s, h, _ = rows[i]
        st_w, y_w = full.clone(), _audio((n, row), dtype, False, fill=fill)
        with _setup([refs[banks_live[0]]], kernel, low):
            refs[banks_live[0]].step_streams(x.view(-1), st_w, cap, _desc([(s, h, i * row, i * row)]), y_w.view(-1), T_max=TM)
            torch.cuda.synchronize()
        assert not torch.equal(y_w[i, :H], y[i, :H]), "two banks give the same output: the comparison shows nothing"
    return k_banked


def _mixed_rows(n, cap, TM, seed):
    """slots permuted, banks pseudo-random (consecutive streams of a workgroup differ), hop counts mixed over 0 .. TM"""
    rng = np.random.default_rng(seed)
    slots = [int(s) for s in rng.permutation(cap)[:n]]
    if n == 1:
        return [(slots[0], TM, 1)]
    banks = [int(b) for b in rng.permutation([i % BANKS for i in range(n)])]
    hops = [int(h) for h in rng.permutation([(TM, 0, TM, 1, TM, TM - 1)[i % 6] for i in range(n)])]
    assert len(set(banks)) == BANKS and 0 in hops and TM in hops and slots != sorted(slots)
    return list(zip(slots, hops, banks))


# ------------------------------------------------------------------ 1. each stream is its own checkpoint's run
@pytest.mark.parametrize("kernel", ["waves4", "wg8"])
@pytest.mark.parametrize("TM", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 37])
@pytest.mark.parametrize("name", SHAPES)
def test_each_stream_is_the_run_of_its_own_checkpoint(name, n, TM, kernel):
    k = _check_banked(name, kernel, TM, _mixed_rows(n, n + 6, TM, seed=n + TM), n + 6)
    if name == "fe_b" and TM == 1:
        assert k.startswith("fe_frame8_kernel" if kernel == "wg8" else "fe_frame_kernel"), k
    if TM == 3:
        assert "generic, streams" in k, k


@pytest.mark.parametrize("TM", [1, 3])
@pytest.mark.parametrize("name", [n for n in ALL_SHAPES if n not in SHAPES])
def test_each_stream_is_the_run_of_its_own_checkpoint_on_the_other_shipped_shapes(name, TM):
    k = _check_banked(name, "wg8", TM, _mixed_rows(37, 43, TM, seed=37 + TM), 43)
    assert ("generic, streams" in k) == (TM == 3), k


# Every shipped shape, every kernel choice, low_lds_companion off and on: the banked persistent instantiations are code of their own per shape (one of
# them - 48 kHz B at hop 480, LOW = 2 - is sensitive to how its source is spelled: the note at fe_frame_kernel's BANK), so each is pinned here against
# the instantiation without banks.  #CUs + 9, 2 #CUs + 9 and 3 #CUs + 9 streams: workgroups that walk two live streams at one, two and three
# workgroups per CU.  (FE_STEP_KERNEL_WG8_PERSIST differs from the default for the shape of the 512-thread kernel only.)
@pytest.mark.parametrize("low", [0, 1])
@pytest.mark.parametrize("rounds", [1, 2, 3])
@pytest.mark.parametrize("name,kernel", [(name, kernel) for name in ALL_SHAPES for kernel in ("waves4", "wg8", "wg8_persist") if kernel != "wg8_persist" or name == "fe_b"])
def test_each_stream_is_the_run_of_its_own_checkpoint_above_the_cu_count(name, kernel, rounds, low):
    """the persistent walk of the shape's own kernels and the low-LDS companion"""
    n = rounds * _cus() + 9
    k = _check_banked(name, kernel, 1, _mixed_rows(n, n + 7, 1, seed=rounds + low), n + 7, low=low)
    if name == "fe_b":
        assert ("fe_frame8_kernel<persistent" in k) == (kernel == "wg8_persist"), k
        if low == 0:
            assert "LOW=" not in k and "persistent" in k, k


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_ragged_hop_counts_on_banks_above_the_cu_count(name):
    """the generic kernel's persistent walk: 0 .. 3 hops per stream, #CUs + 9 streams"""
    n = _cus() + 9
    k = _check_banked(name, "waves4", 3, _mixed_rows(n, n + 7, 3, seed=13), n + 7)
    assert "generic, streams" in k, k


# ------------------------------------------------------------------ 2. the requests issued ahead of the stream they are for
def _walk_rows(case, n, cap, TM, G):
    """streams b, b + G, b + 2 G are the walk of one workgroup of a grid of G workgroups (the test asserts the launch that makes G the grid)"""
    slots = [int(s) for s in np.random.default_rng(n).permutation(cap)[:n]]
    rows = []
    for b in range(n):
        w, pos = b % G, b // G
        last = (n - 1 - w) // G                       # position of the last stream of workgroup w
        hops, bank, slot = TM if case != "c" else 1, (b + pos) % 2, slots[b]
        if case == "a":                               # the first stream of every workgroup on bank 2 (the prologue has staged for it)
            bank = 2 if pos == 0 else (b % 2)
        elif case == "b" and last >= 1:               # bank 0, a skipped stream, bank 1 (two-stream walks: a skipped first stream, then bank 1)
            skipped = pos == last - 1
            bank = 1 if pos == last else 0
            if skipped:
                kind = w % 3
                hops, slot, bank = (0, slot, 2) if kind == 0 else (TM, cap + 3 + w, 0) if kind == 1 else (TM, slot, BANKS + w)
        elif case == "c" and last >= 1:               # a 3-hop stream on bank 1 between 1-hop streams on bank 0
            mid = pos == (1 if last >= 2 else 0)
            hops, bank = (TM, 1) if mid else (1, 0)
        rows.append((slot, hops, bank))
    return rows


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("case,kernel,TM", [("a", "waves4", 1), ("a", "wg8_persist", 1), ("b", "waves4", 1), ("b", "wg8_persist", 1), ("c", "waves4", 3),
                                            ("c", "wg8", 3)])
@pytest.mark.parametrize("name", ["fe_b", "fe_tk_b"])
def test_weight_requests_issued_ahead_follow_the_stream_they_are_for(name, case, kernel, TM, rounds):
    """the shapes' own kernels, one workgroup per CU: #CUs + 9 streams are a persistent launch only then, which the per-hop cases assert - and the
    generic kernel of a shape has the occupancy of its per-hop kernel"""
    n = rounds * _cus() + 9
    k = _check_banked(name, kernel, TM, _walk_rows(case, n, n + 5, TM, _cus()), n + 5, low=0)
    assert ("persistent" in k and "LOW=" not in k) if TM == 1 else "generic" in k, k


@pytest.mark.parametrize("case", ["a", "b"])
def test_weight_requests_issued_ahead_follow_the_stream_in_the_companion(case):
    """fe_b's low-LDS companion runs two workgroups per CU (a companion has at least two; with three, 2 #CUs + 9 streams would not be a persistent
    launch, which the first case asserts): 4 #CUs + 9 streams are walks of two and three streams on a grid of 2 #CUs"""
    G = 2 * _cus()
    k = _check_banked("fe_b", "waves4", 1, _walk_rows(case, G + 9, G + 14, 1, G), G + 14, low=1)
    assert "LOW=1" in k and "persistent" in k, k
    n = 2 * G + 9
    k = _check_banked("fe_b", "waves4", 1, _walk_rows(case, n, n + 5, 1, G), n + 5, low=1)
    assert "LOW=1" in k and "persistent" in k, k


# ------------------------------------------------------------------ 3. no table, and a table of zeros
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("name,kernel,TM,n", [("fe_b", "wg8", 1, 5), ("fe_b", "waves4", 3, 7), ("fe_t", "wg8", 1, 5)])
def test_no_table_and_a_table_of_zeros_give_the_bits_of_the_ctl_step(name, kernel, TM, n, pinned, dtype):
    eng = _banked(name)
    H, cap = eng.cfg.hop_size, n + 4
    slots = [int(s) for s in np.random.default_rng(n + TM).permutation(cap)[:n]]
    hops = [TM] * n if TM == 1 else [(i % TM) + 1 for i in range(n)]
    gain = torch.tensor([0.0 if i % 2 else 0.1 for i in range(cap)], device=_dev())
    fill = FILL if dtype == torch.float32 else 777
    with _setup([eng], kernel):
        full = _seeded_state(eng, cap)
        x = _audio((n, TM * H), dtype, pinned, gen=torch.Generator().manual_seed(21))
        d = _desc([(slots[i], hops[i], i * TM * H, i * TM * H) for i in range(n)])
        runs = {}
        for what, table in (("ctl", "absent"), ("null", None), ("zeros", torch.zeros(cap, dtype=torch.int32, device=_dev())),
                            ("zeros pinned", torch.zeros(cap, dtype=torch.int32).pin_memory())):
            st, y, lv = full.clone(), _audio((n, TM * H), dtype, pinned, fill=fill), torch.full((cap, 4), SENTINEL, device=_dev())
            kw = {} if what == "ctl" else dict(bank=table)
            _step(eng, pinned)(x.view(-1), st, cap, d, y.view(-1), T_max=TM, min_gain=gain, levels=lv, **kw)
            runs[what] = (y, st, lv, eng.last_step_kernel())
            torch.cuda.synchronize()
    y0, st0, lv0, k0 = runs["ctl"]
    assert "banks" not in k0 and runs["null"][3] == k0, (k0, runs["null"][3])
    for what in ("zeros", "zeros pinned"):
        assert ", banks>" in runs[what][3] and _strip_banks(runs[what][3]) == k0, (what, runs[what][3], k0)
    for what, (y, st, lv, _) in runs.items():
        assert torch.equal(y, y0) and _same(st, st0) and _same(lv, lv0), f"{what}: not the bits of the ctl step"
    assert not _same(st0, full)


# ------------------------------------------------------------------ 4. a bank out of range
@pytest.mark.parametrize("name,kernel,TM", [("fe_b", "wg8", 1), ("fe_b", "waves4", 3), ("fe_t", "wg8", 1), ("fe_m", "wg8", 1)])
def test_a_bank_out_of_range_is_a_stream_without_state(name, kernel, TM):
    eng = _banked(name)
    H, cap, guard = eng.cfg.hop_size, 8, 64
    row = TM * H
    bad = [-1, BANKS, 2 ** 30, -2 ** 31]
    rows = [(1, TM, 0)] + [(2 + i, TM, b) for i, b in enumerate(bad)] + [(7, TM, BANKS - 1)]
    n = len(rows)
    with _setup([eng], kernel):
        full = _seeded_state(eng, cap)
        xbuf = torch.full((guard + n * row + guard,), 0.25, device=_dev())
        ybuf = torch.full((guard + n * row + guard,), FILL, device=_dev())
        x, y = xbuf[guard:guard + n * row], ybuf[guard:guard + n * row]
        x.copy_(0.1 * torch.randn(n * row, generator=torch.Generator().manual_seed(8)))
        st, lv = full.clone(), torch.full((cap, 4), SENTINEL, device=_dev())
        table = torch.zeros(cap, dtype=torch.int32)
        for s, _, b in rows:
            table[s] = b
        eng.step_streams(x, st, cap, _desc([(s, h, i * row, i * row) for i, (s, h, _) in enumerate(rows)]), y, T_max=TM, levels=lv, bank=table.to(_dev()))
        torch.cuda.synchronize()
    y = y.view(n, row)
    vs, v0 = _views(eng, st, cap), _views(eng, full, cap)
    for i in range(1, 1 + len(bad)):
        s = rows[i][0]
        assert float(y[i].abs().max()) == 0.0, f"bank {rows[i][2]}: the output rows are not zero"
        assert all(_same(a[s], r[s]) for a, r in zip(vs, v0)), f"bank {rows[i][2]}: the state of slot {s} changed"
        assert bool((lv[s] == SENTINEL).all()), f"bank {rows[i][2]}: a level row was written"
    for i in (0, n - 1):
        s = rows[i][0]
        assert float(y[i].abs().max()) > 0.0 and not _same(vs[0][s], v0[0][s]) and float(lv[s, 0]) != SENTINEL
    assert bool((ybuf[:guard] == FILL).all()) and bool((ybuf[-guard:] == FILL).all()), "the guard floats around wav_out were written"
    assert bool((xbuf[:guard] == 0.25).all()) and bool((xbuf[-guard:] == 0.25).all())


# ------------------------------------------------------------------ 5. against the oracle
HOPS = 6


@functools.lru_cache(maxsize=None)
def _oracle_outputs(name):
    """six hops of one stream from zero state through the oracle of bank 0's and of bank 1's checkpoint"""
    cfg, sds = _checkpoints(name)
    H = cfg.hop_size
    x = (0.1 * torch.randn(1, HOPS * H, generator=torch.Generator().manual_seed(55))).numpy()
    outs = []
    for k in (0, 1):
        orc = FEOracle(cfg, fold_state_dict(sds[k], cfg), np.float32)
        caches, out = orc.initialize_cache(1), []
        for t in range(HOPS):
            o, *caches = orc.step(x[:, t * H:(t + 1) * H], *caches)
            out.append(o)
        outs.append(np.concatenate(out, axis=1)[0])
    assert rms(outs[0] - outs[1]) > 1e-2 * rms(outs[0]), "the two checkpoints give the same output: the comparison shows nothing"
    return x, outs


@pytest.mark.parametrize("kernel", ["waves4", "wg8"])
@pytest.mark.parametrize("name", ["fe_b", "fe_t"])
def test_streams_on_two_banks_match_the_oracle_of_their_own_checkpoint(name, kernel):
    x, want = _oracle_outputs(name)
    eng = _banked(name)
    H, cap, slots = eng.cfg.hop_size, 4, [2, 1]
    xd = torch.from_numpy(x).to(_dev()).repeat(2, 1).contiguous()                    # both streams hear the same audio
    got = {}
    with _setup([eng], kernel):
        for order in ((0, 1), (1, 0)):
            table = torch.zeros(cap, dtype=torch.int32)
            for s, b in zip(slots, order):
                table[s] = b
            table = table.to(_dev())
            st, y = eng.new_state(cap), torch.zeros(2, HOPS * H, device=_dev())
            for t in range(HOPS):
                d = _desc([(slots[i], 1, i * HOPS * H + t * H, i * HOPS * H + t * H) for i in range(2)])
                eng.step_streams(xd.view(-1), st, cap, d, y.view(-1), T_max=1, bank=table)
            torch.cuda.synchronize()
            got[order] = y.cpu().numpy()
    for i, b in enumerate((0, 1)):
        rel = rms(got[(0, 1)][i].astype(np.float64) - want[b]) / max(rms(want[b]), 1e-3)
        print(f"weight_banks parity {name} {kernel}: stream {i} on bank {b}: relative rms {rel:.3e}")
        assert np.isfinite(got[(0, 1)][i]).all() and rel <= TIGHT, f"stream {i} on bank {b}: relative rms {rel:.3e} > {TIGHT:.1e} against its checkpoint's oracle"
    assert np.array_equal(got[(1, 0)][0], got[(0, 1)][1]) and np.array_equal(got[(1, 0)][1], got[(0, 1)][0]), "the outputs do not swap with the banks"


# ------------------------------------------------------------------ 6. loading a bank in place, 7. a captured graph follows the table
def _capture(eng, fn):
    dev = _dev()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                                           # warm-up: nothing allocates in the capture
            fn(warm=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn(warm=False)
    return graph


@pytest.mark.parametrize("kernel", ["waves4", "wg8"])
def test_loading_a_bank_in_place_leaves_the_other_banks_and_the_allocation(kernel):
    name = "fe_b"
    _, sds = _checkpoints(name)
    refs = _refs(name) + [_ref(name, BANKS)]
    eng = _new_banked(name, 2)                                       # (its own engine: bank 1 is reloaded)
    H, cap, n = eng.cfg.hop_size, 6, 4
    rows = [(4, 0), (1, 1), (3, 0), (0, 1)]                          # (slot, bank)
    table = torch.zeros(cap, dtype=torch.int32)
    for s, b in rows:
        table[s] = b
    table = table.to(_dev())
    d = _desc([(s, 1, i * H, i * H) for i, (s, _) in enumerate(rows)])
    g = torch.Generator().manual_seed(31)
    xs = [_audio((n, H), torch.float32, False, gen=g) for _ in range(4)]
    x, y = torch.zeros(n, H, device=_dev()), torch.zeros(n, H, device=_dev())
    with _setup([eng] + refs, kernel):
        st = _seeded_state(refs[0], cap)
        # the references: bank-0 streams on checkpoint 0 throughout; bank-1 streams on checkpoint 1 for two hops, then on the new one
        want, st_ref = [], st.clone()
        for t in range(4):
            y_t = torch.zeros(n, H, device=_dev())
            for b, ref in ((0, refs[0]), (1, refs[1] if t < 2 else refs[BANKS])):
                d_b = _desc([(s, 1 if bk == b else 0, i * H, i * H) for i, (s, bk) in enumerate(rows)])
                ref.step_streams(xs[t].view(-1), st_ref, cap, d_b, y_t.view(-1), T_max=1)
            torch.cuda.synchronize()
            want.append(y_t)
        graph = _capture(eng, lambda warm: eng.step_streams(x.view(-1), st.clone() if warm else st, cap, d, y.view(-1), T_max=1, bank=table))
        for t in range(4):
            if t == 2:
                eng.load_state_dict(_torch_sd(sds[BANKS]), bank=1)
                assert eng.weight_banks == 2
            x.copy_(xs[t])
            graph.replay()                                           # (the graph holds the banks' address: it must still be the banks')
            torch.cuda.synchronize()
            assert _same(y, want[t]), f"hop {t}: rows differ (bank-0 streams: {_same(y[0::2], want[t][0::2])}, bank-1 streams: {_same(y[1::2], want[t][1::2])})"
        assert _same(st, st_ref)


def test_a_captured_graph_follows_a_rewritten_bank_table():
    name = "fe_b"
    eng = _banked(name)
    H, cap, n = eng.cfg.hop_size, 8, 4
    full = _seeded_state(eng, cap)
    x = _audio((n, H), torch.float32, False, gen=torch.Generator().manual_seed(3))
    d = _desc([(i, 1, i * H, i * H) for i in range(n)])
    table = torch.zeros(cap, dtype=torch.int32, device=_dev())
    lv = torch.full((cap, 4), SENTINEL, device=_dev())
    y, st = torch.zeros(n, H, device=_dev()), full.clone()
    graph = _capture(eng, lambda warm: eng.step_streams(x.view(-1), full.clone() if warm else st, cap, d, y.view(-1), T_max=1, levels=lv, bank=table))
    first = None
    for r, banks in enumerate(([0] * cap, [2, 0, 1, BANKS] + [0] * (cap - n), [1, 1, 1, 1] + [0] * (cap - n))):
        table.copy_(torch.tensor(banks, dtype=torch.int32))
        st.copy_(full)
        lv.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        e_st, e_y, e_lv = full.clone(), torch.zeros_like(y), torch.full((cap, 4), SENTINEL, device=_dev())
        eng.step_streams(x.view(-1), e_st, cap, d, e_y.view(-1), T_max=1, levels=e_lv, bank=torch.tensor(banks, dtype=torch.int32, device=_dev()))
        torch.cuda.synchronize()
        assert _same(y, e_y) and _same(st, e_st) and _same(lv, e_lv), f"replay {r}"
        if r == 0:
            first = y.clone()
        if r == 1:
            assert not _same(y[0], first[0]) and _same(y[1], first[1]) and not _same(y[2], first[2]), "the replay did not follow the new table"
            assert float(y[3].abs().max()) == 0.0 and bool((lv[3] == SENTINEL).all()), "a bank out of range in a replay"


# ------------------------------------------------------------------ 8. poisoned LDS
@pytest.mark.parametrize("name,kernel,TM,n", [("fe_b", "wg8", 1, 7), ("fe_b", "wg8", 1, 300), ("fe_b", "wg8_persist", 1, 300), ("fe_b", "waves4", 2, 7),
                                              ("fe_b", "waves4", 1, 300), ("fe_t", "wg8", 1, 7)])
def test_banked_step_from_poisoned_lds_gives_the_bits_of_the_clean_run(name, kernel, TM, n):
    eng = _banked(name)
    H, cap = eng.cfg.hop_size, n
    with _setup([eng], kernel, low=0 if n > 7 else None):
        full = _seeded_state(eng, cap)
        s = _audio((n, TM * H), torch.int16, False, gen=torch.Generator().manual_seed(14))
        d = _desc([(n - 1 - i, 0 if i % 5 == 2 else TM, i * TM * H, i * TM * H) for i in range(n)])
        table = torch.tensor([(3 * i + i // 4) % BANKS for i in range(cap)], dtype=torch.int32, device=_dev())
        runs = []
        for poison in (False, True):
            st, y, lv = full.clone(), _audio((n, TM * H), torch.int16, False, fill=-999), torch.full((cap, 4), SENTINEL, device=_dev())
            if poison:
                eng.poison_lds()
            eng.step_streams(s.view(-1), st, cap, d, y.view(-1), T_max=TM, levels=lv, bank=table)
            torch.cuda.synchronize()
            runs.append((y, st, lv))
    assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]) and _same(runs[0][2], runs[1][2])
    assert bool(torch.isfinite(runs[1][1]).all())


# ------------------------------------------------------------------ 9. end to end: PacketPool
def test_packet_pool_streams_on_three_banks_equal_each_stream_alone_on_its_checkpoint():
    name = "fe_b"
    eng, refs = _banked(name), _refs(name)
    H = eng.cfg.hop_size
    n_streams, ticks, packet = 12, 24, 320                           # 20 ms at 16 kHz against a hop of 256 samples
    banks = [(5 * i + i // 3) % BANKS for i in range(n_streams)]
    assert set(banks) == set(range(BANKS))
    rng = np.random.default_rng(41)
    arrivals = rng.choice([0, 1, 1, 1, 2, 3], size=(ticks, n_streams))
    total = int(arrivals.sum(0).max()) * packet
    pcm = (0.2 * torch.randn(n_streams, total, generator=torch.Generator().manual_seed(42)) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    movers = [0, 4, 7]                                               # these move to a second pool half way

    def feed(pool, slot, i, t, sent):
        for _ in range(int(arrivals[t, i])):
            pool.push(slot, pcm[i, sent[i]:sent[i] + packet])
            sent[i] += packet

    with _setup([eng] + refs, "waves4"):
        pool, second = PacketPool(eng, 16, ring_hops=16, T_max=3), PacketPool(eng, 4, ring_hops=16, T_max=3)
        second.open()                                                # (the movers land on other slot numbers)
        home = {i: (pool, pool.open(bank=banks[i])) for i in range(n_streams)}
        sent, got = {i: 0 for i in range(n_streams)}, {i: [] for i in range(n_streams)}
        for t in range(ticks):
            if t == ticks // 2:
                for i in movers:
                    new = pool.move(home[i][1], second)
                    assert second.bank(new) == banks[i], "move() lost the stream's bank"
                    home[i] = (second, new)
            for i, (p, slot) in home.items():
                feed(p, slot, i, t, sent)
            if pool.tick():
                assert ", banks>" in eng.last_step_kernel() and "streams, pinned, s16" in eng.last_step_kernel(), eng.last_step_kernel()
            second.tick()
            for i, (p, slot) in home.items():
                got[i].append(p.pull(slot))
        together = {i: torch.cat(v) for i, v in got.items()}
        for i in range(n_streams):
            solo = PacketPool(refs[banks[i]], 1, ring_hops=16, T_max=3)
            slot = solo.open()
            sent1, out = {i: 0}, []
            for t in range(ticks):
                feed(solo, slot, i, t, sent1)
                solo.tick()
                out.append(solo.pull(slot))
            alone = torch.cat(out)
            assert "banks" not in refs[banks[i]].last_step_kernel()
            assert alone.numel() > 10 * H and torch.equal(alone, together[i]), f"stream {i} (bank {banks[i]}) differs from the same stream alone on its checkpoint"


# ------------------------------------------------------------------ 10. the banks of a handle: unloaded banks, growing and shrinking
def test_unloaded_banks_are_refused_and_resizing_keeps_the_banks_that_survive():
    from fastenhancer_amd._lib import FEError
    name = "fe_t"
    _, sds = _checkpoints(name)
    refs = _refs(name)
    eng = Engine(product_config(name), _dev())                       # (a handle that has loaded nothing yet)
    H, cap = eng.cfg.hop_size, 4
    x = _audio((3, H), torch.float32, False, gen=torch.Generator().manual_seed(9))
    d = _desc([(i, 1, i * H, i * H) for i in range(3)])
    full = _seeded_state(refs[0], cap)

    def step(table, st=None, **kw):
        y = torch.full((3, H), FILL, device=_dev())
        eng.step_streams(x.view(-1), full.clone() if st is None else st, cap, d, y.view(-1), T_max=1, bank=torch.tensor(table, dtype=torch.int32, device=_dev()), **kw)
        torch.cuda.synchronize()
        return y

    want = []
    for k in range(BANKS):
        y_k = torch.full((3, H), FILL, device=_dev())
        refs[k].step_streams(x.view(-1), full.clone(), cap, d, y_k.view(-1), T_max=1)
        torch.cuda.synchronize()
        want.append(y_k)
    eng.set_weight_banks(2)
    eng.load_state_dict(_torch_sd(sds[1]), bank=1)                   # (bank 1 before bank 0: the first load makes the allocation)
    with pytest.raises(FEError, match=r"\(-4\).*fe_load_weights has not been called"):
        step([0, 1, 0, 0])
    eng.load_state_dict(_torch_sd(sds[0]))
    assert _same(step([0, 1, 1, 0]), torch.stack([want[0][0], want[1][1], want[1][2]]))
    eng.set_weight_banks(3)                                          # banks 0 and 1 move to the new allocation; bank 2 is empty
    with pytest.raises(FEError, match=r"\(-4\).*bank 2 of the handle's 3"):
        step([0, 1, 1, 0])
    y = torch.full((3, H), FILL, device=_dev())
    eng.step_streams(x.view(-1), full.clone(), cap, d, y.view(-1), T_max=1)      # (every other entry point reads bank 0 and asks for nothing else)
    torch.cuda.synchronize()
    assert _same(y, want[0])
    eng.load_state_dict(_torch_sd(sds[2]), bank=2)
    assert _same(step([2, 1, 0, 0]), torch.stack([want[2][0], want[1][1], want[0][2]]))
    eng.set_weight_banks(2)
    y = step([2, 1, 0, 0])
    assert float(y[0].abs().max()) == 0.0 and _same(y[1:], torch.stack([want[1][1], want[0][2]])), "bank 2 of a two-bank handle is out of range"
    eng.set_weight_banks(1)
    assert _same(step([0, 0, 0, 0]), want[0])
