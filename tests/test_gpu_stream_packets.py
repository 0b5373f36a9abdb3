"""The packet-audio streaming step on the GPU (fe_step_streams / fe_step_streams_pinned through Engine.step_streams* and PacketPool).

Every stream of a call advances its own number of hops at its own offsets, in float32 or int16 PCM.  The step must give, bit for bit, what
fe_step_slots gives each stream for its hop count under the same kernel, touch nothing else - no state of a stream without a hop, no
sample outside the ranges its descriptors name - and survive descriptors that point outside the buffers."""
import contextlib

import numpy as np
import pytest
import torch

from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool
from test_gpu_stream_slots import _dev, _engine, _same, _seeded_state, _views

pytestmark = pytest.mark.gpu

SHAPES = ["fe_b", "fe_t", "fe48_b_h480", "fe_tk_b", "fe_dpt_b"]


@contextlib.contextmanager
def _kernel(eng, which):
    """the engines are shared between test modules: the step kernel is put back to the default afterwards"""
    eng.set_step_kernel(which)
    try:
        yield
    finally:
        eng.set_step_kernel("wg8")


def _desc(rows):
    return Engine.pack_stream_desc(rows).to(_dev())


def _audio(shape, dtype, pinned, fill=None, gen=None, scale=0.1):
    """a buffer on the device or in page-locked host memory: random audio (gen) or a fill value"""
    if gen is not None:
        x = scale * torch.randn(*shape, generator=gen)
        x = (x * 32768).round().clamp(-32768, 32767).to(torch.int16) if dtype == torch.int16 else x
    else:
        x = torch.full(shape, fill, dtype=dtype)
    return x.pin_memory() if pinned else x.to(_dev())


def _step(eng, pinned):
    return eng.step_streams_pinned if pinned else eng.step_streams


def _strip(k):
    for tag in (", s16", ", pinned", ", streams", ", slots"):
        k = k.replace(tag + ">", ">")
    return k.replace("<streams>", "").replace("<slots>", "").replace("<streams, s16>", "")


# ------------------------------------------------------------------ 1. ragged hop counts = the dense step of each count
@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("name", SHAPES)
def test_ragged_hop_counts_equal_the_dense_step_of_each_count(name, pinned):
    eng = _engine(name)
    dev, H, cap, n, TM = _dev(), eng.cfg.hop_size, 64, 37, 3
    rng = np.random.default_rng(3)
    slots = [int(s) for s in rng.permutation(cap)[:n]]
    hops = [int(h) for h in rng.permutation(([0, 1, 2, 3] * 10)[:n])]
    assert set(hops) == {0, 1, 2, 3} and slots != sorted(slots)
    with _kernel(eng, "waves4"):
        full = _seeded_state(eng, cap)
        x = _audio((n, TM * H), torch.float32, pinned, gen=torch.Generator().manual_seed(4))
        slots_d = torch.tensor(slots, dtype=torch.int32, device=dev)
        dense = {}
        for k in (1, 2, 3):
            st = full.clone()
            xk = x[:, :k * H].contiguous()
            if pinned:
                out = eng.step_slots_pinned(xk.pin_memory(), st, cap, slots_d, T=k)
            else:
                out = eng.step_slots(xk, st, cap, slots_d, T=k)
            torch.cuda.synchronize()
            dense[k] = (out.clone(), st)
        st = full.clone()
        y = _audio((n, TM * H), torch.float32, pinned, fill=7.0)
        d = _desc([(slots[i], hops[i], i * TM * H, i * TM * H) for i in range(n)])
        _step(eng, pinned)(x.view(-1), st, cap, d, y.view(-1), T_max=TM)
        k_name = eng.last_step_kernel()
        torch.cuda.synchronize()
    assert "generic, streams" + (", pinned>" if pinned else ">") in k_name, k_name
    vs, v0 = _views(eng, st, cap), _views(eng, full, cap)
    for i in range(n):
        h, s = hops[i], slots[i]
        if h < TM:
            assert float((y[i, h * H:] - 7.0).abs().max()) == 0.0, f"stream {i}: rows past its {h} hops were written"
        if h == 0:
            for j, (a, b) in enumerate(zip(vs, v0)):
                assert _same(a[s], b[s]), f"stream {i} (0 hops): state tensor {j} changed"
            continue
        ref_out, ref_st = dense[h]
        assert _same(y[i, :h * H], ref_out[i]), f"stream {i} ({h} hops): output differs from fe_step_slots(T = {h})"
        for j, (a, b) in enumerate(zip(vs, _views(eng, ref_st, cap))):
            assert _same(a[s], b[s]), f"stream {i} ({h} hops): state tensor {j} differs from fe_step_slots(T = {h})"
    others = torch.ones(cap, dtype=torch.bool, device=dev)
    others[torch.tensor(slots, device=dev)] = False
    for j, (a, b) in enumerate(zip(vs, v0)):
        assert _same(a[others], b[others]), f"state tensor {j} of a slot not named changed"


# ------------------------------------------------------------------ 2. the default kernels at T_max = 1
@pytest.mark.parametrize("n", [1, 5, 256, 300])
@pytest.mark.parametrize("name", SHAPES)
def test_default_kernels_with_zero_and_one_hop(name, n):
    eng = _engine(name)
    dev, H = _dev(), eng.cfg.hop_size
    cap = n + 20
    rng = np.random.default_rng(n)
    slots = [int(s) for s in rng.permutation(cap)[:n]]
    hops = [1] if n == 1 else [0 if i % 3 == 1 else 1 for i in range(n)]
    full = _seeded_state(eng, cap)
    x = _audio((n, H), torch.float32, False, gen=torch.Generator().manual_seed(n + 1))
    ref_st = full.clone()
    ref = eng.step_slots(x, ref_st, cap, torch.tensor(slots, dtype=torch.int32, device=dev))       # the same n streams in the same call order
    k_ref = eng.last_step_kernel()
    st = full.clone()
    y = _audio((n, H), torch.float32, False, fill=7.0)
    eng.step_streams(x.view(-1), st, cap, _desc([(slots[i], hops[i], i * H, i * H) for i in range(n)]), y.view(-1), T_max=1)
    k = eng.last_step_kernel()
    torch.cuda.synchronize()
    assert "streams" in k and _strip(k) == _strip(k_ref), (k, k_ref)
    if name == "fe_b" and n <= 256:
        assert k.startswith("fe_frame8_kernel<streams>"), k                 # the 512-thread per-hop kernel
    has = torch.tensor(hops, dtype=torch.bool, device=dev)
    sl = torch.tensor(slots, device=dev)
    assert _same(y[has], ref[has]), "a stream with a hop differs from fe_step_slots"
    if not bool(has.all()):
        assert float((y[~has] - 7.0).abs().max()) == 0.0, "a stream without a hop was written"
    for j, (a, b, c) in enumerate(zip(_views(eng, st, cap), _views(eng, ref_st, cap), _views(eng, full, cap))):
        assert _same(a[sl[has]], b[sl[has]]), f"state tensor {j} of the stepped streams differs"
        keep = torch.ones(cap, dtype=torch.bool, device=dev)
        keep[sl[has]] = False
        assert _same(a[keep], c[keep]), f"state tensor {j} of a stream without a hop (or a slot not named) changed"


# ------------------------------------------------------------------ 3. offsets
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("name,TM", [("fe_b", 1), ("fe_t", 1), ("fe48_b_h480", 1), ("fe_b", 2)])
def test_unaligned_scattered_offsets_give_the_bits_of_the_dense_layout(name, TM, dtype):
    eng = _engine(name)
    H, cap, n = eng.cfg.hop_size, 16, 6
    row = TM * H
    slots = [9, 2, 14, 0, 5, 11]
    in_off = [100001, 7, 50003, 20481, 3333, 70001]           # odd element offsets, not monotonic, far apart
    out_off = [60001, 90003, 13, 30001, 45001, 5001]
    total = 120000
    fill = 123.25 if dtype == torch.float32 else 12345
    full = _seeded_state(eng, cap)
    x = _audio((n, row), dtype, False, gen=torch.Generator().manual_seed(12))
    big_in = _audio((total,), dtype, False, fill=fill)
    for i in range(n):
        big_in[in_off[i]:in_off[i] + row] = x[i]
    big_in0 = big_in.clone()
    big_out = _audio((total,), dtype, False, fill=fill)
    ref_st, st = full.clone(), full.clone()
    ref = _audio((n, row), dtype, False, fill=fill)
    eng.step_streams(x.view(-1), ref_st, cap, _desc([(slots[i], TM, i * row, i * row) for i in range(n)]), ref.view(-1), T_max=TM)
    k_ref = eng.last_step_kernel()
    eng.step_streams(big_in, st, cap, _desc([(slots[i], TM, in_off[i], out_off[i]) for i in range(n)]), big_out, T_max=TM)
    assert eng.last_step_kernel() == k_ref
    torch.cuda.synchronize()
    want = _audio((total,), dtype, False, fill=fill)
    for i in range(n):
        want[out_off[i]:out_off[i] + row] = ref[i]
    assert torch.equal(big_out.view(torch.int16), want.view(torch.int16)), "output rows or the guard regions around them differ"
    assert torch.equal(big_in.view(torch.int16), big_in0.view(torch.int16)), "the input buffer was written"
    assert _same(st, ref_st)
    assert float(ref.float().abs().max()) > 0


# ------------------------------------------------------------------ 4. int16 PCM
def _quantise(y):
    q = torch.nan_to_num((y.double() * 32768.0).round(), nan=0.0, posinf=32767.0, neginf=-32768.0).clamp(-32768, 32767)
    return torch.where(torch.isnan(y), torch.zeros_like(q), q).to(torch.int16)


@pytest.mark.parametrize("pinned", [False, True], ids=["device", "pinned"])
@pytest.mark.parametrize("name,TM,kernel", [("fe_b", 1, "wg8"), ("fe_b", 3, "waves4"), ("fe_t", 1, "wg8"), ("fe48_b_h480", 2, "waves4"), ("fe_dpt_b", 1, "wg8")])
def test_int16_pcm_is_the_float_step_on_s_over_32768_quantised_on_the_way_out(name, TM, kernel, pinned):
    """the overlap-add tails of four streams are set far beyond full scale (both signs) and one holds a NaN: both clamps and NaN -> 0 are hit"""
    eng = _engine(name)
    dev, H, cap, n = _dev(), eng.cfg.hop_size, 24, 12
    L = eng.cfg.cache_len
    slots = [int(s) for s in np.random.default_rng(5).permutation(cap)[:n]]
    hops = [TM if i % 4 else max(TM - 1, 1) for i in range(n)]
    with _kernel(eng, kernel):
        full = _seeded_state(eng, cap)
        tails = _views(eng, full, cap)[1]                       # cache_istft [cap, N - H]: added to the next output hop
        assert tuple(tails.shape) == (cap, L)
        tails[slots[0]] += 5.0
        tails[slots[1]] -= 5.0
        tails[slots[2], ::2] = 3.0
        tails[slots[2], 1::2] = -3.0
        tails[slots[3], 17] = float("nan")
        s = _audio((n, TM * H), torch.int16, pinned, gen=torch.Generator().manual_seed(6), scale=0.25)
        s.view(-1)[:8] = torch.tensor([32767, -32768, 0, 1, -1, 16384, -16384, 12345], dtype=torch.int16)
        xf = _audio((n, TM * H), torch.float32, pinned, fill=0.0)
        xf.copy_(s.float() / 32768.0)
        d = _desc([(slots[i], hops[i], i * TM * H, i * TM * H) for i in range(n)])
        st_f, st_s = full.clone(), full.clone()
        yf = _audio((n, TM * H), torch.float32, pinned, fill=0.0)
        ys = _audio((n, TM * H), torch.int16, pinned, fill=-999)
        _step(eng, pinned)(xf.view(-1), st_f, cap, d, yf.view(-1), T_max=TM)
        k_f = eng.last_step_kernel()
        _step(eng, pinned)(s.view(-1), st_s, cap, d, ys.view(-1), T_max=TM)
        k_s = eng.last_step_kernel()
        torch.cuda.synchronize()
    assert ", s16>" in k_s and k_s.replace(", s16>", ">") == k_f, (k_s, k_f)
    assert torch.equal(st_f.view(torch.int32), st_s.view(torch.int32)), "the state after the int16 call is not the float call's"
    want = torch.full_like(ys, -999)
    for i in range(n):
        want[i, :hops[i] * H] = _quantise(yf[i, :hops[i] * H])
    bad = (want != ys).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} samples differ, first at {bad[0].tolist()}: {int(ys[tuple(bad[0])])} vs {int(want[tuple(bad[0])])}"
    assert bool((want == 32767).any()) and bool((want == -32768).any()), "the clamps were not reached"
    assert bool(torch.isnan(yf).any()), "the NaN did not reach the output"
    used = torch.cat([want[i, :hops[i] * H] for i in range(4, n)]).float()
    assert float(used.abs().mean()) > 10, "the ordinary streams should not be silent"


# ------------------------------------------------------------------ 5. descriptors that point outside
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("name,TM", [("fe_b", 1), ("fe_b", 3), ("fe_t", 1)])
def test_bad_descriptors_touch_nothing_outside_the_buffers(name, TM, dtype):
    eng = _engine(name)
    H, cap, G = eng.cfg.hop_size, 16, 4096
    row = TM * H
    count = 12 * row
    fill = 123.25 if dtype == torch.float32 else 12345
    full = _seeded_state(eng, cap)
    alloc_in = _audio((count + 2 * G,), dtype, False, gen=torch.Generator().manual_seed(2))
    alloc_out = _audio((count + 2 * G,), dtype, False, fill=fill)
    win, wout = alloc_in[G:G + count], alloc_out[G:G + count]          # guard regions before and after both buffers
    in0 = alloc_in.clone()
    rows = [
        (3, TM, 0, 0),                                  # 0: good
        (4, 1, count + 5, 1 * row),                     # 1: input past the end
        (5, 1, 1 * row, count),                         # 2: output past the end
        (6, 1, -7, 2 * row),                            # 3: negative input offset
        (7, 1, 2 * row, -1),                            # 4: negative output offset
        (8, -3, 3 * row, 3 * row),                      # 5: negative hop count: none
        (9, TM + 5, 4 * row, 4 * row),                  # 6: too many hops: T_max of them
        (cap + 2, 1, 5 * row, 5 * row),                 # 7: slot out of range: one zero row
        (-1, TM, 6 * row, 6 * row),                     # 8: slot out of range: T_max zero rows
        (10, TM, count - row + 1, 7 * row),             # 9: input range straddles the end
        (11, TM, 8 * row, count - row + 1),             # 10: output range straddles the end
        (12, 1, 2 ** 62, 9 * row),                      # 11: an offset that would overflow
        (13, 1, 9 * row, -2 ** 63),                     # 12
        (14, TM, count - row, count - row),             # 13: good: the last rows of both buffers
    ]
    st = full.clone()
    eng.step_streams(win, st, cap, _desc(rows), wout, T_max=TM)
    k = eng.last_step_kernel()
    ref_st = full.clone()
    ref_alloc = _audio((count + 2 * G,), dtype, False, fill=fill)
    good = [(3, TM, 0, 0), (9, TM, 4 * row, 4 * row), (14, TM, count - row, count - row)]
    eng.step_streams(win, ref_st, cap, _desc(good), ref_alloc[G:G + count], T_max=TM)
    assert eng.last_step_kernel() == k
    torch.cuda.synchronize()
    ref_alloc[G + 5 * row:G + 5 * row + H] = 0
    ref_alloc[G + 6 * row:G + 7 * row] = 0
    assert torch.equal(alloc_out.view(torch.int16), ref_alloc.view(torch.int16)), "output: a row, a skipped stream's place or a guard region differs"
    assert torch.equal(alloc_in.view(torch.int16), in0.view(torch.int16))
    assert _same(st, ref_st), "a skipped stream or an out-of-range slot touched the state"
    assert not _same(st, full)


# ------------------------------------------------------------------ 6. graph capture
def test_streams_pinned_in_a_captured_graph_follows_descriptors_and_rings():
    eng = _engine("fe_b")
    dev = _dev()
    cap, n, H, R = 64, 12, eng.cfg.hop_size, 4 * eng.cfg.hop_size
    full = _seeded_state(eng, cap)
    twin = full.clone()
    ring_in = _audio((cap, R), torch.int16, True, fill=0)
    ring_out = _audio((cap, R), torch.int16, True, fill=0)
    e_in, e_out = _audio((cap, R), torch.int16, True, fill=0), _audio((cap, R), torch.int16, True, fill=0)
    d = _desc([(i, 1, i * R, i * R) for i in range(n)])
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):                                           # warm-up: attributes, scratch - nothing allocates in the capture
            eng.step_streams_pinned(ring_in, twin.clone(), cap, d, ring_out, T_max=1)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step_streams_pinned(ring_in, full, cap, d, ring_out, T_max=1)
    rng = np.random.default_rng(9)
    gen = torch.Generator().manual_seed(8)
    for r in range(3):
        sl = [int(v) for v in rng.permutation(cap)[:n]]
        rows = [(sl[i], int(rng.integers(0, 2)) if i else 1, sl[i] * R + int(rng.integers(0, 4)) * H, sl[i] * R + int(rng.integers(0, 4)) * H) for i in range(n)]
        d.copy_(Engine.pack_stream_desc(rows))
        ring_in.copy_((0.1 * torch.randn(cap, R, generator=gen) * 32768).round().to(torch.int16))
        ring_out.fill_(r)
        e_in.copy_(ring_in)
        e_out.fill_(r)
        graph.replay()
        eng.step_streams_pinned(e_in, twin, cap, rows, e_out, T_max=1)
        torch.cuda.synchronize()
        assert torch.equal(ring_out, e_out), f"replay {r}"
        assert _same(full, twin), f"replay {r}: state"
        assert int((ring_out != r).sum()) > 0


# ------------------------------------------------------------------ 7. end to end: PacketPool
def test_packet_pool_with_jittered_20ms_packets_equals_each_stream_run_alone():
    eng = _engine("fe_b")
    dev, H = _dev(), eng.cfg.hop_size
    n_streams, ticks, packet = 8, 200, 320                           # 20 ms at 16 kHz against a hop of 256 samples
    rng = np.random.default_rng(31)
    arrivals = rng.choice([0, 1, 1, 1, 2, 3], size=(ticks, n_streams))   # packets per stream and tick: none, one, or a burst
    gen = torch.Generator().manual_seed(32)
    total = int(arrivals.sum(0).max()) * packet
    pcm = (0.2 * torch.randn(n_streams, total, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    with _kernel(eng, "waves4"):
        pool = PacketPool(eng, 12, ring_hops=16, T_max=3)
        slots = [pool.open() for _ in range(n_streams)]
        sent = [0] * n_streams
        got = [[] for _ in range(n_streams)]
        hop_counts = set()
        for t in range(ticks):
            for i in rng.permutation(n_streams):
                for _ in range(int(arrivals[t, i])):
                    pool.push(slots[i], pcm[i, sent[i]:sent[i] + packet])
                    sent[i] += packet
            launched = pool.tick()
            for _, h, _, _ in launched:
                hop_counts.add(h)
            if launched:
                assert "generic, streams, pinned, s16>" in eng.last_step_kernel()
            for i in range(n_streams):
                got[i].append(pool.pull(slots[i]))
        assert hop_counts == {1, 2, 3}
        for i in range(n_streams):
            y = torch.cat(got[i])
            hops = y.numel() // H
            assert y.numel() % H == 0 and sent[i] - 16 * H <= y.numel() <= sent[i] and hops > 150
            solo = eng.new_state(1)
            x = (pcm[i, :hops * H].float() / 32768.0).to(dev)
            ref = torch.cat([eng.step(x[k * H:(k + 1) * H].reshape(1, H), solo)[0] for k in range(hops)])
            want = _quantise(ref).cpu()
            bad = (want != y).nonzero()
            assert bad.numel() == 0, f"stream {i}: {bad.shape[0]} of {y.numel()} samples differ, first at {int(bad[0])}"


# ------------------------------------------------------------------ 8. LDS poison
def test_streams_step_from_poisoned_lds_gives_the_bits_of_the_plain_run():
    eng = _engine("fe_b")
    H, cap, n = eng.cfg.hop_size, 256, 256
    full = _seeded_state(eng, cap)
    s = _audio((n, H), torch.int16, False, gen=torch.Generator().manual_seed(14))
    d = _desc([(n - 1 - i, 0 if i % 5 == 2 else 1, i * H, i * H) for i in range(n)])
    runs = []
    for poison in (False, True):
        st = full.clone()
        y = _audio((n, H), torch.int16, False, fill=-999)
        if poison:
            eng.poison_lds()
        eng.step_streams(s.view(-1), st, cap, d, y.view(-1), T_max=1)
        torch.cuda.synchronize()
        runs.append((y, st))
    assert eng.last_step_kernel().startswith("fe_frame8_kernel<streams, s16>")
    assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    assert int((runs[0][0] == -999).sum()) >= H * (n // 5)
