"""The slot-indexed streaming step on the GPU (fe_step_slots / fe_state_reset_slots through Engine.step_slots / reset_slots and StreamPool).

fe_step_slots must compute, bit for bit, what fe_step computes on a compact state holding only the named slots (the compact copy is
built from split_state views), touch no other byte of the state, and pick the same kernel as fe_step(B = n), in its slotted form."""
import numpy as np
import pytest
import torch

from common import MODEL_KWARGS, hip_model, load_golden, rms
from fastenhancer_amd.engine import _ptr, _stream
from fastenhancer_amd.serving import StreamPool
from oracle.weightgen import make_input

pytestmark = pytest.mark.gpu

MODELS = ["fe_b", "fe_t", "fe_tk_b", "fe_ln_b", "fe_dprnn_b", "fe_dpt_b"]
FAMILY_REL = 2e-5          # tests/test_gpu_parity.py TIGHT_REL["fastenhancer"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        _ENGINES[name] = hip_model(name, device=_dev()).engine
    return _ENGINES[name]


def _views(eng, state, B):
    """per-stream views of every state tensor, stream on dim 0 (split_state's views + the dptransformer ring heads); they cover the buffer"""
    vs = []
    for t in eng.split_state(state, B, head0=True):
        vs.append(t.reshape(B, -1) if t.is_contiguous() else t)
    covered = sum(v.numel() for v in vs)
    if eng.cfg.dpt:
        vs.append(state[covered:covered + B].view(B, 1))          # (the ring heads follow the caches)
        covered += B
    assert covered == state.numel() == eng.state_floats(B), (covered, state.numel())
    for v in vs:
        assert v.shape[0] == B
    return vs


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _seeded_state(eng, cap, hops=3, seed=0):
    """a state of `cap` streams after a few hops of random audio: non-zero everywhere a hop writes (dptransformer heads included)"""
    H = eng.cfg.hop_size
    state = eng.new_state(cap)
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(hops):
        x = (0.1 * torch.randn(cap, H, generator=g)).to(_dev())
        eng.step(x, state, T=1)
    torch.cuda.synchronize()
    return state


def _compact(eng, full, cap, slots_t):
    n = slots_t.numel()
    comp = eng.new_state(n)
    for vc, vf in zip(_views(eng, comp, n), _views(eng, full, cap)):
        vc.copy_(vf[slots_t])
    return comp


def _strip(kernel_name):
    return kernel_name.replace(", slots>", ">").replace("<slots>", "")


def _check_slotted_step(eng, cap, slots, T, calls=2, seed=1):
    """fe_step_slots on a seeded state vs fe_step(n) on its compacted copy: outputs, stepped slots and every other byte, kernel names"""
    dev = _dev()
    H = eng.cfg.hop_size
    n = len(slots)
    full = _seeded_state(eng, cap)
    slots_t = torch.tensor(slots, dtype=torch.long, device=dev)
    slots_d = torch.tensor(slots, dtype=torch.int32, device=dev)
    comp = _compact(eng, full, cap, slots_t)
    others = torch.ones(cap, dtype=torch.bool, device=dev)
    others[slots_t] = False
    before = [v[others].clone() for v in _views(eng, full, cap)]
    g = torch.Generator(device="cpu").manual_seed(seed)
    for c in range(calls):
        x = (0.1 * torch.randn(n, T * H, generator=g)).to(dev)
        ref = eng.step(x, comp, T=T)
        k_ref = eng.last_step_kernel()
        out = eng.step_slots(x, full, cap, slots_d, T=T)
        k = eng.last_step_kernel()
        torch.cuda.synchronize()
        assert "slots" in k and _strip(k) == k_ref, (k, k_ref)
        assert _same(out, ref), f"call {c}: output differs (max {float((out - ref).abs().max()):.3e})"
        for i, (vf, vc) in enumerate(zip(_views(eng, full, cap), _views(eng, comp, n))):
            assert _same(vf[slots_t], vc), f"call {c}: state tensor {i} of the stepped slots differs"
        for i, (vf, b) in enumerate(zip(_views(eng, full, cap), before)):
            assert _same(vf[others], b), f"call {c}: state tensor {i} of a slot not named changed"
    return k


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("name", MODELS)
def test_step_slots_matches_compact_step_and_leaves_other_slots(name, T):
    eng = _engine(name)
    rng = np.random.default_rng(7)
    slots = [int(s) for s in rng.permutation(64)[:23]]
    assert slots != sorted(slots)
    k = _check_slotted_step(eng, 64, slots, T)
    if name == "fe_b" and T == 1:
        assert k.startswith("fe_frame8_kernel<slots>"), k           # the 512-thread per-hop kernel
    if T == 3:
        assert "generic, slots" in k, k


def test_step_slots_above_the_cu_count():
    """600 of 1024 slots: whichever launch fe_step(600) picks above #CUs (low-LDS companion or persistent walk), slotted"""
    eng = _engine("fe_b")
    rng = np.random.default_rng(11)
    slots = [int(s) for s in rng.permutation(1024)[:600]]
    k = _check_slotted_step(eng, 1024, slots, 1, calls=1)
    assert "fe_frame8_kernel<slots>" not in k, k


@pytest.mark.parametrize("name", MODELS)
def test_reset_slots_zeroes_the_named_slots_only(name):
    eng = _engine(name)
    cap = 64
    full = _seeded_state(eng, cap)
    named = [5, 63, 0, 17]
    before = full.clone()
    eng.reset_slots(full, cap, named)
    fresh = torch.full_like(full, 1.0)
    assert eng.lib.fe_state_init(eng._h, _ptr(fresh), cap, _stream(_dev())) == 0
    torch.cuda.synchronize()
    dev = _dev()
    idx = torch.tensor(named, device=dev)
    others = torch.ones(cap, dtype=torch.bool, device=dev)
    others[idx] = False
    for i, (v, vb, vz) in enumerate(zip(_views(eng, full, cap), _views(eng, before, cap), _views(eng, fresh, cap))):
        assert _same(v[idx], vz[idx]), f"state tensor {i}: a reset slot differs from fe_state_init's"
        assert _same(v[others], vb[others]), f"state tensor {i}: a slot not named changed"
        assert float(vb[idx].abs().max()) > 0, f"state tensor {i} was not seeded"
    # a reset slot then steps exactly as a stream started on a fresh state
    H = eng.cfg.hop_size
    x = (0.1 * torch.randn(1, H, generator=torch.Generator().manual_seed(3))).to(dev)
    solo = eng.new_state(1)
    ref = eng.step(x, solo)
    out = eng.step_slots(x, full, cap, [17])
    torch.cuda.synchronize()
    assert _same(out, ref)


@pytest.mark.parametrize("T", [1, 3])
def test_out_of_range_slot_writes_zero_output_and_no_state(T):
    eng = _engine("fe_b")
    dev = _dev()
    cap, H = 32, eng.cfg.hop_size
    full = _seeded_state(eng, cap)
    good, rows = [9, 2, 30], [0, 2, 4]
    slots = [9, cap, 2, -3, 30]                                   # rows 1 and 3: out of range
    comp = _compact(eng, full, cap, torch.tensor(good, device=dev))
    before = full.clone()
    x = (0.1 * torch.randn(5, T * H, generator=torch.Generator().manual_seed(5))).to(dev)
    out = torch.full((5, T * H), 7.0, device=dev)
    eng.step_slots(x, full, cap, torch.tensor(slots, dtype=torch.int32, device=dev), wav_out=out, T=T)
    ref = eng.step(x[rows].contiguous(), comp, T=T)
    torch.cuda.synchronize()
    assert float(out[[1, 3]].abs().max()) == 0.0
    assert _same(out[rows], ref)
    gi = torch.tensor(good, device=dev)
    others = torch.ones(cap, dtype=torch.bool, device=dev)
    others[gi] = False
    for vf, vb, vc in zip(_views(eng, full, cap), _views(eng, before, cap), _views(eng, comp, 3)):
        assert _same(vf[others], vb[others])
        assert _same(vf[gi], vc)


def test_stream_pool_join_leave_schedule_matches_streams_run_alone():
    """40 ticks, 12 streams opening and closing at different ticks: each stream's output is what it gives run alone from a zero state"""
    name = "fe_b"
    eng = _engine(name)
    dev = _dev()
    H = eng.cfg.hop_size
    g = load_golden(name)
    kw, sr, seed = MODEL_KWARGS[name]
    gold_x = make_input(int(g["B"]), int(g["hops"]) * H, seed + 1000, sr)          # the golden's two streams: streams 0 and 1 below
    rng = np.random.default_rng(21)
    spans = [(3, 3 + int(g["hops"])), (10, 10 + int(g["hops"]))]
    while len(spans) < 12:
        a = int(rng.integers(0, 36))
        spans.append((a, int(rng.integers(a + 1, 41))))
    audio = [torch.from_numpy(gold_x[i]) if i < 2 else 0.1 * torch.randn((b - a) * H, generator=torch.Generator().manual_seed(100 + i))
             for i, (a, b) in enumerate(spans)]
    pool = StreamPool(eng, 16)
    slot_of, outs = {}, {i: [] for i in range(len(spans))}
    peak = 0
    kernels = set()
    for tick in range(40):
        for i, (a, b) in enumerate(spans):
            if b == tick:
                pool.close(slot_of.pop(i))
        for i, (a, b) in enumerate(spans):
            if a == tick:
                slot_of[i] = pool.open()
        live = sorted(slot_of, key=lambda i: -slot_of[i])           # (call order differs from slot order)
        peak = max(peak, len(live))
        if not live:
            continue
        x = torch.stack([audio[i][(tick - spans[i][0]) * H:(tick - spans[i][0] + 1) * H] for i in live]).to(dev)
        y = pool.step([slot_of[i] for i in live], x)
        kernels.add(_strip(eng.last_step_kernel()))
        for r, i in enumerate(live):
            outs[i].append(y[r].cpu())
    assert 1 < peak <= 16, peak
    for i, (a, b) in enumerate(spans):
        solo = eng.new_state(1)
        ref = torch.cat([eng.step(audio[i][t * H:(t + 1) * H].reshape(1, H).to(dev), solo)[0].cpu() for t in range(b - a)])
        assert {_strip(eng.last_step_kernel())} == kernels, (eng.last_step_kernel(), kernels)
        got = torch.cat(outs[i])
        assert _same(got, ref), f"stream {i} (ticks {a}..{b}): max diff {float((got - ref).abs().max()):.3e}"
    got = torch.stack([torch.stack(outs[i]) for i in (0, 1)], 1).numpy()         # [hops, 2, H], the golden's layout
    ref = g["stream_wav_out"]
    assert rms(got - ref) <= FAMILY_REL * max(rms(ref), 1e-3), rms(got - ref)


def test_step_slots_in_a_captured_graph_follows_the_slot_tensor():
    eng = _engine("fe_b")
    dev = _dev()
    cap, n, H = 64, 12, eng.cfg.hop_size
    full = _seeded_state(eng, cap)
    twin = full.clone()
    slots_d = torch.arange(n, dtype=torch.int32, device=dev)
    x = torch.zeros(n, H, device=dev)
    y = torch.zeros(n, H, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):                                           # warm-up: attributes, scratch - nothing allocates in the capture
            eng.step_slots(x, twin.clone(), cap, slots_d, wav_out=y)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step_slots(x, full, cap, slots_d, wav_out=y)
    rng = np.random.default_rng(9)
    gen = torch.Generator().manual_seed(8)
    for r in range(3):
        sl = [int(v) for v in rng.permutation(cap)[:n]]
        slots_d.copy_(torch.tensor(sl, dtype=torch.int32))
        x.copy_(0.1 * torch.randn(n, H, generator=gen))
        graph.replay()
        ref = eng.step_slots(x, twin, cap, sl)
        torch.cuda.synchronize()
        assert _same(y, ref), f"replay {r}"
        assert _same(full, twin), f"replay {r}: state"
