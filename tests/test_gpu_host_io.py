"""The pinned streaming steps on the GPU (fe_step_pinned / fe_step_slots_pinned through Engine.step_pinned / step_slots_pinned and
StreamPool.step_host): the kernel reads each hop from page-locked host memory and writes the enhanced hop back there.

Each must compute, bit for bit, what fe_step / fe_step_slots compute on device copies of the same rows, touch no state slot it is not
given, and pick the same kernel, in its pinned form.  Every host buffer handed to a step here is pinned: the refusal of pageable memory
is tested host-side only (tests/test_cpu_host_io.py)."""
import numpy as np
import pytest
import torch

from common import MODEL_KWARGS, load_golden, rms
from fastenhancer_amd.serving import StreamPool
from oracle.weightgen import make_input
from test_gpu_stream_slots import FAMILY_REL, MODELS, _compact, _dev, _engine, _same, _seeded_state, _views

pytestmark = pytest.mark.gpu


def _unpin_name(k):
    return k.replace(", pinned>", ">")


def _host_rows(rows, cols, layout, seed=None, fill=None):
    """a pinned [rows, cols] view with the row layout named: "compact" (stride cols), "wide" (stride cols + 40, 16-byte aligned rows),
    "odd" (stride cols + 3, starting one float into its buffer: rows not 16-byte aligned)"""
    pad, off = {"compact": (0, 0), "wide": (40, 8), "odd": (3, 1)}[layout]
    buf = torch.zeros(rows * (cols + pad) + off + pad).pin_memory()
    if fill is not None:
        buf.fill_(fill)
    view = buf[off:off + rows * (cols + pad)].view(rows, cols + pad)[:, :cols]
    assert view.is_pinned() and view.stride() == (cols + pad, 1)
    if seed is not None:
        view.copy_(0.1 * torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed)))
    return view


@pytest.mark.parametrize("layout", ["compact", "wide", "odd"])
@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("name", MODELS)
def test_step_slots_pinned_matches_device_step_slots(name, T, layout):
    """23 of 64 slots over 12 hops: outputs and the whole state as fe_step_slots on device copies leaves them; slots not named untouched"""
    eng = _engine(name)
    dev = _dev()
    H = eng.cfg.hop_size
    cap = 64
    slots = [int(s) for s in np.random.default_rng(7).permutation(cap)[:23]]
    n = len(slots)
    full = _seeded_state(eng, cap)
    twin = full.clone()
    slots_d = torch.tensor(slots, dtype=torch.int32, device=dev)
    others = torch.ones(cap, dtype=torch.bool, device=dev)
    others[slots_d.long()] = False
    before = [v[others].clone() for v in _views(eng, full, cap)]
    x = _host_rows(n, T * H, layout)
    y = _host_rows(n, T * H, layout, fill=7.0)
    for c in range(12 // T):
        x.copy_(0.1 * torch.randn(n, T * H, generator=torch.Generator().manual_seed(100 + c)))
        ref = eng.step_slots(x.to(dev), twin, cap, slots_d, T=T)
        k_ref = eng.last_step_kernel()
        out = eng.step_slots_pinned(x, full, cap, slots_d, wav_out=y, T=T)
        k = eng.last_step_kernel()
        torch.cuda.synchronize()
        assert out is y
        assert "pinned" in k and _unpin_name(k) == k_ref, (k, k_ref)
        assert _same(y, ref.cpu()), f"call {c}: output differs (max {float((y - ref.cpu()).abs().max()):.3e})"
        assert _same(full, twin), f"call {c}: state differs from fe_step_slots'"
    for i, (vf, b) in enumerate(zip(_views(eng, full, cap), before)):
        assert _same(vf[others], b), f"state tensor {i} of a slot not named changed"
    if name == "fe_b" and T == 1:
        assert k.startswith("fe_frame8_kernel<slots, pinned>"), k
    if T == 4:
        assert "generic, slots, pinned" in k, k


@pytest.mark.parametrize("name,B", [(m, b) for m in MODELS for b in (1, 256)] + [("fe_b", 600), ("fe_t", 600)])
def test_step_pinned_matches_fe_step(name, B):
    """a compact batch over 12 hops: at 256 streams the 512-thread kernel for fe_b; at 600 the companion / persistent walk"""
    eng = _engine(name)
    dev = _dev()
    H = eng.cfg.hop_size
    state = _seeded_state(eng, B)
    twin = state.clone()
    y = torch.empty(B, H).pin_memory()
    for c in range(12):
        x = (0.1 * torch.randn(B, H, generator=torch.Generator().manual_seed(200 + c))).pin_memory()
        ref = eng.step(x.to(dev), twin)
        k_ref = eng.last_step_kernel()
        out = eng.step_pinned(x, state, wav_out=y)
        k = eng.last_step_kernel()
        torch.cuda.synchronize()
        assert _same(out, ref.cpu()), f"hop {c}: output differs (max {float((out - ref.cpu()).abs().max()):.3e})"
        assert _same(state, twin), f"hop {c}: state differs"
        assert "pinned" in k and _unpin_name(k).replace(", slots>", ">").replace("<slots>", "") == k_ref, (k, k_ref)
    if name == "fe_b" and B == 256:
        assert k.startswith("fe_frame8_kernel<slots, pinned>"), k
    if B == 600:
        assert "fe_frame8_kernel" not in k, k


@pytest.mark.parametrize("T", [1, 4])
def test_step_pinned_chunks_and_allocates_its_output(T):
    """T = 4 hops per call, wav_out allocated pinned by the engine, rows wider than T*H"""
    eng = _engine("fe_b")
    dev = _dev()
    B, H = 40, eng.cfg.hop_size
    state = _seeded_state(eng, B)
    twin = state.clone()
    for c in range(12 // T):
        x = _host_rows(B, T * H, "wide", seed=300 + c)
        ref = eng.step(x.to(dev), twin, T=T)
        out = eng.step_pinned(x, state, T=T)
        torch.cuda.synchronize()
        assert out.is_pinned() and out.shape == (B, T * H)
        assert _same(out, ref.cpu()), f"call {c}"
        assert _same(state, twin), f"call {c}: state"


@pytest.mark.parametrize("T", [1, 4])
def test_out_of_range_slot_writes_zero_host_rows_and_no_state(T):
    eng = _engine("fe_b")
    dev = _dev()
    cap, H = 32, eng.cfg.hop_size
    full = _seeded_state(eng, cap)
    good, rows = [9, 2, 30], [0, 2, 4]
    comp = _compact(eng, full, cap, torch.tensor(good, device=dev))
    before = full.clone()
    x = _host_rows(5, T * H, "compact", seed=5)
    y = _host_rows(5, T * H, "compact", fill=7.0)
    eng.step_slots_pinned(x, full, cap, torch.tensor([9, cap, 2, -3, 30], dtype=torch.int32, device=dev), wav_out=y, T=T)
    ref = eng.step(x[rows].to(dev), comp, T=T)
    torch.cuda.synchronize()
    assert float(y[[1, 3]].abs().max()) == 0.0
    assert _same(y[rows], ref.cpu())
    gi = torch.tensor(good, device=dev)
    others = torch.ones(cap, dtype=torch.bool, device=dev)
    others[gi] = False
    for vf, vb, vc in zip(_views(eng, full, cap), _views(eng, before, cap), _views(eng, comp, 3)):
        assert _same(vf[others], vb[others])
        assert _same(vf[gi], vc)


def test_stream_pool_step_host_golden_parity():
    """the golden's two streams and two others through StreamPool.step_host: bit for bit StreamPool.step, and the golden's stream_wav_out"""
    name = "fe_b"
    eng = _engine(name)
    dev = _dev()
    H = eng.cfg.hop_size
    g = load_golden(name)
    kw, sr, seed = MODEL_KWARGS[name]
    hops, nb = int(g["hops"]), int(g["B"])
    gold_x = torch.from_numpy(make_input(nb, hops * H, seed + 1000, sr))
    extra = 0.1 * torch.randn(2, hops * H, generator=torch.Generator().manual_seed(31))
    audio = torch.cat([gold_x, extra])
    host, ref_pool = StreamPool(eng, 8), StreamPool(eng, 8)
    for p in (host, ref_pool):
        for _ in range(6):
            p.open()
        p.close(1)
        p.close(4)
    slots = [5, 0, 3, 2][:nb + 2]                    # open slots, in an order that is not the slot order
    assert set(slots) <= set(host.active)
    x = torch.empty(len(slots), H).pin_memory()
    outs = []
    for t in range(hops):
        x.copy_(audio[:, t * H:(t + 1) * H])
        y = host.step_host(slots, x)
        assert "pinned" in eng.last_step_kernel(), eng.last_step_kernel()
        ref = ref_pool.step(slots, x.to(dev))
        torch.cuda.synchronize()
        assert _same(y, ref.cpu()), f"hop {t}"
        outs.append(y.clone())
    assert _same(host.state, ref_pool.state)
    got = torch.stack([o[:2] for o in outs]).numpy()            # [hops, 2, H], the golden's layout
    want = g["stream_wav_out"]
    assert rms(got - want) <= FAMILY_REL * max(rms(want), 1e-3), rms(got - want)


def test_step_slots_pinned_in_a_captured_graph_follows_host_audio_and_slots():
    """one capture, three replays with new host audio and new slot contents: each matches an eager call"""
    eng = _engine("fe_b")
    dev = _dev()
    cap, n, H = 64, 12, eng.cfg.hop_size
    full = _seeded_state(eng, cap)
    twin = full.clone()
    slots_d = torch.arange(n, dtype=torch.int32, device=dev)
    x = torch.zeros(n, H).pin_memory()
    y = torch.zeros(n, H).pin_memory()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):                                           # warm-up: attributes, scratch - nothing allocates in the capture
            eng.step_slots_pinned(x, twin.clone(), cap, slots_d, wav_out=y)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step_slots_pinned(x, full, cap, slots_d, wav_out=y)
    assert eng.last_step_kernel().startswith("fe_frame8_kernel<slots, pinned>"), eng.last_step_kernel()
    rng = np.random.default_rng(9)
    gen = torch.Generator().manual_seed(8)
    for r in range(3):
        sl = [int(v) for v in rng.permutation(cap)[:n]]
        slots_d.copy_(torch.tensor(sl, dtype=torch.int32))
        x.copy_(0.1 * torch.randn(n, H, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        ref = eng.step_slots_pinned(x, twin, cap, sl)
        torch.cuda.synchronize()
        assert _same(y, ref), f"replay {r}"
        assert _same(full, twin), f"replay {r}: state"
