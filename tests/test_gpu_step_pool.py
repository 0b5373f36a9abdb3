"""fe_step_pool on the GPU: the slot-indexed streaming step of BSRNN, FSPEN and LiSenNet (Engine.step_pool, StreamPool.step).

Stream i of a call is state slot slots[i] of a state sized for `capacity` streams.  Each named stream's output rows and state must be, bit for
bit, those of fe_step(B = n, T) under the same per-stream kernel on a dense state holding the named slots' records; no other byte of the state
may change; a slot out of range writes zero rows and touches nothing; the stream-batched kernels are never taken.  Models: bsrnn_xxt (16
channels: the role-split PART 1 and, under FE_STEP_KERNEL_WAVES4, the phase-by-phase one), bsrnn_s (64 channels: projections in global
scratch), fspen, lisennet.  States are seeded non-zero by four fe_step hops (the helpers of test_gpu_step_chunk.py)."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from common import hip_engine
from fastenhancer_amd import _lib
from fastenhancer_amd.serving import StreamPool
from oracle.weightgen import make_input
from test_gpu_parity import TIGHT_REL, _assert_close
from test_gpu_step_chunk import _cached, _dev, _engine, _same, _seeded_state

pytestmark = pytest.mark.gpu

MODELS = ["bsrnn_xxt", "bsrnn_s", "fspen", "lisennet"]
SB_OPTION = {"bsrnn_xxt": "bsrnn_stream_batch_min", "fspen": "fspen_stream_batch_min", "lisennet": "lisennet_stream_batch_min"}


def _family(name):
    return name.split("_")[0]


def _audio(eng, n, hops, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (0.1 * torch.randn(n, hops * eng.cfg.hop_size, generator=g)).to(_dev())


def _dense(eng, full, cap, slots):
    """the dense state of len(slots) streams holding the records of the named slots of `full`, in call order"""
    n = len(slots)
    dense = eng.new_state(n)
    eng.import_slots(dense, n, list(range(n)), eng.export_slots(full, cap, list(slots)))
    return dense


def _slots_d(slots):
    return torch.tensor(slots, dtype=torch.int32, device=_dev())


def _strip(k):
    return k.replace("<slots>", "").replace(", slots", "")


def _check_kernels(k, k_ref):
    assert "slots" in k, k
    for bad in ("_sb_", "time-pipelined", "fused"):
        assert bad not in k, k
    assert _strip(k) == k_ref, (k, k_ref)


@pytest.mark.parametrize("name,kern", [("bsrnn_xxt", "wg8"), ("bsrnn_xxt", "waves4"), ("bsrnn_s", None), ("fspen", None), ("lisennet", None)])
def test_pool_step_has_the_bits_of_the_dense_step(name, kern):
    """capacity 5, slots [3, 0]: six hops of T = 1 and one call of T = 3 against fe_step(B = 2) on the dense twin; the other three slots keep
    every bit"""
    eng = _engine(name)
    cap, slots, H = 5, [3, 0], eng.cfg.hop_size
    full = _seeded_state(eng, cap, 4)
    before = full.clone()
    dense = _dense(eng, full, cap, slots)
    x = _audio(eng, 2, 9, 21)
    sd = _slots_d(slots)
    try:
        if kern is not None:
            eng.set_step_kernel(kern)
        for t0, T in [(t, 1) for t in range(6)] + [(6, 3)]:
            xt = x[:, t0 * H:(t0 + T) * H]
            y = eng.step_pool(xt, full, cap, sd, T=T)
            k = eng.last_step_kernel()
            ref = eng.step(xt, dense, T=T)
            k_ref = eng.last_step_kernel()
            torch.cuda.synchronize()
            _check_kernels(k, k_ref)
            if name == "bsrnn_xxt" and T == 1:
                assert ("bsrnn_ov_kernel<slots>" if kern == "wg8" else "bsrnn_frame_kernel<PART 1, slots>") in k, k
            assert _same(y, ref), f"hop {t0}, T = {T}: output differs (max {float((y - ref).abs().max()):.3e})"
            assert _same(eng.export_slots(full, cap, slots), eng.export_slots(dense, 2, [0, 1])), f"hop {t0}, T = {T}: the stepped slots' records differ"
    finally:
        if kern is not None:
            eng.set_step_kernel("wg8")
    others = [1, 2, 4]
    assert bool((eng.export_slots(before, cap, others) != 0).any(dim=1).all()), "the other slots are seeded non-zero"
    assert _same(eng.export_slots(full, cap, others), eng.export_slots(before, cap, others)), "a slot that was not named changed"


@pytest.mark.parametrize("name", MODELS)
def test_slots_out_of_range_write_zero_rows_and_touch_no_state(name):
    eng = _engine(name)
    cap, H = 4, eng.cfg.hop_size
    full = _seeded_state(eng, cap, 4, seed=3)
    before = full.clone()
    solo = eng.export_slots(before, cap, [1]).view(-1).clone()
    x = _audio(eng, 3, 1, 22)
    out = torch.full((3, H), 7.0, device=_dev())
    eng.step_pool(x, full, cap, _slots_d([1, 7, -2]), wav_out=out)
    assert "slots" in eng.last_step_kernel()
    ref = eng.step(x[:1], solo, T=1)
    torch.cuda.synchronize()
    assert float(out[1:].abs().max()) == 0.0, "rows of slots out of range must be exactly zero"
    assert _same(out[:1], ref), "slot 1 differs from its solo twin"
    assert _same(eng.export_slots(full, cap, [1]).view(-1), solo), "slot 1's record differs from its solo twin's"
    rest = full.clone()
    eng.import_slots(rest, cap, [1], eng.export_slots(before, cap, [1]))     # slot 1 put back: every other float must be as it was
    torch.cuda.synchronize()
    assert _same(rest, before), "the state outside slot 1 changed"


@pytest.mark.parametrize("name", ["bsrnn_xxt", "lisennet"])
def test_pool_step_above_the_streams_resident_at_once(name):
    """the persistent walk (two workgroups per CU for both models): resident + 5 streams of a capacity 3 larger, permuted, one hop"""
    eng = _engine(name)
    n = 2 * torch.cuda.get_device_properties(_dev()).multi_processor_count + 5
    cap, H = n + 3, eng.cfg.hop_size
    slots = [int(s) for s in np.random.default_rng(5).permutation(cap)[:n]]
    full = _seeded_state(eng, cap, 4, seed=4)
    dense = _dense(eng, full, cap, slots)
    x = _audio(eng, n, 1, 23)
    y = eng.step_pool(x, full, cap, _slots_d(slots))
    k = eng.last_step_kernel()
    # the twin under the same per-stream kernel: at this size LiSenNet's fe_step takes its stream-batched middle by default
    opt = SB_OPTION[name]
    old = eng.get_option(opt)
    try:
        eng.set_option(opt, 0)
        ref = eng.step(x, dense, T=1)
        k_ref = eng.last_step_kernel()
        torch.cuda.synchronize()
    finally:
        eng.set_option(opt, old)
    _check_kernels(k, k_ref)
    assert _same(y, ref), f"output differs (max {float((y - ref).abs().max()):.3e})"
    assert _same(eng.export_slots(full, cap, slots), eng.export_slots(dense, n, list(range(n)))), "records differ"


@pytest.mark.parametrize("name", sorted(SB_OPTION))
def test_pool_step_never_takes_the_stream_batched_kernels(name):
    eng = _engine(name)
    opt = SB_OPTION[name]
    old = eng.get_option(opt)
    cap, slots, H = 6, [4, 0, 5], eng.cfg.hop_size
    full = _seeded_state(eng, cap, 4, seed=5)
    dense = _dense(eng, full, cap, slots)
    x = _audio(eng, 3, 2, 24)
    try:
        for t in range(2):
            xt = x[:, t * H:(t + 1) * H]
            eng.set_option(opt, 0)
            ref = eng.step(xt, dense, T=1)
            assert "_sb_" not in eng.last_step_kernel()
            eng.set_option(opt, 1)
            y = eng.step_pool(xt, full, cap, _slots_d(slots))
            k = eng.last_step_kernel()
            torch.cuda.synchronize()
            assert "slots" in k and "_sb_" not in k, k
            assert _same(y, ref), f"hop {t}: output differs from fe_step with {opt} = 0"
        assert _same(eng.export_slots(full, cap, slots), eng.export_slots(dense, 3, [0, 1, 2]))
    finally:
        eng.set_option(opt, old)


@pytest.mark.parametrize("name", MODELS)
def test_a_permuted_pool_matches_the_oracle_hop_by_hop(name):
    m, orc, cfg, sr = _cached(name)
    eng = m.engine
    cap, slots, hops, H, tight = 5, [4, 1, 2], 8, cfg.hop_size, TIGHT_REL[_family(name)]
    x = make_input(3, hops * H, 4321, sr)
    xd = torch.from_numpy(x).to(_dev())
    full = eng.init_state(eng.new_state(cap), cap)
    sd = _slots_d(slots)
    caches = orc.initialize_cache(3)
    for t in range(hops):
        ref, *caches = orc.step(x[:, t * H:(t + 1) * H], *caches)
        y = eng.step_pool(xd[:, t * H:(t + 1) * H], full, cap, sd)
        torch.cuda.synchronize()
        _assert_close(y.cpu().numpy(), ref, f"{name} hop {t} wav_out", tight=tight)
        for j, (a, b) in enumerate(zip(eng.split_state(_dense(eng, full, cap, slots), 3), caches)):
            _assert_close(a.cpu().numpy(), np.asarray(b), f"{name} hop {t} cache {j}", tight=tight)


@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen"])
def test_streams_join_and_leave_a_pool_position_independently(name):
    """open a, b, c; step [a, c]; close a; open d; step [c, d, b]: every stream as if it were stepped alone with fe_step(B = 1) from a fresh
    record (a stream's results do not depend on its position in the batch or on the batch's size)"""
    eng = _engine(name)
    H = eng.cfg.hop_size
    pool = StreamPool(eng, 4)
    a, b, c = pool.open(), pool.open(), pool.open()
    x1, x2 = _audio(eng, 2, 1, 25), _audio(eng, 3, 1, 26)
    y1 = pool.step([a, c], x1).clone()
    assert "slots" in eng.last_step_kernel()
    rec_a = pool.export([a]).clone()
    pool.close(a)
    d = pool.open()
    assert d == a                                   # the freed slot, reset
    y2 = pool.step([c, d, b], x2).clone()
    torch.cuda.synchronize()

    def alone(rows):
        st = eng.new_state(1)
        return [eng.step(r.unsqueeze(0).contiguous(), st, T=1).clone() for r in rows], st

    (oa,), sa = alone([x1[0]])
    (oc1, oc2), sc = alone([x1[1], x2[0]])
    (od,), sdd = alone([x2[1]])
    (ob,), sbb = alone([x2[2]])
    torch.cuda.synchronize()
    assert _same(y1[0:1], oa) and _same(y1[1:2], oc1), "first step"
    assert _same(y2[0:1], oc2) and _same(y2[1:2], od) and _same(y2[2:3], ob), "second step"
    assert _same(rec_a.view(-1), sa), "record of the stream that left"
    for slot, st in [(c, sc), (d, sdd), (b, sbb)]:
        assert _same(pool.export([slot]).view(-1), st), f"record of slot {slot}"


@pytest.mark.parametrize("name", ["bsrnn_xxt", "lisennet"])
def test_step_pool_in_a_captured_graph_follows_the_slot_tensor(name):
    eng = _engine(name)
    dev = _dev()
    cap, n, H = 6, 2, eng.cfg.hop_size
    full = _seeded_state(eng, cap, 4, seed=6)
    twin = full.clone()
    sd = _slots_d([0, 1])
    x = torch.zeros(n, H, device=dev)
    y = torch.zeros(n, H, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(2):
            eng.step_pool(x, twin.clone(), cap, sd, wav_out=y)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.step_pool(x, full, cap, sd, wav_out=y)
    for r, sl in enumerate([[5, 2], [0, 4], [3, 5]]):
        sd.copy_(torch.tensor(sl, dtype=torch.int32))
        x.copy_(_audio(eng, n, 1, 30 + r))
        graph.replay()
        ref = eng.step_pool(x, twin, cap, sl)
        torch.cuda.synchronize()
        assert _same(y, ref), f"replay {r}"
        assert _same(full, twin), f"replay {r}: state"


@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen", "lisennet"])
def test_what_lds_held_before_does_not_matter(name):
    eng = _engine(name)
    cap, slots, H = 4, [2, 3, 0], eng.cfg.hop_size
    x = _audio(eng, 3, 2, 27)
    res = []
    for poison in (False, True):
        full = _seeded_state(eng, cap, 4, seed=7)
        outs = []
        for t in range(2):
            out = torch.full((3, H), float("nan"), device=_dev())
            if poison:
                eng.poison_lds()
            eng.step_pool(x[:, t * H:(t + 1) * H], full, cap, _slots_d(slots), wav_out=out)
            outs.append(out)
        torch.cuda.synchronize()
        res.append((torch.cat(outs, 1), full.clone()))
    assert bool(torch.isfinite(res[1][0]).all()) and bool(torch.isfinite(res[1][1]).all())
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1]), "the result depends on what was in LDS before the launch"


@pytest.mark.parametrize("name", MODELS)
def test_loaded_handles_answer_every_bad_call_as_fe_step_slots_does(name):
    """code and wording of fe_step_slots on a loaded FastEnhancer handle, before any device work (the pointers are never dereferenced)"""
    from test_cpu_step_pool import BAD_ARGS, NULL
    ref, eng = _engine("fe_b"), _engine(name)
    assert ref.cfg.hop_size == eng.cfg.hop_size == 256
    err = lambda: _lib.load().fe_last_error().decode()
    for args in BAD_ARGS:
        want = (ref.lib.fe_step_slots(ref._h, *args, NULL), err())
        assert want[0] == -1 and ("1 <= n <= capacity" in want[1] or "stride" in want[1]), want
        got = (eng.lib.fe_step_pool(eng._h, *args, NULL), err())
        assert got == want, (args, got, want)
    unloaded = hip_engine(name, _dev())
    assert unloaded.lib.fe_step_pool(unloaded._h, c_void_p(0x1000), 256, c_void_p(0x1000), 4, c_void_p(0x1000), c_void_p(0x1000), 256, 1, 1, NULL) == -4       # FE_ERR_NO_WEIGHTS
