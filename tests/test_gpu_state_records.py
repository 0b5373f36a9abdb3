"""State records on the GPU (fe_state_export_slots / fe_state_import_slots through Engine.export_slots / import_slots, StreamPool.export /
adopt / move / resize, PacketPool.move): a moved stream continues bit for bit, a record is a capacity-1 state, nothing but the named slots is
touched, for every family's region kinds.  All state comparisons are on the bits (int32 views): NaN patterns count."""
import numpy as np
import pytest
import torch

from common import BSRNN_KWARGS, FSPEN_KWARGS, LISENNET_KWARGS, hip_model, product_config
from fastenhancer_amd.engine import _ptr, _stream
from fastenhancer_amd.serving import PacketPool, StreamPool

pytestmark = pytest.mark.gpu

FE_SHAPES = ["fe_t", "fe_tk_b", "fe_dpt_t"]            # STFT caches + GRU states; conv caches; K / V rings + head
BASELINES = ["bsrnn_xxt", "fspen", "lisennet"]
SHAPES = FE_SHAPES + BASELINES
FE_OK, FE_ERR_INVALID_ARG = 0, -1


def _dev(i=0):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device(f"cuda:{i}")


_ENGINES = {}


def _engine(name, dev=0):
    """seeded random weights; the FastEnhancer shapes with the step kernel pinned (the bit-identity contract holds per kernel)"""
    if (name, dev) not in _ENGINES:
        eng = hip_model(name, device=_dev(dev)).engine
        if name in FE_SHAPES:
            eng.set_step_kernel("waves4")
        _ENGINES[(name, dev)] = eng
    return _ENGINES[(name, dev)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _noise(rows, n, seed, dev=0):
    return (0.1 * torch.randn(rows, n, generator=torch.Generator().manual_seed(seed))).to(_dev(dev))


# ---------------------------------------------------------------- the documented layout (include/fastenhancer_hip.h), written out here
def _regions(name):
    """[(rows, len)]: the state of B streams is these tensors back to back, each [rows][B][len]"""
    if name in BSRNN_KWARGS:
        kw = BSRNN_KWARGS[name][0]
        return [(1, 256), (1, 256), (2 * kw["num_layers"], 31 * 2 * kw["num_channels"])]          # h0, c0, h1, c1, ...: [B*31, 2C]
    if name == "fspen":
        d = FSPEN_KWARGS[0]["dpe_kwargs"]
        return [(1, 256), (1, 256), (d["num_blocks"] * d["groups"], (d["freq"] // d["groups"]) * d["channels"])]
    if name == "lisennet":
        nb = LISENNET_KWARGS[0]["n_blocks"]
        return [(1, 256), (1, 256), (1, 257), (1, 4 * 257), (1, 8 * 128), (1, 12 * 64)] + [(1, 32 * 24), (1, 32 * 2 * 32)] * nb + [(1, 4 * 256)]
    c = product_config(name)
    r = [(1, c.n_fft - c.hop_size)] * 2
    if c.dpt:
        r += [(2 * c.rf_blocks, c.rf_freq * c.rf_channels * c.lookbehind), (1, 1)]                  # K, V rings per block, then head
    else:
        r += [(c.rf_blocks, c.rf_freq * c.rf_channels)]
    if c.time_kernel:
        r += [(2 * c.n_layers, (c.kernel_size_time - 1) * c.F1 * c.channels)]
    return r


def _slot_index(name, cap, slot, dev=0):
    """the floats of `slot` in a state of `cap` streams, in record order (= the capacity-1 layout)"""
    idx, off = [], 0
    for rows, ln in _regions(name):
        for r in range(rows):
            idx.append(off + (r * cap + slot) * ln + torch.arange(ln))
        off += rows * cap * ln
    return torch.cat(idx).to(_dev(dev))


def _sentinel(n, seed, dev=0):
    """n floats of random bit patterns, NaNs with payloads, infinities and denormals among them"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    k = torch.arange(n)
    b = torch.where(k % 7 == 3, (0x7FC00000 + 1 + k % 4096).to(torch.int32), b)                     # quiet NaNs, payload k
    b = torch.where(k % 11 == 5, (0x7F800001 + k % 4096).to(torch.int32), b)                        # signalling NaNs
    b = torch.where(k % 13 == 6, torch.tensor(0x7F800000, dtype=torch.int32), b)                    # +inf
    return b.view(torch.float32).to(_dev(dev))


def _sentinel_pair(name):
    eng = _engine(name)
    src, dst = _sentinel(eng.state_floats(5), 1), _sentinel(eng.state_floats(3), 2)
    assert src.numel() == 5 * eng.record_floats and sum(r * ln for r, ln in _regions(name)) == eng.record_floats
    return eng, src, dst


# ---------------------------------------------------------------- 1. a moved stream continues bit for bit
@pytest.mark.parametrize("name", FE_SHAPES)
def test_a_moved_stream_continues_bit_for_bit(name):
    eng = _engine(name)
    H = eng.cfg.hop_size
    T0 = 35 if name == "fe_dpt_t" else 3                  # dptransformer: the ring head is past a wrap of its 31 slots
    a = StreamPool(eng, 5)
    for _ in range(5):
        a.open()
    a.close(0), a.close(3)
    a.step([4, 1, 2], _noise(3, T0 * H, 11), T=T0)
    b = StreamPool(eng, 3)
    for _ in range(3):
        b.open()
    other = _noise(1, 4 * H, 12)
    b.step([1], other[:, :2 * H].contiguous(), T=2)       # slot 1 of pool B: another live stream
    rec = a.export([4, 2])
    assert tuple(rec.shape) == (2, eng.record_floats) and a.active == [1, 2, 4]
    eng.import_slots(b.state, 3, [0, 2], rec)
    x = _noise(3, 2 * H, 13)
    for t in range(2):
        xa = x[:, t * H:(t + 1) * H].contiguous()
        ya = a.step([4, 1, 2], xa)
        xb = torch.stack([xa[0], other[0, (2 + t) * H:(3 + t) * H], xa[2]])
        yb = b.step([0, 1, 2], xb)
        torch.cuda.synchronize()
        assert _same(ya[[0, 2]], yb[[0, 2]]), f"hop {t}: max diff {float((ya[[0, 2]] - yb[[0, 2]]).abs().max()):.3e}"
    assert _same(a.export([4, 2]), b.export([0, 2]))
    if name == "fe_dpt_t":
        assert float(rec[0, -1]) == T0 % 31 and float(a.export([4])[0, -1]) == (T0 + 2) % 31        # the head went along, un-rotated


# ---------------------------------------------------------------- 2. a record is a capacity-1 state
def test_a_record_is_a_capacity_one_state():
    eng = _engine("fe_t")
    H = eng.cfg.hop_size
    pool = StreamPool(eng, 5)
    for _ in range(5):
        pool.open()
    pool.step([3, 0, 4], _noise(3, 3 * H, 21), T=3)
    solo = pool.export([4])[0].clone()                    # handed to fe_step(B = 1) as it stands
    assert solo.numel() == eng.state_floats(1)
    x = _noise(1, 2 * H, 22)
    for t in range(2):
        xt = x[:, t * H:(t + 1) * H].contiguous()
        assert _same(eng.step(xt, solo), pool.step([4], xt))
    assert _same(solo, pool.export([4])[0])


# ---------------------------------------------------------------- 3. nothing else is touched
@pytest.mark.parametrize("name", SHAPES)
def test_export_reads_and_import_writes_exactly_the_named_slots(name):
    eng, src, dst = _sentinel_pair(name)
    src0, dst0 = src.clone(), dst.clone()
    rec = eng.export_slots(src, 5, [4, 2])
    torch.cuda.synchronize()
    assert _same(src, src0), "export wrote to the source state"
    for i, s in enumerate([4, 2]):
        assert _same(rec[i], src0[_slot_index(name, 5, s)]), f"record {i} is not slot {s} in the capacity-1 layout"
    eng.import_slots(dst, 3, [0, 2], rec)
    torch.cuda.synchronize()
    want = dst0.clone()
    for i, s in enumerate([0, 2]):
        want[_slot_index(name, 3, s)] = rec[i]
    changed = torch.cat([_slot_index(name, 3, 0), _slot_index(name, 3, 2)])
    assert changed.unique().numel() == 2 * eng.record_floats
    assert _same(dst, want), f"{int((_bits(dst) != _bits(want)).sum())} floats differ from the documented layout"
    assert _same(src, src0)


# ---------------------------------------------------------------- 4. out-of-range slots
@pytest.mark.parametrize("name", SHAPES)
def test_out_of_range_slots_export_a_fresh_record_and_import_nothing(name):
    eng, src, dst = _sentinel_pair(name)
    dst0 = dst.clone()
    slots = torch.tensor([-1, 5], dtype=torch.int32, device=_dev())
    rec = torch.full((2, eng.record_floats), 3.0, device=_dev())
    eng.export_slots(src, 5, slots, out=rec)                          # (Engine raises unless the library returned FE_OK)
    fresh = torch.full((eng.state_floats(1),), 1.0, device=_dev())
    assert eng.lib.fe_state_init(eng._h, _ptr(fresh), 1, _stream(_dev())) == FE_OK
    torch.cuda.synchronize()
    assert _same(rec[0], fresh) and _same(rec[1], fresh)
    for sl in (slots, torch.tensor([3, -2 ** 31], dtype=torch.int32, device=_dev())):     # (3: the first slot past the destination's capacity)
        eng.import_slots(dst, 3, sl, _sentinel(2 * eng.record_floats, 3).view(2, -1))
    torch.cuda.synchronize()
    assert _same(dst, dst0)


# ---------------------------------------------------------------- 5. alignment paths
@pytest.mark.parametrize("name", SHAPES)
def test_records_off_a_16_byte_boundary_give_the_same_records(name):
    eng, src, dst = _sentinel_pair(name)
    rf = eng.record_floats
    buf = torch.zeros(2 * rf + 8, device=_dev())
    aligned, shifted = buf[:2 * rf].view(2, rf), buf[1:1 + 2 * rf].view(2, rf)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    rec_a = eng.export_slots(src, 5, [1, 3], out=aligned).clone()
    buf.zero_()
    rec_s = eng.export_slots(src, 5, [1, 3], out=shifted).clone()
    torch.cuda.synchronize()
    assert float(buf[0]) == 0.0 and float(buf[1 + 2 * rf:].abs().max()) == 0.0, "export wrote outside its records"
    assert _same(rec_a, rec_s) and _same(rec_a[0], src[_slot_index(name, 5, 1)]) and _same(rec_a[1], src[_slot_index(name, 5, 3)])
    dst_s = dst.clone()
    eng.import_slots(dst_s, 3, [2, 1], shifted)
    buf[:2 * rf].copy_(rec_a.view(-1))
    eng.import_slots(dst, 3, [2, 1], aligned)
    torch.cuda.synchronize()
    assert _same(dst, dst_s) and _same(dst[_slot_index(name, 3, 2)], rec_a[0]) and _same(dst[_slot_index(name, 3, 1)], rec_a[1])


# ---------------------------------------------------------------- 6. pinned host records
@pytest.mark.parametrize("name", ["fe_tk_b", "lisennet"])
def test_pinned_host_records_match_the_device_path(name):
    eng, src, dst = _sentinel_pair(name)
    rf = eng.record_floats
    rec_d = eng.export_slots(src, 5, [0, 4, 2])
    rec_h = eng.export_slots(src, 5, [0, 4, 2], out=torch.zeros(3, rf).pin_memory())
    torch.cuda.synchronize()
    assert not rec_h.is_cuda and _same(rec_h, rec_d.cpu())
    states = []
    for rec in (rec_d, rec_h):
        st = torch.full((eng.state_floats(3),), 1.0, device=_dev())
        assert eng.lib.fe_state_init(eng._h, _ptr(st), 3, _stream(_dev())) == FE_OK
        eng.import_slots(st, 3, [1, 0, 2], rec)
        torch.cuda.synchronize()
        states.append(st)
    assert _same(states[0], states[1]) and _same(states[0][_slot_index(name, 3, 1)], rec_d[0])
    pageable = torch.zeros(3 * rf)
    sl = torch.tensor([0, 1, 2], dtype=torch.int32, device=_dev())
    for fn in ("fe_state_export_slots", "fe_state_import_slots"):
        assert getattr(eng.lib, fn)(eng._h, _ptr(src), 5, _ptr(sl), _ptr(pageable), 3, _stream(_dev())) == FE_ERR_INVALID_ARG
        assert "page-locked" in eng.lib.fe_last_error().decode()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. the baseline families: compaction of a plain fe_step batch
@pytest.mark.parametrize("name", BASELINES)
def test_baseline_batch_is_permuted_and_compacted_bit_for_bit(name):
    """Bit equality throughout: these families' per-stream kernels compute a stream's hop from that stream's rows alone, at any position and
    batch size below their stream-batched thresholds."""
    eng = _engine(name)
    H = eng.cfg.hop_size
    x = _noise(4, 4 * H, 31)
    hop = lambda xs, t: xs[:, t * H:(t + 1) * H].contiguous()
    full = eng.new_state(4)
    for t in range(2):
        eng.step(hop(x, t), full)
    rec = eng.export_slots(full, 4, [0, 1, 2, 3]).clone()
    perm = [2, 0, 3, 1]
    twin = eng.new_state(4)
    eng.import_slots(twin, 4, perm, rec)
    pair = eng.new_state(2)
    eng.import_slots(pair, 2, [0, 1], rec[[0, 3]])
    xp = torch.empty_like(x)
    xp[perm] = x
    for t in range(2, 4):
        y = eng.step(hop(x, t), full)
        yp = eng.step(hop(xp, t), twin)
        y2 = eng.step(hop(x[[0, 3]], t), pair)
        torch.cuda.synchronize()
        assert _same(yp[perm], y), f"hop {t}: permuted batch, max diff {float((yp[perm] - y).abs().max()):.3e}"
        assert _same(y2, y[[0, 3]]), f"hop {t}: compacted batch, max diff {float((y2 - y[[0, 3]]).abs().max()):.3e}"
    after = eng.export_slots(full, 4, [0, 1, 2, 3])
    assert not _same(after, rec)
    assert _same(eng.export_slots(twin, 4, perm), after)
    assert _same(eng.export_slots(pair, 2, [0, 1]), after[[0, 3]])


# ---------------------------------------------------------------- 8. StreamPool.resize / move, PacketPool.move
def test_resize_keeps_the_streams_at_their_slots():
    eng = _engine("fe_t")
    H = eng.cfg.hop_size
    pool, ref = StreamPool(eng, 2), StreamPool(eng, 4)
    assert [pool.open(), pool.open()] == [0, 1] and [ref.open(), ref.open()] == [0, 1]
    with pytest.raises(RuntimeError, match="all 2 slots are open"):
        pool.open()
    x = _noise(2, 6 * H, 41)
    for t in range(6):
        if t == 3:
            old = pool.state
            pool.resize(4)
            assert pool.state is not old and pool.capacity == 4 and pool.state.numel() == eng.state_floats(4)
            assert pool.open() == 2
        xt = x[:, t * H:(t + 1) * H].contiguous()
        assert _same(pool.step([1, 0], xt), ref.step([1, 0], xt)), f"hop {t}"
    assert _same(pool.export([0, 1]), ref.export([0, 1]))
    with pytest.raises(ValueError, match="slot 2 is open"):
        pool.resize(2)
    pool.close(2)
    pool.resize(2)
    assert pool.capacity == 2 and _same(pool.export([0, 1]), ref.export([0, 1]))


def _move_between_pools(eng_a, eng_b):
    """a stream stepped 3 hops in a pool of eng_a, moved to one of eng_b, stepped 2 more: against the same stream never moved"""
    H = eng_a.cfg.hop_size
    x = _noise(1, 5 * H, 51)
    src, dst, ref = StreamPool(eng_a, 3), StreamPool(eng_b, 2), StreamPool(eng_a, 3)
    dst.open()                                                        # (the stream lands in slot 1 there)
    s, r = [src.open(), src.open()][1], [ref.open(), ref.open()][1]
    outs, want = [], []
    for t in range(5):
        if t == 3:
            s = src.move(s, dst)
            assert s == 1 and src.active == [0] and dst.active == [0, 1]
        xt = x[:, t * H:(t + 1) * H].contiguous()
        pool = src if t < 3 else dst
        outs.append(pool.step([s], xt.to(pool.engine.device)).cpu())
        want.append(ref.step([r], xt).cpu())
    assert _same(torch.cat(outs), torch.cat(want))
    assert _same(dst.export([s]).cpu(), ref.export([r]).cpu())


def test_move_between_two_pools_of_one_device():
    _move_between_pools(_engine("fe_t"), _engine("fe_t"))
    with pytest.raises(ValueError, match="different configs"):
        a = StreamPool(_engine("fe_t"), 1)
        a.move(a.open(), StreamPool(_engine("fe_tk_b"), 1))


def test_move_between_two_devices():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    _move_between_pools(_engine("fe_t", 0), _engine("fe_t", 1))


def test_packet_pool_move_carries_state_rings_and_counters():
    """160-sample int16 packets (10 ms: not a multiple of the hop); the stream moves to a pool with another ring_hops while it holds
    un-stepped input and un-pulled output: the pulled PCM is that of a stream that never moved"""
    eng = _engine("fe_t")
    rng = np.random.default_rng(61)
    pcm = torch.from_numpy((rng.standard_normal(40 * 160) * 3000).astype(np.int16))
    ref_pool, a, b = PacketPool(eng, 1, ring_hops=6, T_max=2), PacketPool(eng, 2, ring_hops=6, T_max=2), PacketPool(eng, 3, ring_hops=9, T_max=2)
    b.open()
    r, pool, s = ref_pool.open(), a, [a.open(), a.open()][1]
    got, want = [], []
    for tick in range(40):
        pkt = pcm[tick * 160:(tick + 1) * 160]
        pool.push(s, pkt), ref_pool.push(r, pkt)
        pool.tick(), ref_pool.tick()
        if tick == 14:
            assert pool._pushed[s] > pool._stepped[s] > pool._pulled[s]
            s, pool = pool.move(s, b), b
            assert s == 1 and a.active == [0]
        if tick % 3 == 0:
            got.append(pool.pull(s)), want.append(ref_pool.pull(r))
    got.append(pool.pull(s)), want.append(ref_pool.pull(r))
    got, want = torch.cat(got), torch.cat(want)
    assert got.numel() == want.numel() >= 40 * 160 - 512 and torch.equal(got, want)
    assert int(got.abs().max()) > 0


# ---------------------------------------------------------------- 9. graph replay
def test_export_import_in_a_captured_graph_follow_the_slot_tensors():
    name = "fe_dpt_t"
    eng, src, dst = _sentinel_pair(name)
    dev = _dev()
    rec = torch.zeros(2, eng.record_floats, device=dev)
    from_d, to_d = torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.tensor([0, 1], dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):                                        # warm-up: nothing is set up inside the capture
        eng.import_slots(dst.clone(), 3, to_d, eng.export_slots(src, 5, from_d, out=rec))
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.export_slots(src, 5, from_d, out=rec)
        eng.import_slots(dst, 3, to_d, rec)
    want = dst.clone()
    for frm, to in [([4, 2], [0, 2]), ([1, 3], [2, 1]), ([0, 4], [1, 0])]:
        from_d.copy_(torch.tensor(frm, dtype=torch.int32))
        to_d.copy_(torch.tensor(to, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        for f, t in zip(frm, to):
            want[_slot_index(name, 3, t)] = src[_slot_index(name, 5, f)]
        assert _same(dst, want), (frm, to)
