"""The polyphase resampler on the GPU (fe_resample, fe_resample_streams[_pinned], Resampler, ResampledPacketPool, the callers' --resample).

The reference is tests/resample_oracle.py, the contract's direct form in float64; the bound on the fp32 kernel's error is the contract's,
(K + 2) 2^-24 S peak, computed from the taps (error_bound) - derived, not measured.  Everything else is an equality of bits: a stream under
any packetisation against the whole-signal call, int16 against float input, page-locked against device buffers, the pool against its
steps composed by hand.  Sizes: K - 1 and K straddle the history length, 997 is odd and - at 16 -> 48 and 16 -> 44.1 kHz - more than two
output tiles of 1024; a 441-sample packet at those rates spans two tiles of one stream."""
import numpy as np
import pytest
import torch

import resample_oracle as ro
from fastenhancer_amd import _lib
from fastenhancer_amd.engine import _ptr, _stream
from fastenhancer_amd.resample import Resampler
from fastenhancer_amd.serving import PacketPool, ResampledPacketPool

pytestmark = pytest.mark.gpu

PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (16000, 48000), (16000, 44100)]
SENT = {torch.float32: 123.25, torch.int16: 12345}
CYCLE = [1, 7, 0, 160, 441, 3, 64]
_RS = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rs(sr_in, sr_out):
    if (sr_in, sr_out) not in _RS:
        _RS[(sr_in, sr_out)] = Resampler(sr_in, sr_out, _dev())
    return _RS[(sr_in, sr_out)]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _signal(rows, n, seed, dtype=torch.float32, peak=0.5):
    x = (2.0 * torch.rand(rows, n, generator=torch.Generator().manual_seed(seed)) - 1.0) * peak
    return x if dtype == torch.float32 else torch.round(x * 32768.0).to(torch.int16)


def _as_float64(x):
    return x.double().numpy() / (32768.0 if x.dtype == torch.int16 else 1.0)


def _whole_strided(rs, x, out_dtype, pad=5):
    """fe_resample on rows `pad` elements apart beyond their length, sentinels between them: (the rows' outputs [B, n_out], the whole output buffer)"""
    B, n = x.shape
    n_out = rs.out_count(n)
    xin = torch.full((B, n + pad), SENT[x.dtype], dtype=x.dtype)
    xin[:, :n] = x
    xin = xin.to(_dev())
    out = torch.full((B, n_out + pad), SENT[out_dtype], dtype=out_dtype, device=_dev())
    fmt = lambda t: _lib.FE_AUDIO_S16 if t.dtype == torch.int16 else _lib.FE_AUDIO_F32
    _lib.check(rs.lib.fe_resample(rs._h, _ptr(xin), n + pad, fmt(xin), n, _ptr(out), n_out + pad, fmt(out), B, _stream(_dev())), "fe_resample")
    torch.cuda.synchronize()
    return out[:, :n_out].cpu(), out.cpu()


# ------------------------------------------------------------------ 1. whole signals against the oracle, within the bound
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_whole_signals_match_the_oracle_within_the_bound(sr_in, sr_out, dtype):
    rs = _rs(sr_in, sr_out)
    up, down, K = rs.up, rs.down, rs.taps_per_output
    h = rs.taps().numpy()
    for n in (1, K - 1, K, 997):
        x = _signal(3, n, seed=n + up, dtype=dtype)
        y, buf = _whole_strided(rs, x, dtype)
        assert rs.last_kernel() == "fe_resample_kernel<whole>"
        xd = _as_float64(x)
        want = ro.resample(xd, up, down, h=h)
        assert y.shape == want.shape == (3, rs.out_count(n))
        bound = ro.error_bound(up, down, np.abs(xd).max(), h=h)
        if dtype == torch.int16:            # (the output is rounded to the int16 grid: half a step more; |y| <= 0.5 S < 1 here - nothing clamps)
            err = np.abs(y.double().numpy() / 32768.0 - want).max()
            bound += 0.5 / 32768.0
        else:
            err = np.abs(y.double().numpy() - want).max()
        print(f"{sr_in}->{sr_out} {dtype} N={n}: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert err <= bound, (n, err, bound)
        assert bool((buf[:, rs.out_count(n):] == SENT[dtype]).all()), "an element between two output rows lost the sentinel"


# ------------------------------------------------------------------ 2. a stream is the whole-signal call's prefix, bit for bit
def _stream_run(rs, xs, slots, capacity, shifts, steps, dtype_in, dtype_out, pinned=False):
    """xs [n_streams, N] pushed through step_streams[_pinned] in packets of CYCLE sizes (stream i starts the cycle at shifts[i]):
    (outputs per stream, final state, consumed per stream); every call checks produced, the sentinels past it and the unnamed rows"""
    n_streams = xs.shape[0]
    cap_in, n_in_max = max(CYCLE), max(CYCLE)
    cap_out = rs.out_count(n_in_max) + 1
    state = rs.new_state(capacity)
    named = set(slots)
    for s in range(capacity):
        if s not in named:
            state[s] = 777.0
    untouched = state.clone()
    make = (lambda *shape, dtype: torch.zeros(*shape, dtype=dtype).pin_memory()) if pinned else (lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=_dev()))
    xin = make(n_streams * cap_in, dtype=dtype_in)
    out = make(n_streams * cap_out + 3, dtype=dtype_out)
    produced = make(n_streams, dtype=torch.int32)
    consumed = [0] * n_streams
    got = [[] for _ in range(n_streams)]
    call = rs.step_streams_pinned if pinned else rs.step_streams
    for t in range(steps):
        sizes = [CYCLE[(t + shifts[i]) % len(CYCLE)] for i in range(n_streams)]
        desc = []
        xin.fill_(SENT[dtype_in])
        out.fill_(SENT[dtype_out])
        for i, n in enumerate(sizes):
            xin[i * cap_in:i * cap_in + n] = xs[i, consumed[i]:consumed[i] + n]
            desc.append((slots[i], n, i * cap_in, i * cap_out + 3))
        call(xin, state, capacity, desc, out, n_in_max, produced=produced)
        torch.cuda.synchronize()
        assert rs.last_kernel() == ("fe_resample_kernel<streams,pinned>" if pinned else "fe_resample_kernel<streams>")
        o, p = out.cpu(), produced.cpu().tolist()
        written = torch.zeros(o.numel(), dtype=torch.bool)
        for i, n in enumerate(sizes):
            assert p[i] == rs.produced(consumed[i], n) == ro.emitted(consumed[i] + n, rs.up, rs.down) - ro.emitted(consumed[i], rs.up, rs.down)
            lo = i * cap_out + 3
            got[i].append(o[lo:lo + p[i]].clone())
            written[lo:lo + p[i]] = True
            consumed[i] += n
        assert bool((o[~written] == SENT[dtype_out]).all()), "an output element past `produced` lost the sentinel"
    rest = [s for s in range(capacity) if s not in named]
    assert _same(state[rest], untouched[rest]), "the row of a slot the calls never named changed"
    return [torch.cat(g) for g in got], state, consumed


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_a_stream_is_the_prefix_of_the_whole_signal_bit_for_bit(sr_in, sr_out):
    rs = _rs(sr_in, sr_out)
    steps = 14                                              # two rounds of the cycle
    xs = _signal(3, 2 * sum(CYCLE), seed=sr_in // 100 + sr_out // 1000)
    whole = rs(xs.to(_dev())).cpu()
    outs, state, consumed = _stream_run(rs, xs, [5, 0, 2], 6, [0, 3, 5], steps, torch.float32, torch.float32)
    assert consumed == [2 * sum(CYCLE)] * 3
    M = ro.emitted(consumed[0], rs.up, rs.down)
    assert 0 < M < whole.shape[1]
    for i in range(3):
        assert outs[i].numel() == M
        assert _same(outs[i], whole[i, :M]), f"stream {i} differs from the whole-signal call"
    # the documented row: the last K - 1 samples oldest first, then the count's two words
    K = rs.taps_per_output
    st = state.cpu()
    for i, slot in enumerate([5, 0, 2]):
        assert _same(st[slot, :K - 1], xs[i, consumed[i] - (K - 1):consumed[i]])
        assert st[slot, K - 1:K + 1].view(torch.int32).tolist() == [consumed[i], 0]
    # rows are plain data: a stream continues from a copy of its row in another slot
    moved = rs.new_state(2)
    moved[1] = state[5]
    tail = _signal(1, 100, seed=9)
    out = torch.zeros(rs.out_count(100) + 1, device=_dev())
    made = torch.zeros(1, dtype=torch.int32, device=_dev())
    rs.step_streams(tail[0].to(_dev()).contiguous(), moved, 2, [(1, 100, 0, 0)], out, 100, produced=made)
    both = rs(torch.cat([xs[0], tail[0]]).to(_dev())).cpu()
    M2 = ro.emitted(consumed[0] + 100, rs.up, rs.down)
    assert int(made[0]) == M2 - M and _same(out[:M2 - M].cpu(), both[M:M2])


# ------------------------------------------------------------------ 2b. downsampling across tiles
def test_downsampling_by_six_walks_tiles_of_less_than_1024_outputs():
    """48 -> 8 kHz: a tile may advance 4096 input samples at most, so it holds 682 outputs, not 1024 - the host's tile sizing and its bound
    on the input tile (xcap) at a ratio below 1/4.  5000 samples are two tiles of the whole-signal call; a 4500-sample packet is two tiles
    of one stream.  Bound and bit equality as above."""
    rs = _rs(48000, 8000)
    assert (rs.up, rs.down, rs.taps_per_output) == (1, 6, 121)
    x = _signal(2, 5000, seed=31)
    y, buf = _whole_strided(rs, x, torch.float32)
    assert y.shape == (2, 834)
    h = rs.taps().numpy()
    err = np.abs(y.double().numpy() - ro.resample(x.double().numpy(), 1, 6, h=h)).max()
    bound = ro.error_bound(1, 6, float(x.abs().max()), h=h)
    print(f"48000->8000 N=5000: max err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, (err, bound)
    assert bool((buf[:, 834:] == SENT[torch.float32]).all())
    state = rs.new_state(2)
    out = torch.full((2, 800), SENT[torch.float32], device=_dev())
    made = torch.zeros(2, dtype=torch.int32, device=_dev())
    xd = x.to(_dev())
    got = [[], []]
    for lo, n in ((0, 4500), (4500, 500)):
        out.fill_(SENT[torch.float32])
        rs.step_streams(xd, state, 2, [(1, n, lo, 0), (0, n, 5000 + lo, 800)], out, 4500, produced=made)
        torch.cuda.synchronize()
        p = made.cpu().tolist()
        assert p == [rs.produced(lo, n)] * 2 and (lo > 0 or p[0] == 740)
        for i in range(2):
            got[i].append(out[i, :p[i]].cpu())
            assert bool((out[i, p[i]:] == SENT[torch.float32]).all())
    M = ro.emitted(5000, 1, 6)
    for i in range(2):
        assert _same(torch.cat(got[i]), y[i, :M])


# ------------------------------------------------------------------ 3. int16
@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (16000, 44100)])
def test_int16_input_is_the_float_input_and_int16_output_is_the_rounded_float_output(sr_in, sr_out):
    rs = _rs(sr_in, sr_out)
    s = _signal(2, 997, seed=3, dtype=torch.int16, peak=1.0)
    from_s16 = rs(s.to(_dev()), out_dtype=torch.float32)
    from_f32 = rs((s.float() / 32768.0).to(_dev()))
    assert _same(from_s16.cpu(), from_f32.cpu())
    # a full-scale square wave: the filter's overshoot passes +-1 and must clamp at both ends
    sq = torch.where((torch.arange(997) // 97) % 2 == 0, 1.0, -1.0).float().reshape(1, -1)
    yf = rs(sq.to(_dev())).cpu()
    yi = rs(sq.to(_dev()), out_dtype=torch.int16).cpu()
    assert float(yf.max()) > 1.0 and float(yf.min()) < -1.0
    want = torch.from_numpy(ro.pcm16(yf.numpy()))
    assert _same(yi, want)
    assert int(yi.max()) == 32767 and int(yi.min()) == -32768
    # NaN -> 0
    bad = _signal(1, 400, seed=4)
    bad[0, 200] = float("nan")
    yf = rs(bad.to(_dev())).cpu()
    yi = rs(bad.to(_dev()), out_dtype=torch.int16).cpu()
    nan = torch.isnan(yf)
    assert bool(nan.any()) and not bool(nan.all())
    assert bool((yi[nan] == 0).all()) and _same(yi, torch.from_numpy(ro.pcm16(yf.numpy())))


# ------------------------------------------------------------------ 4. descriptors that point outside
def test_bad_descriptors_touch_nothing():
    rs = _rs(48000, 16000)
    cap, n_in_max, in_count, out_count = 8, 300, 1000, 400
    big_in = torch.full((in_count + 200,), SENT[torch.int16], dtype=torch.int16)
    x = _signal(1, in_count, seed=6, dtype=torch.int16)[0]
    big_in[100:100 + in_count] = x
    big_in = big_in.to(_dev())
    big_out = torch.full((out_count + 200,), SENT[torch.int16], dtype=torch.int16, device=_dev())
    state = rs.new_state(cap)
    warm = torch.zeros(cap * 100, dtype=torch.int16, device=_dev())
    rs.step_streams(big_in[100:400].contiguous(), state, cap, [(s, 300, 0, s * 100) for s in range(cap)], warm, 300)      # every row a live stream
    torch.cuda.synchronize()
    before = state.clone()
    p300 = rs.produced(300, 300)
    cases = [(0, 300, in_count - 299, 0),          # input range runs one past the end
             (1, 300, -1, 0),                      # ... starts before the buffer
             (2, 300, 0, out_count - p300 + 1),    # output range runs one past the end
             (3, 300, 0, -1),                      # ... starts before the buffer
             (8, 300, 0, 0), (-1, 300, 0, 0),      # slot outside [0, capacity)
             (4, -5, 0, 0),                        # negative n_in: clamped to 0
             (5, 100000, 300, 200)]                # n_in above n_in_max: clamped to n_in_max
    desc = Resampler.pack_desc(cases).to(_dev())
    produced = torch.full((len(cases),), -7, dtype=torch.int32, device=_dev())
    view_in, view_out = big_in[100:100 + in_count], big_out[100:100 + out_count]
    rs.step_streams(view_in, state, cap, desc, view_out, n_in_max, produced=produced)
    torch.cuda.synchronize()
    assert produced.cpu().tolist() == [0, 0, 0, 0, 0, 0, 0, p300]
    rest = [0, 1, 2, 3, 4, 6, 7]
    assert _same(state[rest].cpu(), before[rest].cpu()), "the state of a skipped stream changed"
    # the clamped stream ran as a stream of n_in_max samples does
    twin = before.clone()
    twin_out = torch.full((p300,), SENT[torch.int16], dtype=torch.int16, device=_dev())
    rs.step_streams(view_in[300:600].contiguous(), twin, cap, [(5, 300, 0, 0)], twin_out, n_in_max)
    torch.cuda.synchronize()
    assert _same(state[5].cpu(), twin[5].cpu())
    o = big_out.cpu()
    assert _same(o[300:300 + p300], twin_out.cpu())
    o[300:300 + p300] = SENT[torch.int16]
    assert bool((o == SENT[torch.int16]).all()), "an output element outside the one valid range was written"
    assert _same(big_in.cpu()[100:100 + in_count], x)


# ------------------------------------------------------------------ 5. page-locked buffers
def test_pinned_equals_device_bit_for_bit():
    rs = _rs(48000, 16000)
    xs = _signal(3, 2 * sum(CYCLE), seed=8, dtype=torch.int16, peak=0.9)
    dev = _stream_run(rs, xs, [5, 0, 2], 6, [0, 3, 5], 14, torch.int16, torch.int16, pinned=False)
    pin = _stream_run(rs, xs, [5, 0, 2], 6, [0, 3, 5], 14, torch.int16, torch.int16, pinned=True)
    for a, b in zip(dev[0], pin[0]):
        assert a.numel() > 0 and _same(a, b)
    assert _same(dev[1].cpu(), pin[1].cpu())
    with pytest.raises(ValueError, match="page-locked"):
        rs.step_streams_pinned(torch.zeros(8, dtype=torch.int16), rs.new_state(1), 1, [(0, 8, 0, 0)], torch.zeros(8, dtype=torch.int16), 8)


# ------------------------------------------------------------------ 6. the offline caller
def test_offline_caller_resamples_a_48_khz_file(tmp_path, monkeypatch):
    """scripts/enhance_dir.py --resample (test_offline.py run with the flag's switch on) against Resampler + model by hand, bit for bit"""
    import yaml
    from scipy.io import wavfile
    from common import MODEL_KWARGS, build_oracle
    from fastenhancer_amd.scripts import enhance_dir, test_offline
    from fastenhancer_amd.scripts.common import build_model
    kw, sr, _ = MODEL_KWARGS["fe_b"]
    _, sd, _, _ = build_oracle("fe_b")
    logs = tmp_path / "logs" / "run"
    logs.mkdir(parents=True)
    hps = {"model": "fastenhancer.default", "model_kwargs": kw, "data": {"sampling_rate": sr}}
    (logs / "config.yaml").write_text(yaml.safe_dump(hps))
    torch.save({"model": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "epoch": 7}, str(logs / "00007.pth"))
    noisy_dir = tmp_path / "noisy"
    noisy_dir.mkdir()
    t = np.arange(14400) / 48000.0
    x = (0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * np.random.default_rng(1).standard_normal(t.size)).astype(np.float32)
    wavfile.write(str(noisy_dir / "a.wav"), 48000, x)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="resample the file first"):        # off by default
        test_offline.main(["-n", "run", "-i", str(noisy_dir), "-o", str(tmp_path / "out"), "--batch", "1"])
    with pytest.raises(ValueError, match="resample the file first"):        # ... in the caller that carries the flag too
        enhance_dir.main(["-n", "run", "-i", str(noisy_dir), "-o", str(tmp_path / "out"), "--batch", "1"])
    enhance_dir.main(["-n", "run", "-i", str(noisy_dir), "-o", str(tmp_path / "out"), "--batch", "1", "--resample"])
    rate, y = wavfile.read(str(tmp_path / "out" / "a.wav"))
    assert rate == sr == 16000 and y.dtype == np.float32
    model = build_model(hps, "cuda:0", offline=True, checkpoint=str(logs / "00007.pth"))
    x16 = Resampler(48000, 16000, _dev())(torch.from_numpy(x).to(_dev()))
    assert x16.numel() == 4800
    with torch.no_grad():
        want, _ = model(x16.unsqueeze(0))
    assert _same(torch.from_numpy(y), want.squeeze().cpu())


# ------------------------------------------------------------------ 7. the pool
@pytest.mark.parametrize("name", ["fe_b", "bsrnn_xxt"])
def test_resampled_packet_pool_equals_its_steps_composed_by_hand(name):
    from test_gpu_step_chunk import _engine
    eng = _engine(name)
    H = eng.cfg.hop_size
    pool = ResampledPacketPool(eng, 2, 8, 48000, T_max=2, max_packet=1920)
    assert pool.inner.H == H == 256
    hand = PacketPool(eng, 2, 8, T_max=2)
    down, back = Resampler(48000, 16000, _dev()), Resampler(16000, 48000, _dev())
    st_down, st_back = down.new_state(2), back.new_state(2)
    sig = _signal(2, 6 * 960, seed=21, dtype=torch.int16, peak=0.3)
    a, b = pool.open(), pool.open()
    assert (hand.open(), hand.open()) == (a, b) == (0, 1)
    total = {a: 0, b: 0}
    for tick in range(6):
        got, want = {}, {}
        pushed = [a] if tick == 2 else [a, b]               # (slot b misses a packet once: the streams' phases part)
        for s in pushed:
            pool.push(s, sig[s, tick * 960:(tick + 1) * 960])
        pool.tick()
        for s in (a, b):
            got[s] = pool.pull(s)
        # by hand, on device buffers: 48 -> 16 kHz, the packet pool, 16 -> 48 kHz
        for s in pushed:
            n16 = down.produced(tick * 960 if s == a else (tick - (tick > 2)) * 960, 960)
            y16 = torch.zeros(n16, dtype=torch.int16, device=_dev())
            down.step_streams(sig[s, tick * 960:(tick + 1) * 960].to(_dev()).contiguous(), st_down, 2, [(s, 960, 0, 0)], y16, 960)
            hand.push(s, y16.cpu())
        hand.tick()
        for s in (a, b):
            y = hand.pull(s)
            if y.numel():
                made = torch.zeros(1, dtype=torch.int32, device=_dev())
                y48 = torch.zeros(back.out_count(y.numel()) + 1, dtype=torch.int16, device=_dev())
                back.step_streams(y.to(_dev()).contiguous(), st_back, 2, [(s, y.numel(), 0, 0)], y48, y.numel(), produced=made)
                want[s] = y48[:int(made[0])].cpu()
            else:
                want[s] = torch.zeros(0, dtype=torch.int16)
            assert _same(got[s], want[s]), (name, tick, s)
            total[s] += got[s].numel()
    assert total[a] > 3 * 960 and total[b] > 2 * 960 and bool(pool.state_in.any()) and bool(pool.state_out.any())
    assert _same(pool.state_in.cpu(), st_down.cpu()) and _same(pool.state_out.cpu(), st_back.cpu())
    assert pool.to_model.last_kernel() == pool.to_client.last_kernel() == "fe_resample_kernel<streams,pinned>"
    pool.close(b)
    assert not bool(pool.state_in[b].any()) and bool(pool.state_in[a].any())
