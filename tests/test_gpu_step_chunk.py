"""The time-pipelined streaming chunk on the GPU (fe_step_chunk through Engine.step_chunk, enhance_stream(chunk_hops=...) and
StreamPool.catch_up).

fe_step_chunk(B, T) means fe_step(B, T): with the pipeline off it makes fe_step's launch (equal bits); with it on, the T frames of each
stream run on co-resident workgroups and a second launch overlap-adds them, which agrees with the walk to fp32 rounding - wav_out and every
state tensor - and leaves cache_stft (a copy of input samples) bit-identical.  The models are the smallest shipped shapes that reach every
hand-over kind - fe_t / fe_b (GRU state only), fe_ln_b, fe_dprnn_b, fe_tk_b (conv rings) and fe_dpt_t (K / V rings with a head), all n_fft
512 / hop 256, where the overlap N - H equals the hop - and every overlap geometry of the shipped shapes: fe_m (hop 160: N - H = 352 > 2 H,
frames overlap four deep), fe48_b_h480 (n_fft 1024 / hop 480: N - H = 544, the hop is not aligned with N / 2) and fe_l (hop 100: N - H =
412 > 4 H, six deep - the one geometry where T = 4 hops do not cover the overlap and the call must walk)."""
import numpy as np
import pytest
import torch

from common import hip_model
from fastenhancer_amd.serving import StreamPool
from oracle.weightgen import make_input
from test_gpu_parity import TIGHT_REL, _assert_close, _model

pytestmark = pytest.mark.gpu

MODELS = ["fe_t", "fe_b", "fe_ln_b", "fe_dprnn_b", "fe_tk_b", "fe_dpt_t", "fe_m", "fe48_b_h480", "fe_l"]

PIPE_REL = 3e-5            # max |pipelined - serial| <= PIPE_REL * max |serial|: the bound of the pipelined-vs-serial tests of test_gpu_parity.py


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _min_hops(cfg):
    """the fewest hops the pipelined launch takes: T >= 4 and T H >= N - H (the second launch's new caches then hold nothing of the old)"""
    return max(4, -(-(cfg.n_fft - cfg.hop_size) // cfg.hop_size))


_MODELS = {}


def _cached(name):
    """(mirror with the oracle's seeded weights, oracle, oracle config, sampling rate) per configuration name, built once"""
    if name not in _MODELS:
        _MODELS[name] = _model(name)[:4]
    return _MODELS[name]


def _engine(name):
    return _cached(name)[0].engine


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _seed_hops(name):
    return 35 if name == "fe_dpt_t" else 4          # (dptransformer: lookbehind 31 - the ring head is past a wrap)


def _seed_audio(eng, B, hops, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return 0.1 * torch.randn(B, hops * eng.cfg.hop_size, generator=g)


def _seeded_state(eng, B, hops, seed=0):
    """a state of B streams after `hops` per-hop launches on random audio: non-zero everywhere a hop writes"""
    H = eng.cfg.hop_size
    x = _seed_audio(eng, B, hops, seed).to(_dev())
    state = eng.new_state(B)
    for t in range(hops):
        eng.step(x[:, t * H:(t + 1) * H], state, T=1)
    torch.cuda.synchronize()
    return state


def _chunk(eng, width, x, state, **kw):
    """step_chunk under fe_set_time_pipeline(width); the default setting is restored"""
    try:
        eng.set_time_pipeline(width)
        y = eng.step_chunk(x, state, **kw)
        k = eng.last_step_kernel()
        torch.cuda.synchronize()
    finally:
        eng.set_time_pipeline(-1)
    return y, k


def _assert_pipe_close(got, ref, what):
    scale = float(ref.abs().max())
    diff = float((got - ref).abs().max())
    print(f"{what}: max abs diff {diff:.3e}, scale {scale:.3e}, ratio {diff / max(scale, 1e-30):.3e}")
    assert torch.isfinite(got).all(), what
    assert diff <= PIPE_REL * scale, f"{what}: max abs diff {diff:.3e} > {PIPE_REL:.0e} x {scale:.3e}"


def _assert_state_close(eng, B, got, ref, what):
    """every state tensor in the reference's view (dptransformer K / V oldest first, whatever the ring heads); cache_stft equal bits"""
    a, b = eng.split_state(got, B), eng.split_state(ref, B)
    assert len(a) == len(b)
    assert _same(a[0], b[0]), f"{what}: cache_stft differs"
    for i, (u, v) in enumerate(zip(a[1:], b[1:]), 1):
        _assert_pipe_close(u, v, f"{what}: state tensor {i}")


@pytest.mark.parametrize("name", MODELS)
def test_chunks_match_the_oracle_stepping_hop_by_hop(name):
    """two consecutive pipelined chunks of 13 hops, then three fe_step hops on the state they leave: outputs of all three parts and the
    caches after each against the fp32 oracle, within the project's own bound"""
    m, orc, cfg, sr = _cached(name)
    eng = m.engine
    B, T, H, tight = 3, 13, cfg.hop_size, TIGHT_REL["fastenhancer"]
    seed_hops = _seed_hops(name)
    x0 = _seed_audio(eng, B, seed_hops).numpy()
    x = make_input(B, (2 * T + 3) * H, 4243, sr)
    caches = orc.initialize_cache(B)
    for t in range(seed_hops):
        _, *caches = orc.step(x0[:, t * H:(t + 1) * H], *caches)
    refs, ref_caches = [], []
    for t in range(2 * T + 3):
        o, *caches = orc.step(x[:, t * H:(t + 1) * H], *caches)
        refs.append(o)
        if t + 1 in (T, 2 * T, 2 * T + 3):
            ref_caches.append([np.array(c) for c in caches])
    ref = np.concatenate(refs, axis=1)

    state = _seeded_state(eng, B, seed_hops)
    xd = torch.from_numpy(x).to(_dev())
    parts = [(0, T), (T, 2 * T), (2 * T, 2 * T + 3)]
    for i, (t0, t1) in enumerate(parts):
        if i < 2:
            y, k = _chunk(eng, -1, xd[:, t0 * H:t1 * H], state)
            assert "time-pipelined, streaming" in k and "stream_ola_kernel" in k, k
        else:
            y = torch.cat([eng.step(xd[:, t * H:(t + 1) * H], state, T=1) for t in range(t0, t1)], dim=1)
            torch.cuda.synchronize()
        _assert_close(y.cpu().numpy(), ref[:, t0 * H:t1 * H], f"{name} part {i} wav_out", tight=tight)
        for j, (a, b) in enumerate(zip(eng.split_state(state, B), ref_caches[i])):
            _assert_close(a.cpu().numpy(), b, f"{name} cache {j} after part {i}", tight=tight)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", MODELS)
def test_pipelined_chunk_agrees_with_the_serial_walk(name, B):
    """with the pipeline off the call IS fe_step(T) (equal bits); widths 3 and 8 agree with it to fp32 rounding at T = 4 (the least the
    pipeline takes: 4, or 5 for hop 100 where 4 hops are shorter than the overlap), 13 (a multiple of neither width) and 40, cache_stft bit
    for bit"""
    eng = _engine(name)
    H = eng.cfg.hop_size
    start = _seeded_state(eng, B, _seed_hops(name), seed=B)
    for T in (_min_hops(eng.cfg), 13, 40):
        x = torch.from_numpy(make_input(B, T * H, 100 + T, 16000)).to(_dev())
        s_step = start.clone()
        y_step = eng.step(x, s_step, T=T)
        k_step = eng.last_step_kernel()
        s_walk = start.clone()
        y_walk, k_walk = _chunk(eng, 0, x, s_walk)
        assert k_walk == k_step, (k_walk, k_step)
        assert _same(y_walk, y_step) and _same(s_walk, s_step), f"T={T}: the chunk with the pipeline off is not fe_step"
        for width in (3, 8):
            s = start.clone()
            y, k = _chunk(eng, width, x, s)
            assert "time-pipelined, streaming" in k, (width, k)
            _assert_pipe_close(y, y_walk, f"{name} B={B} T={T} width {width}: wav_out")
            _assert_state_close(eng, B, s, s_walk, f"{name} B={B} T={T} width {width}")


def test_chunk_shorter_than_the_overlap_takes_the_walk():
    """fe_l: 4 hops of 100 samples do not cover the overlap of 412, so the second launch could not form the new caches from the chunk
    alone - the call makes fe_step's launch (equal bits, fe_step's kernel), although the work size for (B, 4) is not zero; 5 hops pipeline"""
    eng = _engine("fe_l")
    B, H = 2, eng.cfg.hop_size
    assert _min_hops(eng.cfg) == 5 and eng.chunk_work_floats(B, 4) > 0
    start = _seeded_state(eng, B, 4, seed=2)
    x = torch.from_numpy(make_input(B, 5 * H, 41, 16000)).to(_dev())
    s_step, s_chunk = start.clone(), start.clone()
    y_step = eng.step(x[:, :4 * H], s_step, T=4)
    k_step = eng.last_step_kernel()
    y_chunk, k = _chunk(eng, -1, x[:, :4 * H], s_chunk)
    assert k == k_step and "time-pipelined" not in k, (k, k_step)
    assert _same(y_chunk, y_step) and _same(s_chunk, s_step)
    _, k = _chunk(eng, -1, x, start.clone())
    assert "time-pipelined, streaming" in k, k


@pytest.mark.parametrize("name", MODELS)
def test_pipelined_chunk_is_bit_reproducible(name):
    eng = _engine(name)
    B, T, H = 3, 13, eng.cfg.hop_size
    start = _seeded_state(eng, B, _seed_hops(name), seed=7)
    x = torch.from_numpy(make_input(B, T * H, 55, 16000)).to(_dev())
    runs = []
    for _ in range(2):
        s = start.clone()
        y, k = _chunk(eng, -1, x, s)
        assert "time-pipelined" in k, k
        runs.append((y.clone(), s))
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])


@pytest.mark.parametrize("name", ["fe_b", "fe_tk_b", "fe_dpt_t", "fe_m", "fe48_b_h480"])
def test_strided_rows_and_untouched_memory(name):
    """rows further apart than T*H with sentinels between them, a state with a guard tail: the sentinels, wav_in and the guard keep their
    bits, and the result is that of the same call on packed rows"""
    eng = _engine(name)
    B, T, H = 3, 13, eng.cfg.hop_size
    n, pad, mark = eng.state_floats(B), 37, -123.25
    start = _seeded_state(eng, B, _seed_hops(name), seed=3)
    x = torch.from_numpy(make_input(B, T * H, 77, 16000)).to(_dev())
    s_ref = start.clone()
    y_ref, _ = _chunk(eng, -1, x, s_ref)

    xin = torch.full((B, T * H + pad), mark, device=_dev())
    xin[:, :T * H] = x
    xin_before = xin.clone()
    out = torch.full((B, T * H + pad + 5), mark, device=_dev())
    big = torch.full((n + 256,), mark, device=_dev())
    big[:n] = start
    y, k = _chunk(eng, -1, xin[:, :T * H], big[:n], wav_out=out[:, :T * H])
    assert "time-pipelined" in k, k
    assert y.data_ptr() == out.data_ptr()
    assert _same(xin, xin_before), "wav_in or the sentinels between its rows were written"
    assert bool((out[:, T * H:] == mark).all()), "the sentinels between the rows of wav_out were written"
    assert bool((big[n:] == mark).all()), "memory behind fe_state_floats(h, B) was written"
    assert _same(out[:, :T * H], y_ref) and _same(big[:n], s_ref)


def test_kernel_names():
    eng = _engine("fe_b")
    B, H = 2, eng.cfg.hop_size
    for T, width, piped in [(8, -1, True), (8, 3, True), (8, 0, False), (8, 1, False), (3, -1, False), (1, -1, False)]:
        x = torch.from_numpy(make_input(B, T * H, 9, 16000)).to(_dev())
        eng.step(x, eng.new_state(B), T=T)
        k_step = eng.last_step_kernel()
        _, k = _chunk(eng, width, x, eng.new_state(B))
        if piped:
            assert k == "fe_frame_kernel<time-pipelined, streaming> + stream_ola_kernel [shape B]", (T, width, k)
        else:
            assert k == k_step and "time-pipelined" not in k, (T, width, k, k_step)


def test_step_chunk_can_be_captured_into_a_hip_graph():
    """a caller-supplied work buffer: the call allocates nothing - one capture, two replays with new audio, each equal in bits to an eager
    call from the same state"""
    eng = _engine("fe_b")
    B, T, H = 1, 8, eng.cfg.hop_size
    work = torch.empty(eng.chunk_work_floats(B, T), device=_dev())
    audio = [torch.from_numpy(make_input(B, T * H, 300 + i, 16000)).to(_dev()) for i in range(3)]
    x = audio[0].clone()
    y = torch.empty(B, T * H, device=_dev())
    state = _seeded_state(eng, B, 4, seed=11)
    eng.step_chunk(x, state.clone(), work=work)               # (first launch outside the capture: sets the function attribute)
    assert "time-pipelined" in eng.last_step_kernel()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s_graph = state.clone()
    with torch.cuda.graph(g):
        eng.step_chunk(x, s_graph, wav_out=y, work=work)
    s_graph.copy_(state)
    s_eager = state.clone()
    for i in (1, 2):
        x.copy_(audio[i])
        g.replay()
        torch.cuda.synchronize()
        y_eager = eng.step_chunk(audio[i], s_eager, work=torch.empty_like(work))
        torch.cuda.synchronize()
        assert _same(y, y_eager) and _same(s_graph, s_eager), f"replay {i}"


def test_enhance_stream_in_chunks_agrees_with_the_hop_loop():
    from fastenhancer_amd.streaming import enhance_stream
    m = _cached("fe_b")[0]
    wav = torch.from_numpy(make_input(1, 16000, 21, 16000)).to(_dev())
    y_loop = enhance_stream(m, wav)
    y_chunks = enhance_stream(m, wav, chunk_hops=64)
    assert "time-pipelined, streaming" in m.engine.last_step_kernel()          # (1 s = 64 hops: one chunk)
    assert y_chunks.shape == y_loop.shape == wav.shape
    _assert_pipe_close(y_chunks, y_loop, "enhance_stream(chunk_hops=64) vs the hop loop")


@pytest.mark.parametrize("name", ["fe_b", "fe_dpt_t"])
def test_stream_pool_catch_up(name):
    """slot a takes a 40-hop backlog in one call while slot b is not named: b keeps its bits, and a's output - the backlog and two live hops
    after it - is that of a twin stepped hop by hop"""
    eng = _engine(name)
    H, T = eng.cfg.hop_size, 40
    pool = StreamPool(eng, 4)
    a, b = pool.open(), pool.open()
    seed = _seed_audio(eng, 2, _seed_hops(name), seed=5).to(_dev())
    for t in range(seed.shape[1] // H):
        pool.step([a, b], seed[:, t * H:(t + 1) * H])
    twin = pool.export([a]).clone().view(-1)                   # (a state record is a capacity-1 state)
    b_before = pool.export([b]).clone()
    x = torch.from_numpy(make_input(1, (T + 2) * H, 808, 16000)).to(_dev())
    ys = [pool.catch_up(a, x[:, :T * H], T)]
    assert "time-pipelined" in eng.last_step_kernel()
    for t in range(T, T + 2):
        ys.append(pool.step([a], x[:, t * H:(t + 1) * H]).clone())
    y = torch.cat(ys, dim=1)
    torch.cuda.synchronize()
    assert _same(pool.export([b]), b_before), "the slot that was not named changed"
    y_twin = torch.cat([eng.step(x[:, t * H:(t + 1) * H], twin, T=1) for t in range(T + 2)], dim=1)
    torch.cuda.synchronize()
    _assert_pipe_close(y, y_twin, f"{name}: catch_up + two live hops vs the twin")
    _assert_state_close(eng, 1, pool.export([a]).view(-1), twin, f"{name}: state after catch_up + two live hops")


def test_baseline_family_takes_the_path_of_fe_step():
    eng = hip_model("bsrnn_xxt", device=_dev()).engine
    B, T, H = 2, 5, eng.cfg.hop_size
    assert eng.chunk_work_floats(B, T) == 0
    x = torch.from_numpy(make_input(B, T * H, 5, 16000)).to(_dev())
    s1, s2 = eng.new_state(B), eng.new_state(B)
    y1 = eng.step(x, s1, T=T)
    k1 = eng.last_step_kernel()
    y2 = eng.step_chunk(x, s2, T=T)
    torch.cuda.synchronize()
    assert eng.last_step_kernel() == k1
    assert _same(y1, y2) and _same(s1, s2)


def test_stream_chunks_command_line(tmp_path, monkeypatch):
    """scripts/stream_chunks.py: test_streaming.py's flags + --chunk-hops; with the flag the file goes through step_chunk and agrees with
    the hop-by-hop run of the same script to fp32 rounding"""
    import yaml
    from scipy.io import wavfile
    from common import MODEL_KWARGS, build_oracle
    from fastenhancer_amd.scripts import stream_chunks
    kw, sr, seed = MODEL_KWARGS["fe_t"]
    sd = build_oracle("fe_t")[1]
    logs = tmp_path / "logs" / "run"
    logs.mkdir(parents=True)
    (logs / "config.yaml").write_text(yaml.safe_dump({"model": "fastenhancer.default", "model_kwargs": kw, "data": {"sampling_rate": sr}}))
    torch.save({"model": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "epoch": 7}, str(logs / "00007.pth"))
    wavfile.write(str(tmp_path / "a.wav"), sr, make_input(1, 5000, 91, sr)[0])
    monkeypatch.chdir(tmp_path)
    common = ["-n", "run", "--audio-path", str(tmp_path / "a.wav"), "--save-output", "--n-fft", "512", "--hop-size", "256"]
    stream_chunks.main(common + ["--output-path", str(tmp_path / "hops.wav")])
    stream_chunks.main(common + ["--output-path", str(tmp_path / "chunks.wav"), "--chunk-hops", "8"])
    (r1, y1), (r2, y2) = wavfile.read(str(tmp_path / "hops.wav")), wavfile.read(str(tmp_path / "chunks.wav"))
    assert r1 == r2 == sr and y1.shape == y2.shape == (5000,)
    _assert_pipe_close(torch.from_numpy(np.asarray(y2, np.float32)), torch.from_numpy(np.asarray(y1, np.float32)), "stream_chunks CLI")
