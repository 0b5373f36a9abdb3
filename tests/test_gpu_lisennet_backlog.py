"""LiSenNet's streaming state carried through the time pipeline (fe_step_backlog under an explicit fe_set_time_pipeline(P >= 2) with a work
buffer of fe_lisennet_backlog_work_floats; Engine.step_backlog(work=...), enhance_stream(chunk_hops=...), StreamPool.catch_up).

The pipelined call is zero_counters_kernel, lisennet_frame_kernel<time-pipelined, streaming> - frame 0 takes the nine caches from the
caller's state, the last frames leave theirs there, in place - and stream_ola_kernel.  It agrees with fe_step(B, T) to fp32 rounding (wav_out
and every state tensor), leaves cache_stft bit-identical, and is fe_step's launch wherever the pipeline is not asked for or cannot run.

Bounds: PIPE_REL = 3e-5 (tests/test_gpu_step_chunk.py, asserted by its _assert_pipe_close) for pipelined against serial, TIGHT_REL["lisennet"]
(tests/test_gpu_parity.py) against the fp32 oracle.  Every state here is seeded non-zero by four fe_step hops."""
import numpy as np
import pytest
import torch

from fastenhancer_amd.serving import StreamPool
from oracle.weightgen import make_input
from test_gpu_parity import TIGHT_REL, _assert_close
from test_gpu_step_chunk import _assert_pipe_close, _assert_state_close, _cached, _dev, _same, _seed_audio, _seeded_state

pytestmark = pytest.mark.gpu

SEED_HOPS = 4
N_CACHES = 9            # phase, enc2, enc3, enc4, per block (2) the GRU state and the ConvGLU's two frames, dec


def _eng():
    return _cached("lisennet")[0].engine


def _backlog(eng, width, x, state, T=None, sized=True, **kw):
    """step_backlog under fe_set_time_pipeline(width), with the family's work buffer unless the caller passes work= or sized=False;
    the default setting is restored"""
    try:
        eng.set_time_pipeline(width)
        if sized and "work" not in kw:
            kw["work"] = eng.lisennet_backlog_work(x.shape[0], x.shape[1] // eng.cfg.hop_size)
        y = eng.step_backlog(x, state, T=T, **kw)
        k = eng.last_step_kernel()
        torch.cuda.synchronize()
    finally:
        eng.set_time_pipeline(-1)
    return y, k


def _piped(k):
    return "lisennet_frame_kernel<time-pipelined, streaming>" in k and "stream_ola_kernel" in k


def _assert_seeded(eng, B, state):
    """every one of the nine caches (and both STFT caches) of the seeded state is non-zero"""
    parts = eng.split_state(state, B)
    assert len(parts) == 2 + N_CACHES, len(parts)
    for j, c in enumerate(parts):
        assert float(c.abs().max()) > 0, f"tensor {j} of the seeded state is zero"


@pytest.mark.parametrize("B", [1, 3])
def test_pipelined_backlog_agrees_with_the_serial_walk(B):
    """T = 4 (the least the pipeline takes), 5 (the ConvGLU's frames T-2 and T-1 next to frames 0 and 1: the tightest in-place case) and 9
    at widths 2 (a workgroup runs several frames), 3 and 8, from one seeded state: wav_out and every state tensor within PIPE_REL of
    fe_step(B, T), cache_stft bit for bit; the sentinels between the rows of wav_out keep their bits"""
    eng = _eng()
    H, pad, mark = eng.cfg.hop_size, 37, -123.25
    start = _seeded_state(eng, B, SEED_HOPS, seed=B)
    _assert_seeded(eng, B, start)
    for T in (4, 5, 9):
        x = torch.from_numpy(make_input(B, T * H, 100 + T, 16000)).to(_dev())
        s_step = start.clone()
        y_step = eng.step(x, s_step, T=T)
        torch.cuda.synchronize()
        xin = torch.full((B, T * H + pad), mark, device=_dev())
        xin[:, :T * H] = x
        for width in (2, 3, 8):
            out = torch.full((B, T * H + pad + 5), mark, device=_dev())
            s = start.clone()
            y, k = _backlog(eng, width, xin[:, :T * H], s, wav_out=out[:, :T * H])
            what = f"lisennet B={B} T={T} width {width}"
            assert _piped(k), (what, k)
            assert y.data_ptr() == out.data_ptr()
            assert bool((out[:, T * H:] == mark).all()), f"{what}: the sentinels between the rows of wav_out were written"
            _assert_pipe_close(y, y_step, f"{what}: wav_out")
            _assert_state_close(eng, B, s, s_step, what)


def test_backlog_chunks_match_the_oracle_stepping_hop_by_hop():
    """two consecutive pipelined chunks of 13 hops, then three fe_step hops on the state they leave - the outputs of all three parts and
    the caches after each against the fp32 oracle stepped hop by hop (a state written in the wrong layout or half shows here)"""
    m, orc, cfg, sr = _cached("lisennet")
    eng = m.engine
    B, T, H, tight = 3, 13, cfg.hop_size, TIGHT_REL["lisennet"]
    x0 = _seed_audio(eng, B, SEED_HOPS).numpy()
    x = make_input(B, (2 * T + 3) * H, 4243, sr)
    caches = orc.initialize_cache(B)
    for t in range(SEED_HOPS):
        _, *caches = orc.step(x0[:, t * H:(t + 1) * H], *caches)
    assert len(caches) == 2 + N_CACHES
    for j, c in enumerate(caches):
        assert np.abs(np.asarray(c)).max() > 0, f"cache {j} of the seeded state is zero"
    refs, ref_caches = [], []
    for t in range(2 * T + 3):
        o, *caches = orc.step(x[:, t * H:(t + 1) * H], *caches)
        refs.append(o)
        if t + 1 in (T, 2 * T, 2 * T + 3):
            ref_caches.append([np.array(c) for c in caches])
    ref = np.concatenate(refs, axis=1)

    state = _seeded_state(eng, B, SEED_HOPS)
    _assert_seeded(eng, B, state)
    xd = torch.from_numpy(x).to(_dev())
    for i, (t0, t1) in enumerate([(0, T), (T, 2 * T), (2 * T, 2 * T + 3)]):
        if i < 2:
            y, k = _backlog(eng, 8, xd[:, t0 * H:t1 * H], state)
            assert _piped(k), k
        else:
            y = torch.cat([eng.step(xd[:, t * H:(t + 1) * H], state, T=1) for t in range(t0, t1)], dim=1)
            torch.cuda.synchronize()
        _assert_close(y.cpu().numpy(), ref[:, t0 * H:t1 * H], f"lisennet part {i} wav_out", tight=tight)
        for j, (a, b) in enumerate(zip(eng.split_state(state, B), ref_caches[i])):
            _assert_close(a.cpu().numpy(), b, f"lisennet cache {j} after part {i}", tight=tight)


@pytest.mark.parametrize("T,width", [(9, 3), (5, 2)])
def test_lisennet_backlog_work_floats_cover_the_call(T, width):
    """exactly lisennet_backlog_work_floats(B, T) floats, NaN-filled, with a sentinel region behind them: the sentinels keep their bits and
    the results are finite and those of a run with a roomy zero-filled buffer, bit for bit (the method of tests/test_gpu_work_bounds.py) -
    and once more with the LDS of every CU poisoned first; a buffer one float short is refused before the call"""
    eng = _eng()
    B, H, guard, mark = 2, eng.cfg.hop_size, 4096, 7.5
    need = eng.lisennet_backlog_work_floats(B, T)
    assert need >= B * T * eng.cfg.n_fft and eng.backlog_work_floats(B, T) == 0
    start = _seeded_state(eng, B, SEED_HOPS, seed=13)
    _assert_seeded(eng, B, start)
    x = torch.from_numpy(make_input(B, T * H, 77, 16000)).to(_dev())
    results = []
    for kind in ("tight", "roomy", "poisoned"):
        if kind == "roomy":
            buf = torch.zeros(4 * need + guard, device=_dev())
        else:
            buf = torch.full((need + guard,), float("nan"), device=_dev())
            buf[need:] = mark
        if kind == "poisoned":
            eng.poison_lds()
        s = start.clone()
        y, k = _backlog(eng, width, x, s, work=buf if kind == "roomy" else buf[:need])
        assert _piped(k), k
        if kind != "roomy":
            assert bool((buf[need:] == mark).all()), f"floats behind lisennet_backlog_work_floats({B}, {T}) were written ({kind})"
        results.append((y.clone(), s))
    assert torch.isfinite(results[0][0]).all() and torch.isfinite(results[0][1]).all()
    for y, s in results[1:]:
        assert _same(results[0][0], y) and _same(results[0][1], s)
    with pytest.raises(ValueError, match="work has"):
        _backlog(eng, width, x, start.clone(), work=torch.empty(need - 1, device=_dev()))


def test_backlog_is_fe_step_where_the_pipeline_is_not_taken():
    """an explicit width with work=None, and with T = 3 and a work buffer: the bits and the kernel string of eng.step"""
    eng = _eng()
    B, H = 2, eng.cfg.hop_size
    start = _seeded_state(eng, B, SEED_HOPS, seed=5)
    spare = torch.empty(eng.lisennet_backlog_work_floats(B, 9), device=_dev())
    for T, width, work in [(9, 2, None), (9, 8, None), (3, 2, spare), (3, 8, spare)]:
        x = torch.from_numpy(make_input(B, T * H, 60 + T, 16000)).to(_dev())
        s_step, s = start.clone(), start.clone()
        y_step = eng.step(x, s_step, T=T)
        k_step = eng.last_step_kernel()
        y, k = _backlog(eng, width, x, s, work=work)
        assert k == k_step and "time-pipelined" not in k, (T, width, k, k_step)
        assert _same(y, y_step) and _same(s, s_step), f"T={T} width {width}: not the bits of fe_step"


def test_the_pipelined_backlog_can_be_captured_into_a_hip_graph():
    """a caller-supplied work buffer: the call allocates nothing - one capture, three replays on successive audio chunks with the state
    carried, against three eager calls"""
    eng = _eng()
    B, T, H = 1, 8, eng.cfg.hop_size
    work = torch.empty(eng.lisennet_backlog_work_floats(B, T), device=_dev())
    audio = [torch.from_numpy(make_input(B, T * H, 300 + i, 16000)).to(_dev()) for i in range(3)]
    x = audio[0].clone()
    y = torch.empty(B, T * H, device=_dev())
    state = _seeded_state(eng, B, SEED_HOPS, seed=11)
    try:
        eng.set_time_pipeline(4)
        eng.step_backlog(x, state.clone(), work=work)             # (first launch outside the capture)
        assert _piped(eng.last_step_kernel())
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s_graph = state.clone()
        with torch.cuda.graph(g):
            eng.step_backlog(x, s_graph, wav_out=y, work=work)
        s_graph.copy_(state)
        s_eager = state.clone()
        for i in range(3):
            x.copy_(audio[i])
            g.replay()
            torch.cuda.synchronize()
            y_eager = eng.step_backlog(audio[i], s_eager, work=torch.empty_like(work))
            assert _piped(eng.last_step_kernel())
            torch.cuda.synchronize()
            _assert_pipe_close(y, y_eager, f"replay {i}: wav_out")
            _assert_state_close(eng, B, s_graph, s_eager, f"replay {i}")
    finally:
        eng.set_time_pipeline(-1)


def test_stream_pool_catch_up_on_a_lisennet_pool():
    """slot a of a 2-slot LiSenNet pool takes an 8-hop backlog in one call under width 4, then two live hops (catch_up of one hop:
    fe_step's launch), while slot b is not named: b keeps its bits, and a's output and state are those of a twin stepped hop by hop"""
    eng = _eng()
    H, T = eng.cfg.hop_size, 8
    pool = StreamPool(eng, 2)
    a, b = pool.open(), pool.open()
    seed = _seed_audio(eng, 2, SEED_HOPS, seed=5).to(_dev())
    for t in range(SEED_HOPS):
        for i, slot in enumerate((a, b)):
            pool.catch_up(slot, seed[i:i + 1, t * H:(t + 1) * H], 1)
    twin = pool.export([a]).clone().view(-1)                   # (a state record is a capacity-1 state)
    _assert_seeded(eng, 1, twin)
    b_before = pool.export([b]).clone()
    x = torch.from_numpy(make_input(1, (T + 2) * H, 808, 16000)).to(_dev())
    try:
        eng.set_time_pipeline(4)
        ys = [pool.catch_up(a, x[:, :T * H], T).clone()]
        assert _piped(eng.last_step_kernel()), eng.last_step_kernel()
        for t in range(T, T + 2):
            ys.append(pool.catch_up(a, x[:, t * H:(t + 1) * H], 1).clone())
            assert "time-pipelined" not in eng.last_step_kernel()
    finally:
        eng.set_time_pipeline(-1)
    y = torch.cat(ys, dim=1)
    torch.cuda.synchronize()
    assert _same(pool.export([b]), b_before), "the slot that was not named changed"
    y_twin = torch.cat([eng.step(x[:, t * H:(t + 1) * H], twin, T=1) for t in range(T + 2)], dim=1)
    torch.cuda.synchronize()
    _assert_pipe_close(y, y_twin, "lisennet: catch_up + two live hops vs the twin")
    _assert_state_close(eng, 1, pool.export([a]).view(-1), twin, "lisennet: state after catch_up + two live hops")


def test_enhance_stream_in_chunks_runs_lisennet_on_the_pipeline_when_asked():
    from fastenhancer_amd.streaming import enhance_stream
    m = _cached("lisennet")[0]
    N, H = m.cfg.n_fft, m.cfg.hop_size
    length = 12 * H - (N - H)                                                     # 12 hops: chunks of 8 and 4
    wav = torch.from_numpy(make_input(1, length, 21, 16000)).to(_dev())
    y_loop = enhance_stream(m, wav)
    y_walk = enhance_stream(m, wav, chunk_hops=8)
    assert "time-pipelined" not in m.engine.last_step_kernel()                    # (the default setting: the walk)
    try:
        m.engine.set_time_pipeline(4)
        y_chunks = enhance_stream(m, wav, chunk_hops=8)
        assert _piped(m.engine.last_step_kernel()), m.engine.last_step_kernel()
    finally:
        m.engine.set_time_pipeline(-1)
    assert y_chunks.shape == y_loop.shape == wav.shape
    _assert_pipe_close(y_walk, y_loop, "lisennet enhance_stream(chunk_hops=8) at the default setting vs the hop loop")
    _assert_pipe_close(y_chunks, y_loop, "lisennet enhance_stream(chunk_hops=8) under width 4 vs the hop loop")
