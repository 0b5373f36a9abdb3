"""Every work-buffer size query covers what its call writes (fe_offline, fe_step_chunk, fe_step_streams_chunk, fe_offline_ragged).

The C ABI is called through ctypes directly, as tests/test_c_abi_errors.py does.  The work buffer of exactly the queried size sits inside a
larger allocation, FRONT sentinel floats before it and BACK behind it; after a stream synchronise both sentinel regions must be
bit-identical to before, and every output (and the state, where the call has one) must be bit-equal to the same call made with a
generously oversized work buffer.  Both work buffers start from the same fill, so a read of a float the call has not written shows too.

Every case asserts what fe_last_step_kernel reports - a time-pipelined kernel (the ragged case: the time-batched engine's) - so that a
refused or unpipelined call fails instead of passing vacuously.  The shapes are the smallest that reach each term of a layout: two streams,
6 frames (above the pipeline's 4), and 70 frames at fe_set_time_pipeline(64), the widest ring the buffers are sized for."""
import functools
from ctypes import c_int, c_void_p

import pytest
import torch

from common import product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.family import family_of

pytestmark = pytest.mark.gpu

FRONT, BACK = 1024, 4096
FILL = 7.0
NULL = c_void_p(0)


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _engine(name):
    cfg = product_config(name)
    eng = Engine(cfg, _dev())
    eng.load_state_dict(family_of(cfg).default_state_dict(cfg, torch.Generator().manual_seed(5)))
    if hasattr(cfg, "rf_blocks"):       # FastEnhancer: the frame walk and its time pipeline, not the time-batched engine
        eng.set_offline_engine("frame_walk")
    return eng


def _p(t):
    return c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Guarded:
    """`n` work floats between two sentinel regions"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((FRONT + n + BACK,), FILL, device=_dev())
        self.pattern = torch.arange(FRONT + BACK, dtype=torch.float32, device=_dev()) * 0.5 - 77.0
        self.buf[:FRONT] = self.pattern[:FRONT]
        self.buf[FRONT + n:] = self.pattern[FRONT:]
        self.work = self.buf[FRONT:FRONT + n]

    def check(self, what):
        assert torch.equal(_bits(self.buf[:FRONT]), _bits(self.pattern[:FRONT])), f"{what}: floats in front of the work buffer were written"
        assert torch.equal(_bits(self.buf[FRONT + self.n:]), _bits(self.pattern[FRONT:])), f"{what}: floats behind the work buffer's {self.n} were written"


def _tight_and_roomy(need, call, what):
    """call(work) -> tensors; once on exactly `need` floats between sentinels, once on a buffer with plenty of room"""
    assert need > 0, what
    g = _Guarded(need)
    got = call(g.work)
    torch.cuda.synchronize()
    g.check(what)
    roomy = torch.full((2 * need + 65536,), FILL, device=_dev())
    ref = call(roomy)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: output {i} differs from the call with an oversized work buffer"
        assert torch.isfinite(a).all(), f"{what}: output {i}"


def _offline(name, frames, width):
    eng, lib = _engine(name), _lib.load()
    cfg, h, B = eng.cfg, eng._h, 2
    H = cfg.hop_size
    Tw = (frames - 1) * H + 7
    T = 1 + Tw // H
    assert T == frames
    x = 0.1 * torch.randn(B, Tw, generator=torch.Generator().manual_seed(3)).to(_dev())
    eng.set_time_pipeline(width)
    try:
        need = int(lib.fe_offline_work_floats(h, B, Tw))

        def call(work):
            wav = torch.full((B, H * (T - 1)), FILL, device=_dev())
            spec = torch.full((B, eng.family.spec_bins(cfg), T, 2), FILL, device=_dev())
            assert lib.fe_offline(h, _p(x), B, Tw, _p(wav), _p(spec), _p(work), _stream()) == 0, lib.fe_last_error()
            k = eng.last_step_kernel()
            assert "time-pipelined" in k and "istft_ola_kernel" in k, k
            return wav, spec

        _tight_and_roomy(need, call, f"fe_offline {name} {B} x {frames} frames, pipeline {width}")
    finally:
        eng.set_time_pipeline(-1)


@pytest.mark.parametrize("name", ["fe_b", "fe_tk_b", "fe_dpt_b", "bsrnn_xt", "fspen", "lisennet"])
def test_offline_work_floats_cover_the_pipelined_call(name):
    _offline(name, 6, -1)


@pytest.mark.parametrize("name", ["fe_tk_b", "fe_dpt_b", "lisennet"])
def test_offline_work_floats_cover_the_widest_ring(name):
    _offline(name, 70, 64)


@pytest.mark.parametrize("name,T,width", [("fe_tk_b", 70, 64), ("fe_dpt_b", 70, 64), ("fe_b", 6, -1)])
def test_step_chunk_work_floats_cover_the_call(name, T, width):
    eng, lib = _engine(name), _lib.load()
    h, B, H = eng._h, 2, eng.cfg.hop_size
    g = torch.Generator().manual_seed(4)
    state0 = eng.new_state(B)
    eng.step(0.1 * torch.randn(B, 2 * H, generator=g).to(_dev()), state0, T=2)       # a state that is not all zeros
    x = 0.1 * torch.randn(B, T * H, generator=g).to(_dev())
    eng.set_time_pipeline(width)
    try:
        need = int(lib.fe_step_chunk_work_floats(h, B, T))

        def call(work):
            st, y = state0.clone(), torch.full((B, T * H), FILL, device=_dev())
            assert lib.fe_step_chunk(h, _p(x), T * H, _p(st), _p(y), T * H, B, T, _p(work), _stream()) == 0, lib.fe_last_error()
            k = eng.last_step_kernel()
            assert "time-pipelined" in k and "stream_ola_kernel" in k, k
            return y, st

        _tight_and_roomy(need, call, f"fe_step_chunk {name} {B} x {T} hops, pipeline {width}")
    finally:
        eng.set_time_pipeline(-1)


def test_step_streams_chunk_work_floats_cover_the_call():
    eng, lib = _engine("fe_b"), _lib.load()
    h, H, n, cap, T_max = eng._h, eng.cfg.hop_size, 2, 3, 6
    g = torch.Generator().manual_seed(6)
    state0 = eng.new_state(cap)
    eng.step(0.1 * torch.randn(cap, 2 * H, generator=g).to(_dev()), state0, T=2)
    count = n * T_max * H
    x = 0.1 * torch.randn(count, generator=g).to(_dev())
    desc = Engine.pack_stream_desc([(2, 6, 0, 0), (0, 3, T_max * H, T_max * H)]).to(_dev())
    need = int(lib.fe_step_streams_chunk_work_floats(h, n, T_max))

    def call(work):
        st, y = state0.clone(), torch.full((count,), FILL, device=_dev())
        rc = lib.fe_step_streams_chunk(h, _p(x), count, _p(st), cap, _p(desc), _p(y), count, n, T_max, _lib.FE_AUDIO_F32, NULL, NULL, NULL, _p(work), _stream())
        assert rc == 0, lib.fe_last_error()
        k = eng.last_step_kernel()
        assert "time-pipelined" in k and "stream_ola_streams_kernel" in k, k
        return y, st

    _tight_and_roomy(need, call, f"fe_step_streams_chunk fe_b, hops (6, 3) of {T_max}")


def test_offline_ragged_work_floats_cover_the_batched_call():
    """the time-batched engine's layout with the utterance lengths behind it (the one batched form of a ragged call)"""
    cfg = product_config("fe_b")
    eng, lib = Engine(cfg, _dev()), _lib.load()       # (its own engine: the automatic offline engine, which batches a ragged call)
    eng.load_state_dict(family_of(cfg).default_state_dict(cfg, torch.Generator().manual_seed(5)))
    h, B, H = eng._h, 2, cfg.hop_size
    lens = [5 * H + 7, 3 * H + 7]                       # 6 and 4 frames
    Tw = max(lens)
    T = 1 + Tw // H
    x = 0.1 * torch.randn(B, Tw, generator=torch.Generator().manual_seed(8)).to(_dev())
    need = int(lib.fe_offline_ragged_work_floats(h, B, Tw))
    n_out = H * (T - 1)

    def call(work):
        wav = torch.zeros(B, n_out, device=_dev())
        spec = torch.full((B, eng.family.spec_bins(cfg), T, 2), FILL, device=_dev())
        rc = lib.fe_offline_ragged(h, _p(x), Tw, (c_int * B)(*lens), B, _p(wav), n_out, _p(spec), _p(work), _stream())
        assert rc == 0, lib.fe_last_error()
        k = eng.last_step_kernel()
        assert k.startswith("tb_enc_kernel") and "istft_ola_kernel" in k, k
        Tb = [1 + n // H for n in lens]
        return [wav] + [spec[b, :, :Tb[b]] for b in range(B)]

    _tight_and_roomy(need, call, "fe_offline_ragged fe_b, 6 and 4 frames")
