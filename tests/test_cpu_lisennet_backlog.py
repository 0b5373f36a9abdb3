"""CPU tests of LiSenNet's opt-in time pipeline under fe_step_backlog (fe_lisennet_backlog_work_floats, Engine.lisennet_backlog_work_floats /
lisennet_backlog_work, and which call enhance_stream(chunk_hops=...) and StreamPool.catch_up make for the family): the declaration, the
size contract of the new query, fe_step_backlog_work_floats staying 0, and the callers' choice with the engine calls recorded, not run."""
import re
from ctypes import c_int, c_size_t, c_void_p
from pathlib import Path

import pytest
import torch

from common import hip_engine, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.family import chunk_step
from fastenhancer_amd.serving import StreamPool
from fastenhancer_amd.streaming import enhance_stream

NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
TS = (4, 5, 13, 40, 251)
BS = (1, 2, 3, 8, 129)
CACHE_FLOATS = 257 + 4 * 257 + 8 * 128 + 12 * 64 + 2 * (32 * 24 + 2 * 16 * 2 * 32) + 4 * 256      # the nine caches of one stream
RING_SLOTS = 64 + 2                                                                             # the widest pipeline and two more


def test_the_header_declares_the_query_and_the_binding_types_it():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bsize_t\s+fe_lisennet_backlog_work_floats\s*\(([^)]*)\)\s*;", text)
    assert m and " ".join(m.group(1).split()) == "const fe_handle* h, int B, int T"
    assert _lib.SYMBOLS["fe_lisennet_backlog_work_floats"] == (c_size_t, [c_void_p, c_int, c_int])
    assert _lib.SYMBOLS["fe_lisennet_backlog_work_floats"] == _lib.SYMBOLS["fe_step_backlog_work_floats"]
    lib = _lib.load()
    assert lib.fe_lisennet_backlog_work_floats.restype == c_size_t and lib.fe_lisennet_backlog_work_floats.argtypes == [c_void_p, c_int, c_int]


def test_the_query_is_zero_where_the_pipeline_takes_nothing():
    lib = _lib.load()
    assert lib.fe_lisennet_backlog_work_floats(NULL, 1, 8) == 0
    for name in ("bsrnn_xxt", "fspen", "fe_b"):
        eng = hip_engine(name)
        for B in BS:
            for T in (1, 3) + TS:
                assert eng.lisennet_backlog_work_floats(B, T) == 0, (name, B, T)
    ls = hip_engine("lisennet")
    for B, T in [(0, 8), (-1, 8), (1, 0), (1, 1), (1, 3), (4, 3), (129, 3), (1, -2)]:
        assert ls.lisennet_backlog_work_floats(B, T) == 0, (B, T)


def test_the_query_is_counters_frames_and_rings_whatever_the_setting():
    ls = hip_engine("lisennet")
    N = ls.cfg.n_fft
    for B in BS:
        row = [ls.lisennet_backlog_work_floats(B, T) for T in TS]
        for T, v in zip(TS, row):
            assert v >= B * T * N, (B, T, v)                                   # the windowed frames at least
            assert v == (9 * B + 3) // 4 * 4 + B * T * N + B * RING_SLOTS * CACHE_FLOATS, (B, T, v)
        assert all(a < b for a, b in zip(row, row[1:])), (B, row)
    before = ls.lisennet_backlog_work_floats(3, 13)
    try:
        for setting in (0, 1, 2, 8, 64, -1):                                   # the size does not follow fe_set_time_pipeline
            ls.set_time_pipeline(setting)
            assert ls.lisennet_backlog_work_floats(3, 13) == before
            for B in BS:                                                       # ... and the family's general query stays 0 at every setting
                for T in (1, 3) + TS:
                    assert ls.backlog_work_floats(B, T) == 0, (setting, B, T)
    finally:
        ls.set_time_pipeline(-1)


class _StubEngine:
    """what enhance_stream(chunk_hops=...) and StreamPool.catch_up need of a LiSenNet Engine, recorded instead of run"""
    def __init__(self, cfg, width=None):
        self.cfg = cfg
        self.device = torch.device("cpu")
        self.calls = []
        self.record = torch.arange(6, dtype=torch.float32).view(1, 6)
        if width is not None:
            self._time_pipeline = width

    def new_state(self, B):
        return torch.zeros(B)

    def export_slots(self, state, capacity, slots, out=None):
        return self.record

    def import_slots(self, state, capacity, slots, records):
        pass

    def lisennet_backlog_work(self, B, T):
        self.calls.append(("work", B, T))
        return torch.zeros(B * T) if T >= 4 else None

    def step_chunk(self, wav_in, state, wav_out=None, T=None, work=None):
        self.calls.append(("step_chunk", tuple(wav_in.shape), T, work))
        return wav_in if wav_out is None else wav_out.copy_(wav_in)

    def step_backlog(self, wav_in, state, wav_out=None, T=None, work=None):
        self.calls.append(("step_backlog", tuple(wav_in.shape), T, None if work is None else work.numel()))
        return wav_in if wav_out is None else wav_out.copy_(wav_in)


class _StubModel:
    def __init__(self, cfg, width):
        self.cfg, self.engine = cfg, _StubEngine(cfg, width)


@pytest.mark.parametrize("width", [None, -1, 0, 1])
def test_without_an_explicit_width_the_callers_make_the_call_they_always_made(width):
    cfg = product_config("lisennet")
    eng = _StubEngine(cfg, width)
    assert chunk_step(eng) == eng.step_chunk
    m = _StubModel(cfg, width)
    enhance_stream(m, 0.1 * torch.ones(1, 9 * cfg.hop_size), chunk_hops=8)
    assert [c[0] for c in m.engine.calls] == ["step_chunk", "step_chunk"]
    real = hip_engine("lisennet")
    real.set_time_pipeline(-1)
    assert chunk_step(real) == real.step_chunk and real.lisennet_backlog_work(1, 8) is None


@pytest.mark.parametrize("width", [2, 8])
def test_under_an_explicit_width_the_callers_size_and_pass_the_work_buffer(width):
    cfg = product_config("lisennet")
    H = cfg.hop_size
    m = _StubModel(cfg, width)
    enhance_stream(m, 0.1 * torch.ones(1, 9 * H), chunk_hops=8)             # 10 hops: chunks of 8 and 2
    assert m.engine.calls == [("work", 1, 8), ("step_backlog", (1, 8 * H), 8, 8), ("work", 1, 2), ("step_backlog", (1, 2 * H), 2, None)]
    eng = _StubEngine(cfg, width)
    pool = StreamPool.__new__(StreamPool)
    pool.engine, pool.capacity, pool.state, pool._open = eng, 2, torch.zeros(2), {1}
    pool.catch_up(1, torch.ones(5 * H))                                     # (T from the length)
    assert eng.calls == [("work", 1, 5), ("step_backlog", (1, 5 * H), None, 5)]


def test_the_engine_hands_out_its_scratch_only_under_an_explicit_width(monkeypatch):
    ls = hip_engine("lisennet")
    made = []
    monkeypatch.setattr(torch, "empty", lambda n, **kw: made.append(n) or torch.zeros(n))
    try:
        for width in (-1, 0, 1):
            ls.set_time_pipeline(width)
            assert ls.lisennet_backlog_work(2, 8) is None
        ls.set_time_pipeline(4)
        assert ls.lisennet_backlog_work(2, 3) is None                          # T < 4: the call walks
        w = ls.lisennet_backlog_work(2, 8)
        assert w is not None and w.numel() == ls.lisennet_backlog_work_floats(2, 8) and made == [w.numel()]
        assert ls.lisennet_backlog_work(1, 8) is w and len(made) == 1        # grow-only
    finally:
        ls.set_time_pipeline(-1)
        ls._chunk_work = None
    assert hip_engine("bsrnn_xxt").lisennet_backlog_work(2, 8) is None
