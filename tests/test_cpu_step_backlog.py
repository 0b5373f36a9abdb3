"""CPU tests of fe_step_backlog - fe_step for few streams and many hops, for every family with a streaming state (fe_step_backlog,
fe_step_backlog_work_floats, Engine.step_backlog / backlog_work_floats, and which of step_chunk / step_backlog enhance_stream(chunk_hops=...)
and StreamPool.catch_up call): the declarations, the work-buffer size contract, the argument checks that come before any device work, and
the callers' choice with the engine calls recorded instead of run."""
import re
from ctypes import c_void_p
from pathlib import Path

import pytest
import torch

from common import hip_engine, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import StreamPool
from fastenhancer_amd.streaming import enhance_stream

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
TS = (4, 5, 13, 40, 251)
BS = (1, 2, 3, 8, 129, 300)


def _err():
    return _lib.load().fe_last_error().decode()


def test_the_header_declares_both_functions_and_the_binding_types_them_like_fe_step_chunk():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(fe_step_(?:backlog|chunk)(?:_work_floats)?)\s*\(([^)]*)\)\s*;", text)}
    assert set(decls) == {"fe_step_chunk", "fe_step_chunk_work_floats", "fe_step_backlog", "fe_step_backlog_work_floats"}
    assert decls["fe_step_backlog"] == decls["fe_step_chunk"]                        # the same parameter list, word for word
    assert decls["fe_step_backlog_work_floats"] == decls["fe_step_chunk_work_floats"]
    assert re.search(r"\bsize_t\s+fe_step_backlog_work_floats\s*\(", text) and re.search(r"\bint\s+fe_step_backlog\s*\(", text)
    assert _lib.SYMBOLS["fe_step_backlog"] == _lib.SYMBOLS["fe_step_chunk"]
    assert _lib.SYMBOLS["fe_step_backlog_work_floats"] == _lib.SYMBOLS["fe_step_chunk_work_floats"]
    lib = _lib.load()
    assert lib.fe_step_backlog.argtypes == lib.fe_step_chunk.argtypes and lib.fe_step_backlog.restype == lib.fe_step_chunk.restype


def test_backlog_work_floats_is_zero_where_nothing_is_pipelined():
    lib = _lib.load()
    assert lib.fe_step_backlog_work_floats(NULL, 1, 8) == 0
    for name in ("bsrnn_xxt", "fspen", "fe_b"):
        eng = hip_engine(name)
        for B, T in [(0, 8), (-1, 8), (1, 0), (1, 1), (1, 3), (4, 3), (300, 3)]:
            assert eng.backlog_work_floats(B, T) == 0, (name, B, T)
    ls = hip_engine("lisennet")
    for B in BS:
        for T in (1, 3) + TS:
            assert ls.backlog_work_floats(B, T) == 0, (B, T)


@pytest.mark.parametrize("name", ["bsrnn_xxt", "bsrnn_s", "fspen"])
def test_backlog_work_floats_is_positive_and_monotone(name):
    eng = hip_engine(name)
    N = eng.cfg.n_fft
    prev_row = None
    for B in BS:                                    # (also above the streams the pipeline takes: one size for every setting)
        row = [eng.backlog_work_floats(B, T) for T in TS]
        assert all(v > 0 for v in row), (B, row)
        assert all(a < b for a, b in zip(row, row[1:])), (B, row)
        assert all(v >= B * T * N for v, T in zip(row, TS)), (B, row)          # the windowed frames [B][T][N] at least
        if prev_row is not None:
            assert all(a <= b for a, b in zip(prev_row, row)), (B, prev_row, row)
        prev_row = row
    before = eng.backlog_work_floats(3, 40)
    for setting in (0, 1, 4, 64, -1):               # the size does not follow fe_set_time_pipeline
        eng.set_time_pipeline(setting)
        assert eng.backlog_work_floats(3, 40) == before
    assert eng.chunk_work_floats(3, 40) == 0        # fe_step_chunk keeps its contract for the family


def test_fastenhancer_backlog_work_floats_is_the_chunk_query():
    eng = hip_engine("fe_b")
    for B in BS:
        for T in (1, 3) + TS:
            assert eng.backlog_work_floats(B, T) == eng.chunk_work_floats(B, T), (B, T)


def test_step_backlog_refuses_a_null_handle():
    lib = _lib.load()
    assert lib.fe_step_backlog(NULL, P, 256 * 8, P, P, 256 * 8, 1, 8, P, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("name", ["fe_b", "bsrnn_xxt", "fspen", "lisennet"])
def test_step_backlog_checks_its_arguments_as_fe_step_does(name):
    eng = hip_engine(name)
    lib, H = eng.lib, eng.cfg.hop_size
    row = 8 * H
    for args in [(NULL, row, P, P, row, 2, 8), (P, row, NULL, P, row, 2, 8), (P, row, P, NULL, row, 2, 8),
                 (P, row, P, P, row, 0, 8), (P, row, P, P, row, -1, 8), (P, row, P, P, row, 2, 0), (P, row, P, P, row, 2, -3)]:
        assert lib.fe_step_backlog(eng._h, *args, P, NULL) == FE_ERR_INVALID_ARG, args
        assert "bad argument" in _err()
    assert lib.fe_step_backlog(eng._h, P, row - 1, P, P, row, 2, 8, P, NULL) == FE_ERR_INVALID_ARG
    assert f"in_stride {row - 1} < T*H" in _err()
    assert lib.fe_step_backlog(eng._h, P, row, P, P, H, 2, 8, P, NULL) == FE_ERR_INVALID_ARG
    assert f"out_stride {H} < T*H" in _err()


@pytest.mark.parametrize("name", ["bsrnn_xxt", "bsrnn_s", "fspen"])
def test_step_backlog_refuses_a_null_work_buffer_before_any_device_work(name):
    eng = hip_engine(name)
    H = eng.cfg.hop_size
    for B, T in [(1, 4), (2, 8), (3, 40)]:
        assert eng.lib.fe_step_backlog(eng._h, P, T * H, P, P, T * H, B, T, NULL, NULL) == FE_ERR_INVALID_ARG
        assert f"fe_step_backlog: null work buffer (fe_step_backlog_work_floats(h, {B}, {T}) floats)" in _err()


def test_step_backlog_refuses_the_noncausal_model_as_fe_step_does():
    eng = hip_engine("fe_nc")
    H = eng.cfg.hop_size
    assert eng.lib.fe_step_backlog(eng._h, P, 8 * H, P, P, 8 * H, 1, 8, P, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()
    assert eng.backlog_work_floats(1, 8) == 0


def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


@pytest.mark.parametrize("wav_in,kw,match", [
    (torch.zeros(256 * 4), {}, "wav_in"),                                  # not 2-D
    (torch.zeros(2, 256 * 4, dtype=torch.float64), {}, "wav_in"),
    (torch.zeros(2, 256 * 4 + 1), {}, "wav_in"),                           # not a whole number of hops
    (torch.zeros(2, 256 * 4), {"T": 3}, "wav_in"),                         # T does not match the rows
    (torch.zeros(2, 256 * 4), {"T": 0}, "wav_in"),
    (torch.zeros(2, 128), {}, "wav_in"),                                   # shorter than a hop: T = 0
    (torch.zeros(0, 256 * 4), {}, "wav_in"),
    (torch.zeros(2, 256 * 8)[:, ::2], {}, "wav_in"),                       # samples not contiguous
    (torch.zeros(2, 256 * 4), {"wav_out": torch.zeros(2, 256 * 3)}, "wav_out"),
    (torch.zeros(2, 256 * 4), {"wav_out": torch.zeros(2, 256 * 4, dtype=torch.float64)}, "wav_out"),
    (torch.zeros(2, 256 * 4), {"state": torch.zeros(4, 4)}, "state"),
    (torch.zeros(2, 256 * 4), {"state": torch.zeros(8, dtype=torch.int32)}, "state"),
    (torch.zeros(2, 256 * 4), {"work": torch.zeros(8, dtype=torch.float64)}, "work"),
])
def test_step_backlog_checks_shapes_before_any_native_call(monkeypatch, wav_in, kw, match):
    eng = hip_engine("bsrnn_xxt")
    assert eng.cfg.hop_size == 256
    _no_native(monkeypatch, eng)
    kw = dict(kw)
    state = kw.pop("state", torch.zeros(1))
    with pytest.raises(ValueError, match=match):
        eng.step_backlog(wav_in, state, **kw)


def test_step_backlog_needs_a_gpu_after_the_host_checks(monkeypatch):
    eng = hip_engine("fspen")
    H = eng.cfg.hop_size
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        eng.step_backlog(torch.zeros(1, H * 8), torch.zeros(eng.state_floats(1)))
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        eng.step_backlog(torch.zeros(3, H * 8), torch.zeros(eng.state_floats(3)), wav_out=torch.zeros(3, H * 8), T=8, work=torch.zeros(16))
    _no_native(monkeypatch, eng)                    # ... and a bad shape is reported first, without the library
    with pytest.raises(ValueError, match="wav_in"):
        eng.step_backlog(torch.zeros(1, H // 2), torch.zeros(1))


class _StubEngine:
    """what enhance_stream(chunk_hops=...) and StreamPool.catch_up need of an Engine, recorded instead of run"""
    def __init__(self, cfg):
        self.cfg = cfg
        self.device = torch.device("cpu")
        self.calls = []
        self.record = torch.arange(6, dtype=torch.float32).view(1, 6)

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        self.calls.append(("reset", capacity, list(slots)))

    def export_slots(self, state, capacity, slots, out=None):
        self.calls.append(("export", capacity, list(slots)))
        return self.record

    def import_slots(self, state, capacity, slots, records):
        self.calls.append(("import", capacity, list(slots)))

    def step_chunk(self, wav_in, state, wav_out=None, T=None, work=None):
        self.calls.append(("step_chunk", tuple(wav_in.shape), T))
        if wav_out is None:
            return wav_in * 2.0
        wav_out.copy_(wav_in * 2.0)
        return wav_out

    def step_backlog(self, wav_in, state, wav_out=None, T=None, work=None):
        self.calls.append(("step_backlog", tuple(wav_in.shape), T))
        if wav_out is None:
            return wav_in * 3.0
        wav_out.copy_(wav_in * 3.0)
        return wav_out


class _StubModel:
    def __init__(self, cfg):
        self.cfg, self.engine = cfg, _StubEngine(cfg)


@pytest.mark.parametrize("name,call,gain", [("bsrnn_xxt", "step_backlog", 3.0), ("fspen", "step_backlog", 3.0), ("fe_b", "step_chunk", 2.0)])
def test_enhance_stream_in_chunks_calls_the_familys_entry_point(name, call, gain):
    m = _StubModel(product_config(name))
    N, H = m.cfg.n_fft, m.cfg.hop_size
    wav = 0.1 * torch.ones(1, 20 * H)
    y = enhance_stream(m, wav, chunk_hops=8)
    n_hops = len(range(0, 20 * H + N - H, H))
    sizes = [8] * (n_hops // 8) + ([n_hops % 8] if n_hops % 8 else [])
    assert m.engine.calls == [(call, (1, T * H), T) for T in sizes]
    assert y.shape == wav.shape and torch.allclose(y[:, :20 * H - (N - H)], torch.full((1, 20 * H - (N - H)), 0.1 * gain))


@pytest.mark.parametrize("name,call,gain", [("bsrnn_xxt", "step_backlog", 3.0), ("fspen", "step_backlog", 3.0), ("fe_b", "step_chunk", 2.0)])
def test_stream_pool_catch_up_calls_the_familys_entry_point(name, call, gain):
    eng = _StubEngine(product_config(name))
    pool = StreamPool(eng, 4)
    a, b = pool.open(), pool.open()
    assert eng.calls == [("reset", 4, [a]), ("reset", 4, [b])]          # (a stand-in without a family description: reset_slots)
    del eng.calls[:]
    y = pool.catch_up(b, torch.ones(5 * 4), 5)
    assert eng.calls == [("export", 4, [b]), (call, (1, 20), 5), ("import", 4, [b])]
    assert torch.equal(y, torch.full((1, 20), gain))


def test_a_pool_of_a_baseline_family_opens_a_slot_with_a_zero_record(monkeypatch):
    """fe_state_reset_slots is the FastEnhancer family's: a BSRNN / FSPEN / LiSenNet pool imports a zero record instead (the state records
    are built for every family), a FastEnhancer pool resets as it always has"""
    for name, first in [("fspen", "import"), ("bsrnn_xxt", "import"), ("lisennet", "import"), ("fe_b", "reset")]:
        eng = hip_engine(name)
        calls = []
        monkeypatch.setattr(Engine, "new_state", lambda self, B: torch.zeros(self.state_floats(B)))
        monkeypatch.setattr(Engine, "reset_slots", lambda self, state, capacity, slots: calls.append(("reset", capacity, list(slots))))
        monkeypatch.setattr(Engine, "import_slots", lambda self, state, capacity, slots, records: calls.append(
            ("import", capacity, list(slots), tuple(records.shape), float(records.abs().max()))))
        pool = StreamPool(eng, 2)
        s = pool.open()
        assert calls == ([("import", 2, [s], (1, eng.record_floats), 0.0)] if first == "import" else [("reset", 2, [s])]), (name, calls)
