"""CPU tests of the time-pipelined streaming chunk (fe_step_chunk, fe_step_chunk_work_floats, Engine.step_chunk / chunk_work_floats,
StreamPool.catch_up): argument checks that come before any device work, the work-buffer size contract, and the pool's export -> step ->
import order with the engine calls stubbed."""
from ctypes import c_void_p

import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import StreamPool

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)


def _err():
    return _lib.load().fe_last_error().decode()


def test_step_chunk_refuses_a_null_handle():
    lib = _lib.load()
    assert lib.fe_step_chunk(NULL, P, 256 * 8, P, P, 256 * 8, 1, 8, P, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()
    assert lib.fe_step_chunk_work_floats(NULL, 1, 8) == 0


def test_step_chunk_checks_its_arguments_as_fe_step_does():
    eng = Engine(product_config("fe_b"), None)
    lib, H = eng.lib, eng.cfg.hop_size
    row = 8 * H
    for args in [(NULL, row, P, P, row, 2, 8), (P, row, NULL, P, row, 2, 8), (P, row, P, NULL, row, 2, 8),
                 (P, row, P, P, row, 0, 8), (P, row, P, P, row, -1, 8), (P, row, P, P, row, 2, 0), (P, row, P, P, row, 2, -3)]:
        assert lib.fe_step_chunk(eng._h, *args, P, NULL) == FE_ERR_INVALID_ARG, args
        assert "bad argument" in _err()
    assert lib.fe_step_chunk(eng._h, P, row - 1, P, P, row, 2, 8, P, NULL) == FE_ERR_INVALID_ARG
    assert f"in_stride {row - 1} < T*H" in _err()
    assert lib.fe_step_chunk(eng._h, P, row, P, P, H, 2, 8, P, NULL) == FE_ERR_INVALID_ARG
    assert f"out_stride {H} < T*H" in _err()


def test_step_chunk_refuses_the_noncausal_model_as_fe_step_does():
    eng = Engine(product_config("fe_nc"), None)
    H = eng.cfg.hop_size
    assert eng.lib.fe_step_chunk(eng._h, P, 8 * H, P, P, 8 * H, 1, 8, P, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()
    assert eng.chunk_work_floats(1, 8) == 0


def test_chunk_work_floats_is_zero_where_nothing_is_pipelined():
    eng = Engine(product_config("fe_b"), None)
    for B, T in [(1, 1), (1, 3), (4, 3), (0, 8), (-1, 8), (1, 0)]:
        assert eng.chunk_work_floats(B, T) == 0, (B, T)
    bs = Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xxt"][0]), None)
    assert bs.chunk_work_floats(2, 5) == 0 and bs.chunk_work_floats(1, 251) == 0


def test_chunk_work_floats_is_positive_and_monotone():
    eng = Engine(product_config("fe_b"), None)
    N = eng.cfg.n_fft
    prev_row = None
    for B in (1, 2, 3, 8, 129, 300):                # (also above the streams the pipeline takes: one size for every setting)
        row = [eng.chunk_work_floats(B, T) for T in (4, 5, 13, 40, 251)]
        assert all(v > 0 for v in row)
        assert all(a < b for a, b in zip(row, row[1:])), (B, row)
        assert all(v >= B * T * N for v, T in zip(row, (4, 5, 13, 40, 251)))        # the windowed frames [B][T][N] at least
        if prev_row is not None:
            assert all(a < b for a, b in zip(prev_row, row)), (B, prev_row, row)
        prev_row = row
    before = eng.chunk_work_floats(3, 40)
    for setting in (0, 1, 4, 64, -1):               # the size does not follow fe_set_time_pipeline
        eng.set_time_pipeline(setting)
        assert eng.chunk_work_floats(3, 40) == before


@pytest.mark.parametrize("name", ["fe_tk_b", "fe_dpt_t"])
def test_chunk_work_floats_holds_the_rings_of_the_ring_variants(name):
    """time_kernel / dptransformer: the frames in flight hand their conv inputs / K-V through rings of L + P slots in the work buffer - even
    the narrowest pipeline (P = 2) needs that many floats beyond what a default model of the same n_fft needs"""
    eng, ref = Engine(product_config(name), None), Engine(product_config("fe_b"), None)
    c = eng.cfg
    assert c.n_fft == ref.cfg.n_fft
    for B, T in [(1, 4), (3, 13), (2, 40)]:
        if c.dpt:
            ring = 2 * c.rf_blocks * B * c.rf_freq * c.rf_channels * (c.lookbehind + 2)
        else:
            ring = 2 * c.n_layers * B * (c.kernel_size_time - 1 + 2) * c.F1 * c.channels
        assert ring > 0
        assert eng.chunk_work_floats(B, T) >= ref.chunk_work_floats(B, T) + ring, (B, T)


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
def test_step_chunk_checks_shapes_before_any_native_call(monkeypatch, wav_in, kw, match):
    eng = Engine(product_config("fe_b"), None)
    _no_native(monkeypatch, eng)
    kw = dict(kw)
    state = kw.pop("state", torch.zeros(1))
    with pytest.raises(ValueError, match=match):
        eng.step_chunk(wav_in, state, **kw)


def test_step_chunk_needs_a_gpu_after_the_host_checks(monkeypatch):
    eng = Engine(product_config("fe_b"), None)
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        eng.step_chunk(torch.zeros(1, 256 * 8), torch.zeros(eng.state_floats(1)))
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        eng.step_chunk(torch.zeros(3, 256 * 8), torch.zeros(eng.state_floats(3)), wav_out=torch.zeros(3, 256 * 8), T=8, work=torch.zeros(16))
    _no_native(monkeypatch, eng)                    # ... and a bad shape is reported first, without the library
    with pytest.raises(ValueError, match="wav_in"):
        eng.step_chunk(torch.zeros(1, 100), torch.zeros(1))


class _StubEngine:
    """what StreamPool.catch_up needs of an Engine, recorded instead of run"""
    def __init__(self):
        self.calls = []
        self.record = torch.arange(6, dtype=torch.float32).view(1, 6)

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        self.calls.append(("reset", capacity, list(slots)))

    def export_slots(self, state, capacity, slots, out=None):
        self.calls.append(("export", capacity, list(slots)))
        return self.record

    def step_chunk(self, wav_in, state, wav_out=None, T=None, work=None):
        self.calls.append(("step_chunk", tuple(wav_in.shape), state.data_ptr(), tuple(state.shape), T))
        state += 1.0                                # (the step updates the record in place)
        return wav_in * 2.0

    def import_slots(self, state, capacity, slots, records):
        self.calls.append(("import", capacity, list(slots), records.clone()))


def test_stream_pool_catch_up_exports_steps_and_imports_in_that_order():
    eng = _StubEngine()
    pool = StreamPool(eng, 4)
    a, b = pool.open(), pool.open()
    del eng.calls[:]
    x = torch.ones(5 * 4)
    y = pool.catch_up(b, x, 5)
    assert [c[0] for c in eng.calls] == ["export", "step_chunk", "import"]
    assert eng.calls[0] == ("export", 4, [b])
    assert eng.calls[1] == ("step_chunk", (1, 20), eng.record.data_ptr(), (6,), 5)       # one stream, stepped on the record itself
    assert eng.calls[2][:3] == ("import", 4, [b])
    assert torch.equal(eng.calls[2][3], torch.arange(6, dtype=torch.float32).view(1, 6) + 1.0)      # ... and the stepped record goes back
    assert tuple(y.shape) == (1, 20) and torch.equal(y, torch.full((1, 20), 2.0))
    assert a in pool.active and b in pool.active


def test_stream_pool_catch_up_refuses_a_slot_that_is_not_open_before_any_engine_call():
    eng = _StubEngine()
    pool = StreamPool(eng, 3)
    a = pool.open()
    pool.close(a)
    del eng.calls[:]
    for slot in (a, 2, 7, -1):
        with pytest.raises(ValueError, match="not open"):
            pool.catch_up(slot, torch.zeros(1, 8), 2)
    assert eng.calls == []
    b = pool.open()
    del eng.calls[:]
    with pytest.raises(ValueError, match="ONE stream"):
        pool.catch_up(b, torch.zeros(2, 8), 2)
    assert eng.calls == []
