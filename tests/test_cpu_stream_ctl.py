"""CPU tests of the packet step's per-stream controls (fe_step_streams_ctl / fe_step_streams_ctl_pinned, Engine.step_streams*(min_gain=, levels=),
serving.PacketPool.set_suppression_limit / levels): the ABI, the argument checks that come before any device work - those of fe_step_streams,
plus the alignment of the level table - and PacketPool's bookkeeping of limits and level rows with the engine call replaced by a stub."""
import ctypes
import math
import os
import re
from ctypes import c_void_p

import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool, StreamLevels

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastenhancer_hip.h")
FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
ENTRY_POINTS = ("fe_step_streams_ctl", "fe_step_streams_ctl_pinned")


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0, min_gain=P, levels=P):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, min_gain, levels, NULL)


def _call_plain(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, NULL)


# ------------------------------------------------------------------ the ABI
def test_both_entry_points_are_bound_with_the_two_tables_before_the_stream():
    lib = _lib.load()
    for fn in ENTRY_POINTS:
        assert fn in _lib.SYMBOLS and hasattr(lib, fn)
        restype, argtypes = _lib.SYMBOLS[fn]
        plain = _lib.SYMBOLS[fn.replace("_ctl", "")][1]
        assert restype is ctypes.c_int and argtypes == plain[:-1] + [c_void_p, c_void_p] + plain[-1:]


def test_stream_levels_of_the_header_is_the_ctypes_struct():
    src = open(HEADER).read()
    body = re.search(r"typedef struct fe_stream_levels \{(.*?)\} fe_stream_levels;", src, re.S).group(1)
    assert [n.strip() for n in body.replace("float", "").strip(" ;").split(",")] == ["in_sumsq", "in_peak", "out_sumsq", "out_peak"]
    assert [(n, t) for n, t in _lib.fe_stream_levels._fields_] == [(n, ctypes.c_float) for n in ("in_sumsq", "in_peak", "out_sumsq", "out_peak")]
    assert ctypes.sizeof(_lib.fe_stream_levels) == 16
    for fn in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % fn, src), fn


# ------------------------------------------------------------------ argument checks of the library (no GPU: they come first)
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_ctl_entry_points_refuse_a_null_handle(fn):
    lib = _lib.load()
    assert _call(lib, fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("tables", [dict(), dict(min_gain=NULL), dict(levels=NULL), dict(min_gain=NULL, levels=NULL)], ids=["both", "levels", "gain", "none"])
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_ctl_entry_points_give_the_argument_errors_of_the_plain_step(fn, tables):
    eng = Engine(product_config("fe_b"), None)
    plain = fn.replace("_ctl", "")
    bad = [dict(wav_in=NULL), dict(state=NULL), dict(desc=NULL), dict(wav_out=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0),
           dict(T_max=0), dict(T_max=-2), dict(in_count=0), dict(out_count=0), dict(fmt=2), dict(fmt=-1), dict(fmt=16)]
    for kw in bad:
        want = _call_plain(eng.lib, plain, eng._h, **kw)
        want_text = _err()
        assert want == FE_ERR_INVALID_ARG
        assert _call(eng.lib, fn, eng._h, **kw, **tables) == want, kw
        assert _err() == want_text.replace(plain + ":", fn + ":"), (kw, _err(), want_text)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_a_level_table_that_is_not_16_byte_aligned_is_refused(fn):
    eng = Engine(product_config("fe_b"), None)
    for off in (4, 8, 12, 1):
        assert _call(eng.lib, fn, eng._h, levels=c_void_p(0x1000 + off)) == FE_ERR_INVALID_ARG, off
        assert fn in _err() and "16-byte aligned" in _err(), _err()
    assert _call(eng.lib, fn, eng._h, min_gain=c_void_p(0x1004), levels=NULL) != FE_ERR_UNSUPPORTED_CONFIG       # (any float alignment for min_gain)
    assert "16-byte" not in _err()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_ctl_entry_points_refuse_the_baseline_families_and_the_noncausal_model(fn):
    eng = Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xt"][0]), None)
    assert _call(eng.lib, fn, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "FastEnhancer family" in _err() and fn in _err()
    nc = Engine(product_config("fe_nc"), None)
    assert _call(nc.lib, fn, nc._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()


def test_engine_checks_the_tables_before_any_device_call():
    for what, t, shape, match in [("min_gain", torch.zeros(7), (8,), r"min_gain must be a contiguous float32 tensor \[8\]"),
                                  ("min_gain", torch.zeros(8, dtype=torch.float64), (8,), "min_gain must be a contiguous float32"),
                                  ("min_gain", [0.0] * 8, (8,), "min_gain must be a contiguous float32"),
                                  ("levels", torch.zeros(8, 3), (8, 4), r"levels must be a contiguous float32 tensor \[8, 4\]"),
                                  ("levels", torch.zeros(4, 8).t(), (8, 4), "levels must be a contiguous float32"),
                                  ("min_gain", torch.zeros(8), (8,), "min_gain must be a device tensor or a CPU tensor in page-locked memory")]:
        with pytest.raises(ValueError, match=match):
            Engine._stream_table(what, t, shape)
    assert Engine._stream_table("levels", None, (8, 4)) is None


# ------------------------------------------------------------------ PacketPool with the engine stubbed
class _Cfg:
    hop_size = 256


class _StubEngine:
    """what PacketPool needs of an Engine: the launch copies the input hops to their output place and writes the level rows an identity
    model would meter; it records the tables it was handed"""
    cfg = _Cfg()

    def __init__(self):
        self.calls = []

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        pass

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        pass

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, **ctl):
        H = self.cfg.hop_size
        fin, fout = wav_in.view(-1), wav_out.view(-1)
        for slot, hops, i0, o0 in desc:
            fout[o0:o0 + hops * H] = fin[i0:i0 + hops * H]
            if ctl.get("levels") is not None:
                x = fin[i0:i0 + hops * H].double() / 32768.0
                ctl["levels"][slot] = torch.tensor([float((x * x).sum()), float(x.abs().max())] * 2)
        self.calls.append((list(desc), ctl.get("min_gain").clone() if ctl.get("min_gain") is not None else None, sorted(ctl)))
        return wav_out


def _pcm(n, seed):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3000).round().to(torch.int16)


def test_set_suppression_limit_validation_and_units():
    eng = _StubEngine()
    pool = PacketPool(eng, 4, ring_hops=4)
    a, b = pool.open(), pool.open()
    for bad in (0.5, 3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="at or below 0"):
            pool.set_suppression_limit(a, bad)
    with pytest.raises(ValueError, match="not open"):
        pool.set_suppression_limit(3, -20.0)
    assert pool.suppression_limit(a) is None and pool._gain is None
    pool.set_suppression_limit(a, None)
    pool.set_suppression_limit(a, -math.inf)
    assert pool._gain is None, "lifting a limit that was never set needs no table"
    pool.set_suppression_limit(a, -20.0)
    pool.set_suppression_limit(b, 0)
    assert pool._gain.dtype == torch.float32 and pool._gain.tolist() == [pytest.approx(0.1, rel=1e-7), 1.0, 0.0, 0.0]
    assert pool.suppression_limit(a) == pytest.approx(-20.0, abs=1e-5) and pool.suppression_limit(b) == 0.0
    pool.set_suppression_limit(a, -math.inf)
    assert pool.suppression_limit(a) is None and float(pool._gain[a]) == 0.0
    pool.set_suppression_limit(b, None)
    assert pool.suppression_limit(b) is None


def test_a_pool_without_limits_or_meters_launches_the_plain_step():
    eng = _StubEngine()
    pool = PacketPool(eng, 2, ring_hops=4)
    s = pool.open()
    pool.push(s, _pcm(256, 1))
    assert pool.tick() == [(s, 1, 0, 0)]
    assert eng.calls[-1][1:] == (None, [])
    with pytest.raises(RuntimeError, match="meters=True"):
        pool.levels(s)
    pool.set_suppression_limit(s, -12.0)
    pool.push(s, _pcm(256, 2))
    assert pool.tick() == [(s, 1, 256, 256)]                          # (the return value of tick() is what it was)
    assert eng.calls[-1][2] == ["levels", "min_gain"] and eng.calls[-1][1][s] == pytest.approx(10 ** (-12 / 20))


def test_open_resets_limit_and_level_row_and_levels_follow_the_ticks():
    eng = _StubEngine()
    pool = PacketPool(eng, 3, ring_hops=8, T_max=2, meters=True)
    a, b = pool.open(), pool.open()
    assert pool.levels(a) == StreamLevels() and pool.levels(a).samples == 0 and pool.levels(a).in_rms_dbfs == -math.inf
    pool.set_suppression_limit(b, -40.0)
    xa, xb = _pcm(512, 3), _pcm(256, 4)
    pool.push(a, xa)
    pool.push(b, xb)
    pool.tick()
    assert eng.calls[-1][2] == ["levels", "min_gain"] and eng.calls[-1][1].tolist() == [0.0, pytest.approx(0.01), 0.0]
    la, lb = pool.levels(a), pool.levels(b)
    fa = xa.double() / 32768.0
    assert la.samples == 512 and lb.samples == 256
    assert la.in_sumsq == pytest.approx(float((fa * fa).sum()), rel=1e-6) and la.in_peak == pytest.approx(float(fa.abs().max()), rel=1e-7)
    assert la.in_peak_dbfs == pytest.approx(20 * math.log10(float(fa.abs().max())), abs=1e-4)
    assert la.out_rms_dbfs == pytest.approx(10 * math.log10(float((fa * fa).mean())), abs=1e-4)
    pool.push(a, _pcm(100, 5))
    assert pool.tick() == [] and pool.levels(a) == la, "a tick without a hop leaves the row"
    pool.close(b)
    c = pool.open()
    assert c == b and pool.suppression_limit(c) is None and float(pool._gain[c]) == 0.0
    assert pool.levels(c) == StreamLevels() and pool._levels[c].tolist() == [0.0] * 4


def test_move_and_resize_carry_the_limit():
    eng = _StubEngine()
    src, dst = PacketPool(eng, 2, ring_hops=4, meters=True), PacketPool(eng, 3, ring_hops=4)
    eng.export_slots = lambda state, capacity, slots, out=None: torch.zeros(len(slots), 1)
    eng.import_slots = lambda state, capacity, slots, records: None
    eng.record_floats = 1
    dst.open()
    s = src.open()
    src.set_suppression_limit(s, -17.5)
    bits = float(src._gain[s])
    new = src.move(s, dst)
    assert new == 1 and float(dst._gain[new]) == bits and dst.suppression_limit(new) == pytest.approx(-17.5, abs=1e-5)
    plain = src.open()
    assert src.suppression_limit(plain) is None
    assert src.move(plain, dst) == 2 and dst.suppression_limit(2) is None
    dst.resize(6)
    assert dst._gain.numel() == 6 and float(dst._gain[1]) == bits and dst._gain.tolist()[2:] == [0.0] * 4
    t = src.open()
    src.set_suppression_limit(t, -6.0)
    src.push(t, _pcm(256, 6))
    src.tick()
    row = src.levels(t)
    src.resize(5)
    assert src._levels.shape == (5, 4) and src.levels(t) == row and src.suppression_limit(t) == pytest.approx(-6.0, abs=1e-5)
    src.resize(1)
    assert src._gain.numel() == 1 and src._levels.shape == (1, 4) and src.levels(t) == row
