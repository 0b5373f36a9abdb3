"""CPU tests of LiSenNet's opt-in time pipeline under fe_step_pool_streams_chunk[_pinned] (fe_lisennet_pool_streams_chunk_work_floats,
Engine.lisennet_pool_streams_chunk_work_floats, the scratch Engine.step_pool_streams_chunk* and serving.BacklogPacketPool pick for the family):
the declaration, the size contract of the new query, fe_step_pool_streams_chunk_work_floats staying 0, the argument checks - which never ask
for a work buffer - and the callers' choice of the scratch with the engine calls recorded, not run."""
import re
from ctypes import c_int, c_size_t, c_void_p
from pathlib import Path

import pytest
import torch

from common import hip_engine, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.family import packet_chunk_on_request
from fastenhancer_amd.serving import BacklogPacketPool, FamilyPacketPool, PacketPool
from test_cpu_lisennet_backlog import BS, CACHE_FLOATS, RING_SLOTS, TS
from test_cpu_pool_stream_ctl import BAD_ARGS, TABLES, _pcm
from test_cpu_pool_streams_chunk import ENTRY_POINTS, FE_ERR_INVALID_ARG, FE_ERR_NO_WEIGHTS, NULL, SERIAL, P, _call, _ChunkStub, _err, _no_native, _serial

HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
WIDTHS = (-1, 0, 1, 2, 8)


# ------------------------------------------------------------------ the ABI and the query
def test_the_header_declares_the_query_and_the_binding_types_it():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bsize_t\s+fe_lisennet_pool_streams_chunk_work_floats\s*\(([^)]*)\)\s*;", text)
    assert m and " ".join(m.group(1).split()) == "const fe_handle* h, int n, int T_max"
    assert _lib.SYMBOLS["fe_lisennet_pool_streams_chunk_work_floats"] == (c_size_t, [c_void_p, c_int, c_int])
    lib = _lib.load()
    fn = lib.fe_lisennet_pool_streams_chunk_work_floats
    assert fn.restype == c_size_t and fn.argtypes == [c_void_p, c_int, c_int]


def test_the_query_is_zero_where_the_pipeline_takes_nothing():
    lib = _lib.load()
    assert lib.fe_lisennet_pool_streams_chunk_work_floats(NULL, 1, 8) == 0
    for name in ("bsrnn_xxt", "bsrnn_s", "fspen", "fe_b"):
        eng = hip_engine(name)
        for n in BS:
            for T in (1, 3) + TS:
                assert eng.lisennet_pool_streams_chunk_work_floats(n, T) == 0, (name, n, T)
    ls = hip_engine("lisennet")
    for n, T in [(0, 8), (-1, 8), (1, 0), (1, 1), (1, 3), (4, 3), (129, 3), (1, -2)]:
        assert ls.lisennet_pool_streams_chunk_work_floats(n, T) == 0, (n, T)


def test_the_query_is_counters_frames_and_rings_whatever_the_setting():
    ls = hip_engine("lisennet")
    N = ls.cfg.n_fft
    prev = None
    for n in BS + (300,):                                   # (also above the streams the pipeline takes: one size for every setting)
        row = [ls.lisennet_pool_streams_chunk_work_floats(n, T) for T in TS]
        for T, v in zip(TS, row):
            assert v > n * T * N, (n, T, v)                 # more than the windowed frames [n][T_max][N]
            assert v == (9 * n + 3) // 4 * 4 + n * T * N + n * RING_SLOTS * CACHE_FLOATS, (n, T, v)
            assert v == ls.lisennet_backlog_work_floats(n, T)          # (one layout: the backlog call's)
        assert all(a <= b for a, b in zip(row, row[1:])), (n, row)    # non-decreasing in T_max ...
        if prev is not None:
            assert all(a <= b for a, b in zip(prev, row)), (n, prev, row)      # ... and in n
        prev = row
    before = ls.lisennet_pool_streams_chunk_work_floats(3, 13)
    try:
        for setting in (0, 1, 2, 8, 64, -1):                # the size does not follow fe_set_time_pipeline
            ls.set_time_pipeline(setting)
            assert ls.lisennet_pool_streams_chunk_work_floats(3, 13) == before > 0
            for n in BS:                                    # ... and the general query stays 0 for the family at every setting
                for T in (1, 3) + TS:
                    assert ls.pool_streams_chunk_work_floats(n, T) == 0, (setting, n, T)
    finally:
        ls.set_time_pipeline(-1)


# ------------------------------------------------------------------ the C call's checks
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_no_setting_makes_the_work_buffer_an_argument_error(fn):
    """an unloaded handle: with a null and with a non-null work buffer, at every width, where the pipeline would and would not run, the call
    reaches the readiness check"""
    ls = hip_engine("lisennet")
    try:
        for width in WIDTHS:
            ls.set_time_pipeline(width)
            for work in (NULL, P):
                for kw in (dict(T_max=8), dict(T_max=3), dict(T_max=251), dict(T_max=8, capacity=1000, n=1000)):
                    assert _call(ls.lib, fn, ls._h, work=work, **kw) == FE_ERR_NO_WEIGHTS, (width, work, kw, _err())
                    assert "work buffer" not in _err()
    finally:
        ls.set_time_pipeline(-1)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
@pytest.mark.parametrize("width", [2, 8])
def test_under_an_explicit_width_bad_calls_are_answered_as_the_serial_packet_step_answers_them(fn, width):
    """code and wording of fe_step_pool_streams_ctl[_pinned] under the chunk's name, in the same order (the last call is a good one)"""
    ls = hip_engine("lisennet")
    try:
        ls.set_time_pipeline(width)
        for tables in TABLES:
            for kw in BAD_ARGS + [dict()]:
                args = {**kw, **({} if "T_max" in kw else dict(T_max=8))}
                code, text = _serial(ls.lib, SERIAL[fn], ls._h, **args, **tables), _err()
                assert code != 0
                if kw:
                    assert code == FE_ERR_INVALID_ARG and SERIAL[fn] + ":" in text, (kw, text)
                want = (code, text.replace(SERIAL[fn] + ":", fn + ":"))
                for work in (NULL, P):
                    got = (_call(ls.lib, fn, ls._h, work=work, **args, **tables), _err())
                    assert got == want, (kw, tables, work, got, want)
    finally:
        ls.set_time_pipeline(-1)


# ------------------------------------------------------------------ Engine.step_pool_streams_chunk*: which query sizes the scratch
def test_the_rule_names_lisennet_under_an_explicit_width_only():
    ls = hip_engine("lisennet")
    try:
        for width in WIDTHS:
            ls.set_time_pipeline(width)
            assert packet_chunk_on_request(ls) == (width >= 2), width
    finally:
        ls.set_time_pipeline(-1)
    for name in ("bsrnn_xxt", "fspen", "fe_b"):
        eng = hip_engine(name)
        try:
            eng.set_time_pipeline(8)
            assert not packet_chunk_on_request(eng), name
        finally:
            eng.set_time_pipeline(-1)
    assert not packet_chunk_on_request(object())


def test_an_explicit_work_is_checked_against_the_lisennet_query_under_an_explicit_width(monkeypatch):
    ls = hip_engine("lisennet")
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: True)
    s, d = torch.zeros(4096, dtype=torch.int16), [(0, 8, 0, 0)]
    small = torch.zeros(8 * 512 - 1)
    try:
        for width in (2, 8):
            ls.set_time_pipeline(width)
            with pytest.raises(ValueError, match="lisennet_pool_streams_chunk_work_floats"):
                ls.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, d, s.clone(), 8, work=small)
            with pytest.raises(ValueError, match="work must be"):
                ls.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, d, s.clone(), 8, work=small.double())
        for width in (-1, 0, 1):                            # the serial call: a work buffer is passed through unread, whatever its size
            ls.set_time_pipeline(width)
            with pytest.raises(_lib.FEError, match="needs a GPU"):
                ls.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, d, s.clone(), 8, work=small)
    finally:
        ls.set_time_pipeline(-1)


# ------------------------------------------------------------------ BacklogPacketPool with the engine calls recorded
class _LisStub(_ChunkStub):
    """the recording engine of tests/test_cpu_pool_streams_chunk.py with LiSenNet's query, and the width Engine.set_time_pipeline keeps"""
    def __init__(self, cfg, width=None):
        super().__init__(cfg)
        if width is not None:
            self._time_pipeline = width

    def lisennet_pool_streams_chunk_work_floats(self, n, T_max):
        self.log.append(("lisennet_pool_streams_chunk_work_floats", n, T_max))
        return n * T_max * 512 + 1000


def _tick_a_backlog(eng, cap=4, K=8):
    pool = BacklogPacketPool(eng, cap, ring_hops=16, T_max=1, backlog_hops=K, meters=True)
    s = pool.open()
    pool.push(s, _pcm(11 * 256, 3))
    assert pool.tick() == [(s, K, s * 16 * 256, s * 16 * 256)]
    return pool, s


@pytest.mark.parametrize("width", [2, 8, 64])
def test_under_an_explicit_width_the_backlog_pool_sizes_its_scratch_by_the_lisennet_query(width):
    eng = _LisStub(product_config("lisennet"), width)
    pool, s = _tick_a_backlog(eng)
    assert [l[0] for l in eng.log] == ["lisennet_pool_streams_chunk_work_floats", "step_pool_streams_chunk_pinned", "sync"]
    assert eng.log[0] == ("lisennet_pool_streams_chunk_work_floats", 4, 8)
    assert eng.log[1][3] == ["levels", "work"] and eng.log[1][4][0] == 4 * 8 * 512 + 1000           # passed as work=
    ptr = eng.log[1][4][1]
    del eng.log[:]
    assert pool.tick() == [(s, 3, s * 4096 + 8 * 256, s * 4096 + 8 * 256)]
    assert [l[0] for l in eng.log] == ["step_pool_streams_chunk_pinned", "sync"] and eng.log[0][4][1] == ptr      # made once
    pool.resize(6)                                          # resize makes it again, for the new capacity
    pool.push(s, _pcm(2 * 256, 7))
    del eng.log[:]
    pool.tick()
    assert eng.log[0] == ("lisennet_pool_streams_chunk_work_floats", 6, 8) and eng.log[1][4][0] == 6 * 8 * 512 + 1000


@pytest.mark.parametrize("width", [None, -1, 0, 1])
def test_without_an_explicit_width_the_backlog_pool_asks_what_it_always_asked(width):
    eng = _LisStub(product_config("lisennet"), width)
    _tick_a_backlog(eng)
    assert [l[0] for l in eng.log] == ["pool_streams_chunk_work_floats", "step_pool_streams_chunk_pinned", "sync"]
    assert eng.log[1][4][0] == 4 * 8 * 512 + 4


def test_the_width_is_read_when_the_scratch_is_first_made_and_again_after_resize():
    eng = _LisStub(product_config("lisennet"), -1)
    pool, s = _tick_a_backlog(eng)
    eng._time_pipeline = 8                                  # Engine.set_time_pipeline(8) after the first backlog tick
    del eng.log[:]
    pool.tick()
    assert [l[0] for l in eng.log] == ["step_pool_streams_chunk_pinned", "sync"] and eng.log[0][4][0] == 4 * 8 * 512 + 4      # the scratch it had
    pool.resize(5)
    pool.push(s, _pcm(2 * 256, 9))
    del eng.log[:]
    pool.tick()
    assert eng.log[0] == ("lisennet_pool_streams_chunk_work_floats", 5, 8)


@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen", "fe_b"])
def test_the_other_families_never_ask_the_lisennet_query(name):
    eng = _LisStub(product_config(name), 8)
    _tick_a_backlog(eng)
    assert not any(l[0] == "lisennet_pool_streams_chunk_work_floats" for l in eng.log), eng.log


def test_the_older_pools_keep_refusing_the_backlog_for_lisennet():
    eng = _LisStub(product_config("lisennet"), 8)
    for cls in (PacketPool, FamilyPacketPool):
        with pytest.raises(ValueError, match="LiSenNet"):
            cls(eng, 4, ring_hops=16, T_max=1, backlog_hops=8)


def test_no_native_call_is_made_by_the_size_check(monkeypatch):
    """the explicit work buffer is refused by size before any call into the library but the query"""
    ls = hip_engine("lisennet")
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: True)
    s = torch.zeros(4096, dtype=torch.int16)
    try:
        ls.set_time_pipeline(8)
        _no_native(monkeypatch, ls)
        with pytest.raises(ValueError, match="work has"):
            ls.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, [(0, 8, 0, 0)], s.clone(), 8, work=torch.zeros(100))
    finally:
        monkeypatch.undo()
        ls.set_time_pipeline(-1)
