"""CPU tests of fe_step_pool_streams_chunk[_pinned] - the packet step with each stream's hops on the time pipeline for every family with a
streaming state (fe_step_pool_streams_chunk_work_floats, Engine.step_pool_streams_chunk* / pool_streams_chunk_work_floats,
family.packet_chunk_step, serving.BacklogPacketPool): the declarations, the argument checks that come before any device work, the
work-buffer size contract, and the pool's two descriptor lists with the engine calls recorded instead of run."""
import ctypes
import re
from ctypes import c_void_p
from pathlib import Path

import pytest
import torch

from common import hip_engine, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.family import packet_chunk_step
from fastenhancer_amd.serving import BacklogPacketPool, FamilyPacketPool, PacketPool
from test_cpu_pool_stream_ctl import BAD_ARGS, TABLES, _StubEngine, _pcm

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG, FE_ERR_NO_WEIGHTS = -1, -2, -4
P = c_void_p(0x1000)         # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
ENTRY_POINTS = ("fe_step_pool_streams_chunk", "fe_step_pool_streams_chunk_pinned")
SERIAL = {"fe_step_pool_streams_chunk": "fe_step_pool_streams_ctl", "fe_step_pool_streams_chunk_pinned": "fe_step_pool_streams_ctl_pinned"}
BASELINES = ["bsrnn_xt", "fspen", "lisennet"]


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0, min_gain=P, levels=P, work=P):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, min_gain, levels, work, NULL)


def _serial(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0, min_gain=P, levels=P):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, min_gain, levels, NULL)


# ------------------------------------------------------------------ the ABI
def test_the_header_declares_the_entry_points_and_the_binding_types_them():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(fe_step_pool_streams_(?:chunk|ctl)(?:_pinned)?)\s*\(([^)]*)\)\s*;", text)}
    assert set(decls) == set(ENTRY_POINTS) | set(SERIAL.values())
    assert re.search(r"\bsize_t\s+fe_step_pool_streams_chunk_work_floats\s*\(\s*const\s+fe_handle\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    lib = _lib.load()
    for fn in ENTRY_POINTS:
        # the serial call's parameter list with the work buffer in front of the stream
        head, stream = decls[SERIAL[fn]].rsplit(",", 1)
        assert re.sub(r"\s+", " ", decls[fn]) == f"{head}, float* work_dev,{stream}"
        ctl = _lib.SYMBOLS[SERIAL[fn]][1]
        assert _lib.SYMBOLS[fn] == (ctypes.c_int, ctl[:-1] + [c_void_p] + ctl[-1:])
        assert getattr(lib, fn).argtypes == _lib.SYMBOLS[fn][1] and getattr(lib, fn).restype is ctypes.c_int
    assert _lib.SYMBOLS["fe_step_pool_streams_chunk_work_floats"] == _lib.SYMBOLS["fe_step_streams_chunk_work_floats"]
    assert lib.fe_step_pool_streams_chunk_work_floats.restype is ctypes.c_size_t


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_a_null_handle_is_refused_and_sizes_nothing(fn):
    lib = _lib.load()
    assert _call(lib, fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()
    assert lib.fe_step_pool_streams_chunk_work_floats(NULL, 1, 8) == 0


@pytest.mark.parametrize("fn", ENTRY_POINTS)
@pytest.mark.parametrize("name", BASELINES + ["fe_b"])
def test_every_bad_call_is_answered_as_the_serial_packet_step_answers_it(name, fn):
    """code and wording of fe_step_pool_streams_ctl[_pinned] on the same handle, under the new function's name, with either, both or neither
    table given (the last call is a good one: these handles have no weights, and that refusal is the same too)"""
    eng = hip_engine(name)
    for tables in TABLES:
        for kw in BAD_ARGS + [dict()]:
            code, text = _serial(eng.lib, SERIAL[fn], eng._h, **kw, **tables), _err()
            assert code != 0
            if kw:
                assert code == FE_ERR_INVALID_ARG and SERIAL[fn] + ":" in text, (kw, text)
            want = (code, text.replace(SERIAL[fn] + ":", fn + ":"))
            for T_extra in (dict(), dict(T_max=8) if "T_max" not in kw else dict()):      # (also where the pipeline would run)
                if T_extra:
                    code, text = _serial(eng.lib, SERIAL[fn], eng._h, **{**kw, **T_extra}, **tables), _err()
                    want = (code, text.replace(SERIAL[fn] + ":", fn + ":"))
                got = (_call(eng.lib, fn, eng._h, **{**kw, **T_extra}, **tables), _err())
                assert got == want, (kw, tables, got, want)


@pytest.mark.parametrize("fn", ENTRY_POINTS)
@pytest.mark.parametrize("name", BASELINES)
def test_a_level_table_that_is_not_16_byte_aligned_is_refused(name, fn):
    eng = hip_engine(name)
    for off in (4, 8, 12, 1):
        assert _call(eng.lib, fn, eng._h, levels=c_void_p(0x1000 + off), T_max=8) == FE_ERR_INVALID_ARG
        assert "16-byte aligned" in _err() and fn + ":" in _err()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
@pytest.mark.parametrize("name", ["bsrnn_xt", "fspen"])
def test_a_null_work_buffer_is_refused_where_the_pipeline_would_run(name, fn):
    """an argument check: before the weights check, and it names the query.  Where nothing is pipelined no buffer is asked for."""
    eng = hip_engine(name)
    assert _call(eng.lib, fn, eng._h, T_max=8, work=NULL) == FE_ERR_INVALID_ARG
    assert fn + ": null work buffer" in _err() and "fe_step_pool_streams_chunk_work_floats(h, 1, 8)" in _err()
    assert _call(eng.lib, fn, eng._h, T_max=8, n=0, work=NULL) == FE_ERR_INVALID_ARG and "null work buffer" not in _err()      # the other arguments first
    assert _call(eng.lib, fn, eng._h, T_max=3, work=NULL) == FE_ERR_NO_WEIGHTS
    for width in (0, 1):
        eng.set_time_pipeline(width)
        assert _call(eng.lib, fn, eng._h, T_max=8, work=NULL) == FE_ERR_NO_WEIGHTS, width
    eng.set_time_pipeline(-1)
    assert _call(eng.lib, fn, eng._h, T_max=8, capacity=1000, n=1000, work=NULL) == FE_ERR_NO_WEIGHTS      # too many streams for two workgroups each
    lis = hip_engine("lisennet")
    assert _call(lis.lib, fn, lis._h, T_max=8, work=NULL) == FE_ERR_NO_WEIGHTS


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_fastenhancer_handles_take_fe_step_streams_chunk(fn):
    eng = hip_engine("fe_b")
    for n, T in [(1, 8), (3, 40), (2, 3), (0, 8)]:
        assert eng.pool_streams_chunk_work_floats(n, T) == eng.streams_chunk_work_floats(n, T)
    assert eng.pool_streams_chunk_work_floats(3, 40) > 0
    nc = hip_engine("fe_nc")
    assert _call(nc.lib, fn, nc._h, T_max=8) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err() and "use fe_offline" in _err()
    assert nc.pool_streams_chunk_work_floats(2, 8) == 0
    # fe_step_streams_chunk itself keeps refusing the baseline families
    bs = hip_engine("bsrnn_xt")
    assert bs.lib.fe_step_streams_chunk(bs._h, P, 4096, P, 4, P, P, 4096, 1, 8, 0, NULL, NULL, NULL, P, NULL) == FE_ERR_UNSUPPORTED_CONFIG
    assert bs.streams_chunk_work_floats(2, 8) == 0


# ------------------------------------------------------------------ the work buffer's size
@pytest.mark.parametrize("name", ["bsrnn_xt", "bsrnn_s", "fspen"])
def test_the_work_size_is_zero_or_covers_the_frames_and_is_monotone(name):
    eng = hip_engine(name)
    N = eng.cfg.n_fft
    for n, T in [(1, 1), (1, 3), (4, 3), (0, 8), (-1, 8), (1, 0), (1, -4)]:
        assert eng.pool_streams_chunk_work_floats(n, T) == 0, (n, T)
    Ts = (4, 5, 13, 40, 251)
    prev_row = None
    for n in (1, 2, 3, 8, 129, 300):                 # (also above the streams the pipeline takes: one size for every setting)
        row = [eng.pool_streams_chunk_work_floats(n, T) for T in Ts]
        assert all(v >= n * T * N for v, T in zip(row, Ts))          # the windowed frames [n][T_max][N] at least
        assert all(a < b for a, b in zip(row, row[1:])), (n, row)
        if prev_row is not None:
            assert all(a < b for a, b in zip(prev_row, row)), (n, prev_row, row)
        prev_row = row
    before = eng.pool_streams_chunk_work_floats(3, 40)
    assert before == eng.backlog_work_floats(3, 40)                  # (one layout: the backlog call's)
    for setting in (0, 1, 8, -1):                    # the size does not follow fe_set_time_pipeline
        eng.set_time_pipeline(setting)
        assert eng.pool_streams_chunk_work_floats(3, 40) == before > 0


def test_lisennet_needs_no_work_buffer():
    eng = hip_engine("lisennet")
    for n, T in [(1, 4), (2, 9), (8, 251)]:
        assert eng.pool_streams_chunk_work_floats(n, T) == 0


# ------------------------------------------------------------------ Engine.step_pool_streams_chunk*: the host checks of step_streams_chunk
def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen"])
def test_step_pool_streams_chunk_checks_buffers_and_work_before_any_native_call(monkeypatch, name):
    eng = hip_engine(name)
    _no_native(monkeypatch, eng)
    f, s = torch.zeros(4096), torch.zeros(4096, dtype=torch.int16)
    d = [(0, 8, 0, 0)]
    with pytest.raises(ValueError, match="one format per call"):
        eng.step_pool_streams_chunk(f, torch.zeros(1), 8, d, s, 8)
    with pytest.raises(ValueError, match="float32 or int16"):
        eng.step_pool_streams_chunk(torch.zeros(4096, dtype=torch.float64), torch.zeros(1), 8, d, f, 8)
    with pytest.raises(ValueError, match="must be a device tensor"):
        eng.step_pool_streams_chunk(f, torch.zeros(1), 8, d, f, 8)
    with pytest.raises(ValueError, match="page-locked"):
        eng.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, d, s, 8)
    with pytest.raises(TypeError):                                         # no bank table in this call
        eng.step_pool_streams_chunk(f, torch.zeros(1), 8, d, f, 8, bank=torch.zeros(8, dtype=torch.int32))
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: True)
    for work, match in [(torch.zeros(8 * 512 - 1), "work has"), (torch.zeros(8 * 512, dtype=torch.float64), "work must be"),
                        (torch.zeros(2, 8 * 512)[:, ::2], "work must be")]:
        with pytest.raises(ValueError, match=match):
            eng.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, d, s.clone(), 8, work=work)
    with pytest.raises(ValueError, match="pool_streams_chunk_work_floats"):
        eng.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, d, s.clone(), 8, work=torch.zeros(8 * 512 - 1))
    with pytest.raises(ValueError, match="min_gain must be"):
        eng.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, d, s.clone(), 8, min_gain=torch.zeros(7))
    with pytest.raises(ValueError, match="T_max"):
        eng.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, [(0, 0, 0, 0)], s.clone(), 0)


def test_step_pool_streams_chunk_needs_a_gpu_after_the_host_checks(monkeypatch):
    eng = hip_engine("fspen")
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: True)
    s = torch.zeros(4096, dtype=torch.int16)
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        eng.step_pool_streams_chunk_pinned(s, torch.zeros(1), 8, [(0, 8, 0, 0)], s.clone(), 8)


# ------------------------------------------------------------------ BacklogPacketPool with the engine calls recorded
class _ChunkStub(_StubEngine):
    """the stub engine of tests/test_cpu_pool_stream_ctl.py with the two pipelined packet calls and their queries, recorded alike"""
    device = None
    weight_banks = 1

    def __init__(self, cfg=None):
        super().__init__(cfg)
        self.log = []

    def synchronize(self):
        self.log.append(("sync",))

    def streams_chunk_work_floats(self, n, T_max):
        self.log.append(("streams_chunk_work_floats", n, T_max))
        return n * T_max * 512 + 8

    def pool_streams_chunk_work_floats(self, n, T_max):
        self.log.append(("pool_streams_chunk_work_floats", n, T_max))
        return n * T_max * 512 + 4

    def _packets(self, call, wav_in, state, capacity, desc, wav_out, T_max, ctl):
        out = super()._packets(call, wav_in, state, capacity, desc, wav_out, T_max, {k: v for k, v in ctl.items() if k in ("min_gain", "levels")})
        work = ctl.get("work")
        self.log.append((call, list(desc), T_max, sorted(k for k, v in ctl.items() if v is not None), None if work is None else (work.numel(), work.data_ptr())))
        return out

    def step_streams_chunk_pinned(self, wav_in, state, capacity, desc, wav_out, T_max, *, min_gain=None, levels=None, bank=None, work=None):
        return self._packets("step_streams_chunk_pinned", wav_in, state, capacity, desc, wav_out, T_max, dict(min_gain=min_gain, levels=levels, bank=bank, work=work))

    def step_pool_streams_chunk_pinned(self, wav_in, state, capacity, desc, wav_out, T_max, *, min_gain=None, levels=None, work=None):
        return self._packets("step_pool_streams_chunk_pinned", wav_in, state, capacity, desc, wav_out, T_max, dict(min_gain=min_gain, levels=levels, work=work))

    def step_pool_streams_chunk(self, *a, **kw):
        raise AssertionError("the device-audio step is not a packet pool's")

    step_streams_chunk = step_pool_streams_chunk


FAMILIES = [("bsrnn_xxt", "BSRNN"), ("bsrnn_s", "BSRNN"), ("fspen", "FSPEN"), ("lisennet", "LiSenNet")]


@pytest.mark.parametrize("name,call", [(n, "step_pool_streams_chunk") for n, _ in FAMILIES] + [("fe_b", "step_streams_chunk"), (None, "step_streams_chunk")])
def test_packet_chunk_step_names_the_familys_call(name, call):
    eng = _ChunkStub(product_config(name) if name else None)
    assert packet_chunk_step(eng, pinned=True) == getattr(eng, call + "_pinned")
    assert packet_chunk_step(eng, pinned=False) == getattr(eng, call)


@pytest.mark.parametrize("name,family", FAMILIES)
def test_a_baseline_backlog_pool_serves_the_backlog_in_a_second_list(name, family):
    H, K, R = 256, 8, 16 * 256
    eng = _ChunkStub(product_config(name))
    pool = BacklogPacketPool(eng, 4, ring_hops=16, T_max=1, backlog_hops=K, meters=True)
    assert pool.backlog_hops == K
    s, o1, o2 = pool.open(), pool.open(), pool.open()
    pool.set_suppression_limit(s, -12.0)
    x = _pcm(11 * H, 3)
    pool.push(s, x)
    pool.push(o1, _pcm(H, 4))
    pool.push(o2, _pcm(H, 5))
    got = pool.tick()
    assert got == [(o1, 1, o1 * R, o1 * R), (o2, 1, o2 * R, o2 * R), (s, K, s * R, s * R)]          # the ordinary launch's first, then the backlog's
    assert [l[0] for l in eng.log] == ["step_pool_streams_ctl_pinned", "pool_streams_chunk_work_floats", "step_pool_streams_chunk_pinned", "sync"]
    assert eng.log[0][1:4] == (got[:2], 1, ["levels", "min_gain"]) and eng.log[0][4] is None
    assert eng.log[1] == ("pool_streams_chunk_work_floats", 4, K)                                  # the scratch: once, for (capacity, K)
    assert eng.log[2][1:4] == (got[2:], K, ["levels", "min_gain", "work"]) and eng.log[2][4][0] == 4 * K * 512 + 4
    gains = eng.calls[-1][2]
    assert gains.tolist() == [pytest.approx(10 ** (-12 / 20)), 0.0, 0.0, 0.0]
    assert pool._stepped[s] == K * H and pool._level_samples[s] == K * H and pool.levels(s).samples == K * H
    assert torch.equal(pool.pull(s), x[:K * H])
    work_ptr = eng.log[2][4][1]
    del eng.log[:]
    assert pool.tick() == [(s, 3, s * R + K * H, s * R + K * H)]                                    # the other three: more than T_max, the backlog list again
    assert [l[0] for l in eng.log] == ["step_pool_streams_chunk_pinned", "sync"] and eng.log[0][4][1] == work_ptr
    assert torch.equal(pool.pull(s), x[K * H:])
    pool.push(s, _pcm(H, 6))
    del eng.log[:]
    assert pool.tick() == [(s, 1, s * R + 11 * H, s * R + 11 * H)]                                  # exactly T_max hops: the ordinary list
    assert [l[0] for l in eng.log] == ["step_pool_streams_ctl_pinned", "sync"]
    # resize: the scratch is made again, for the new capacity
    pool.resize(6)
    pool.push(s, _pcm(2 * H, 7))
    del eng.log[:]
    pool.tick()
    assert [l[0] for l in eng.log] == ["pool_streams_chunk_work_floats", "step_pool_streams_chunk_pinned", "sync"]
    assert eng.log[0] == ("pool_streams_chunk_work_floats", 6, K) and eng.log[1][4][0] == 6 * K * 512 + 4
    assert pool.tick() == [] and len(eng.log) == 3


@pytest.mark.parametrize("name,family", FAMILIES)
def test_a_baseline_backlog_pool_without_controls_hands_over_no_tables(name, family):
    eng = _ChunkStub(product_config(name))
    pool = BacklogPacketPool(eng, 2, ring_hops=16, T_max=2, backlog_hops=4)
    s, o = pool.open(), pool.open()
    pool.push(s, _pcm(5 * 256, 1))
    pool.push(o, _pcm(2 * 256, 2))
    assert pool.tick() == [(o, 2, o * 4096, o * 4096), (s, 4, s * 4096, s * 4096)]
    assert [l[0] for l in eng.log] == ["step_pool_streams_pinned", "pool_streams_chunk_work_floats", "step_pool_streams_chunk_pinned", "sync"]
    assert eng.log[2][3] == ["work"]
    with pytest.raises(ValueError, match="backlog_hops"):
        BacklogPacketPool(eng, 2, ring_hops=16, T_max=1, backlog_hops=3)
    with pytest.raises(ValueError, match="backlog_hops"):
        BacklogPacketPool(eng, 2, ring_hops=16, T_max=4, backlog_hops=4)


@pytest.mark.parametrize("name", ["fe_b", None])
def test_on_a_fastenhancer_engine_the_backlog_pool_is_packet_pool_call_for_call(name):
    logs = []
    for cls in (PacketPool, BacklogPacketPool):
        eng = _ChunkStub(product_config(name) if name else None)
        H = eng.cfg.hop_size
        pool = cls(eng, 3, ring_hops=16, T_max=2, meters=True, backlog_hops=8)
        a, b = pool.open(), pool.open()
        ticks = []
        for t in range(4):
            if t == 2:
                pool.set_suppression_limit(b, -20.0)
            pool.push(a, _pcm(H + 7, 10 + t))
            pool.push(b, _pcm((5 if t == 1 else 2) * H, 20 + t))
            ticks.append(pool.tick())
        logs.append((ticks, [l[:4] + (l[4] and l[4][0],) if len(l) > 4 else l for l in eng.log], pool.levels(a), pool.levels(b)))
    assert logs[0] == logs[1]
    names = [l[0] for l in logs[1][1]]
    assert "step_streams_chunk_pinned" in names and "streams_chunk_work_floats" in names and not any("pool" in n for n in names)
    chunk = [l for l in logs[1][1] if l[0] == "step_streams_chunk_pinned"][0]
    assert chunk[3] == ["levels", "work"]


@pytest.mark.parametrize("name,family", FAMILIES)
def test_the_older_pools_still_refuse_the_backlog_and_the_new_one_banks(name, family):
    eng = _ChunkStub(product_config(name))
    for cls in (PacketPool, FamilyPacketPool):
        with pytest.raises(ValueError, match=family) as e:
            cls(eng, 4, ring_hops=16, T_max=1, backlog_hops=8)
        assert "the pipelined packet step (backlog_hops)" in str(e.value) and "FastEnhancer family" in str(e.value)
    pool = BacklogPacketPool(eng, 4, ring_hops=16, T_max=1, backlog_hops=8)
    s = pool.open()
    with pytest.raises(ValueError, match=family) as e:
        pool.set_bank(s, 1)
    assert "BacklogPacketPool" in str(e.value) and "weight bank" in str(e.value)
    with pytest.raises(ValueError, match=family):
        pool.open(bank=1)
    pool.set_bank(s, 0)
    assert pool.bank(s) == 0 and pool.active == [s] and eng.log == []
