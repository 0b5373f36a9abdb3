"""CPU tests of the packet step's time-pipelined form (fe_step_streams_chunk[_pinned], fe_step_streams_chunk_work_floats,
Engine.step_streams_chunk* / streams_chunk_work_floats, PacketPool(backlog_hops=) and PacketPool.catch_up): the argument checks that come
before any device work, the work-buffer size contract, and the pool's two descriptor lists with the engine calls stubbed."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool, StreamPool

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
ENTRY_POINTS = ("fe_step_streams_chunk", "fe_step_streams_chunk_pinned")


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, wav_in=P, in_count=4096, state=P, capacity=4, desc=P, wav_out=P, out_count=4096, n=1, T_max=8, fmt=0, work=P):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, NULL, NULL, NULL, work, NULL)


# ------------------------------------------------------------------ argument checks of the library (no GPU: they come first)
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_chunk_entry_points_refuse_a_null_handle(fn):
    lib = _lib.load()
    assert _call(lib, fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()
    assert lib.fe_step_streams_chunk_work_floats(NULL, 1, 8) == 0


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_chunk_entry_points_check_their_arguments_as_the_packet_step_does(fn):
    eng = Engine(product_config("fe_b"), None)
    bad = [dict(wav_in=NULL), dict(state=NULL), dict(desc=NULL), dict(wav_out=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0),
           dict(T_max=0), dict(T_max=-2), dict(in_count=0), dict(out_count=0)]
    for kw in bad:
        assert _call(eng.lib, fn, eng._h, **kw) == FE_ERR_INVALID_ARG, kw
        assert fn in _err() and "1 <= n <= capacity" in _err() and "T_max >= 1" in _err(), (kw, _err())
    for fmt in (2, -1, 16):
        assert _call(eng.lib, fn, eng._h, fmt=fmt) == FE_ERR_INVALID_ARG, fmt
        assert "FE_AUDIO_S16" in _err() and str(fmt) in _err()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_chunk_entry_points_refuse_the_families_the_packet_step_refuses(fn):
    from common import FSPEN_KWARGS, LISENNET_KWARGS
    from fastenhancer_amd.config import FSPENConfig, LiSenNetConfig
    engines = [Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xt"][0]), None),
               Engine(FSPENConfig.from_model_kwargs(**FSPEN_KWARGS[0]), None),
               Engine(LiSenNetConfig.from_model_kwargs(**LISENNET_KWARGS[0]), None)]
    for eng in engines:
        ref = eng.lib.fe_step_streams(eng._h, P, 4096, P, 4, P, P, 4096, 1, 8, 0, NULL)
        assert ref == FE_ERR_UNSUPPORTED_CONFIG
        assert _call(eng.lib, fn, eng._h) == ref
        assert "FastEnhancer family" in _err() and fn in _err()
        assert eng.streams_chunk_work_floats(2, 8) == 0
    nc = Engine(product_config("fe_nc"), None)
    assert _call(nc.lib, fn, nc._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()


# ------------------------------------------------------------------ the work buffer's size
def test_streams_chunk_work_floats_is_zero_where_nothing_is_pipelined():
    eng = Engine(product_config("fe_b"), None)
    for n, T in [(1, 1), (1, 3), (4, 3), (0, 8), (-1, 8), (1, 0)]:
        assert eng.streams_chunk_work_floats(n, T) == 0, (n, T)
    for name in ("fe_tk_b", "fe_dpt_t", "fe_nc"):                # the ring variants take the serial packet step; the noncausal model has no step
        e = Engine(product_config(name), None)
        assert e.streams_chunk_work_floats(2, 8) == 0 and e.streams_chunk_work_floats(1, 251) == 0, name
    bs = Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xxt"][0]), None)
    assert bs.streams_chunk_work_floats(2, 5) == 0 and bs.streams_chunk_work_floats(1, 251) == 0


def test_streams_chunk_work_floats_is_positive_and_monotone():
    eng = Engine(product_config("fe_b"), None)
    N = eng.cfg.n_fft
    Ts = (4, 5, 13, 40, 251)
    prev_row = None
    for n in (1, 2, 3, 8, 129, 300):                 # (also above the streams the pipeline takes: one size for every setting)
        row = [eng.streams_chunk_work_floats(n, T) for T in Ts]
        assert all(v > 0 for v in row)
        assert all(a < b for a, b in zip(row, row[1:])), (n, row)
        assert all(v >= n * T * N for v, T in zip(row, Ts))          # the windowed frames [n][T_max][N] at least
        if prev_row is not None:
            assert all(a < b for a, b in zip(prev_row, row)), (n, prev_row, row)
        prev_row = row
    before = eng.streams_chunk_work_floats(3, 40)
    for setting in (0, 1, 4, 64, -1):                # the size does not follow fe_set_time_pipeline
        eng.set_time_pipeline(setting)
        assert eng.streams_chunk_work_floats(3, 40) == before


# ------------------------------------------------------------------ Engine: shapes and dtypes before any native call
def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


def test_step_streams_chunk_checks_its_buffers_before_any_native_call(monkeypatch):
    eng = Engine(product_config("fe_b"), None)
    _no_native(monkeypatch, eng)
    f, s = torch.zeros(4096), torch.zeros(4096, dtype=torch.int16)
    d = [(0, 8, 0, 0)]
    with pytest.raises(ValueError, match="one format per call"):
        eng.step_streams_chunk(f, torch.zeros(1), 8, d, s, 8)
    with pytest.raises(ValueError, match="float32 or int16"):
        eng.step_streams_chunk(torch.zeros(4096, dtype=torch.float64), torch.zeros(1), 8, d, f, 8)
    with pytest.raises(ValueError, match="float32 or int16"):
        eng.step_streams_chunk(f, torch.zeros(1), 8, d, torch.zeros(4096, dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="must be a device tensor"):
        eng.step_streams_chunk(f, torch.zeros(1), 8, d, f, 8)
    with pytest.raises(ValueError, match="page-locked"):
        eng.step_streams_chunk_pinned(s, torch.zeros(1), 8, d, s, 8)


@pytest.mark.parametrize("work,match", [
    (torch.zeros(8 * 512 - 1), "work has"),                                  # shorter than the windowed frames [1][8][512]
    (torch.zeros(8 * 512, dtype=torch.float64), "work must be"),
    (torch.zeros(2, 8 * 512)[:, ::2], "work must be"),
])
def test_step_streams_chunk_checks_the_work_tensor_before_any_native_call(monkeypatch, work, match):
    eng = Engine(product_config("fe_b"), None)
    # (a stand-in for page-locked audio: the buffers' own checks pass, so the work tensor's are reached without a GPU)
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: True)
    _no_native(monkeypatch, eng)
    s = torch.zeros(4096, dtype=torch.int16)
    with pytest.raises(ValueError, match=match):
        eng.step_streams_chunk_pinned(s, torch.zeros(1), 8, [(0, 8, 0, 0)], s.clone(), 8, work=work)
    with pytest.raises(ValueError, match="T_max"):
        eng.step_streams_chunk_pinned(s, torch.zeros(1), 8, [(0, 0, 0, 0)], s.clone(), 0, work=work)


def test_step_streams_chunk_needs_a_gpu_after_the_host_checks(monkeypatch):
    eng = Engine(product_config("fe_b"), None)
    monkeypatch.setattr(torch.Tensor, "is_pinned", lambda self, *a, **k: True)
    s = torch.zeros(4096, dtype=torch.int16)
    with pytest.raises(_lib.FEError, match="needs a GPU"):
        eng.step_streams_chunk_pinned(s, torch.zeros(1), 8, [(0, 8, 0, 0)], s.clone(), 8)


# ------------------------------------------------------------------ PacketPool with the engine stubbed
class _Cfg:
    hop_size = 256


class _StubEngine:
    """what PacketPool needs of an Engine: either launch copies every launched input hop to its output place (an identity "model") and
    records its descriptors and keyword arguments"""
    cfg = _Cfg()
    device = None
    weight_banks = 2

    def __init__(self):
        self.launches, self.calls = [], []
        self.record = torch.arange(6, dtype=torch.float32).view(1, 6)

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        pass

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        self.launches.append(("sync",))

    def streams_chunk_work_floats(self, n, T_max):
        self.launches.append(("work_floats", n, T_max))
        return n * T_max * 512 + 4

    def _copy(self, wav_in, capacity, desc, wav_out, T_max):
        H = self.cfg.hop_size
        assert wav_in.dtype == wav_out.dtype == torch.int16
        fin, fout = wav_in.view(-1), wav_out.view(-1)
        for slot, hops, i0, o0 in desc:
            assert 1 <= hops <= T_max and 0 <= slot < capacity
            assert 0 <= i0 and i0 + hops * H <= fin.numel() and 0 <= o0 and o0 + hops * H <= fout.numel()
            fout[o0:o0 + hops * H] = fin[i0:i0 + hops * H]

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, **ctl):
        self._copy(wav_in, capacity, desc, wav_out, T_max)
        self.launches.append(("serial", list(desc), T_max, sorted(ctl)))
        return wav_out

    def step_streams_chunk_pinned(self, wav_in, state, capacity, desc, wav_out, T_max, *, min_gain=None, levels=None, bank=None, work=None):
        self._copy(wav_in, capacity, desc, wav_out, T_max)
        self.launches.append(("chunk", list(desc), T_max, work.numel(), work.data_ptr(), min_gain is not None, levels is not None, bank is not None))
        return wav_out

    # (catch_up)
    def export_slots(self, state, capacity, slots, out=None):
        self.calls.append(("export", capacity, list(slots)))
        return self.record

    def step_chunk(self, wav_in, state, wav_out=None, T=None, work=None):
        self.calls.append(("step_chunk", tuple(wav_in.shape), T))
        return wav_in * 2.0

    def import_slots(self, state, capacity, slots, records):
        self.calls.append(("import", capacity, list(slots)))


def _pcm(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-32768, 32768, size=n, dtype=np.int16))


def test_packet_pool_without_backlog_hops_makes_the_calls_of_today():
    eng = _StubEngine()
    pool = PacketPool(eng, 4, ring_hops=16, T_max=2)
    assert pool.backlog_hops == 0
    a, b = pool.open(), pool.open()
    x = _pcm(11 * 256, 1)
    pool.push(a, x)
    pool.push(b, x[:256])
    R = 16 * 256
    assert pool.tick() == [(a, 2, a * R, a * R), (b, 1, b * R, b * R)]       # eleven hops wait: two a tick
    assert eng.launches == [("serial", [(a, 2, a * R, a * R), (b, 1, b * R, b * R)], 2, []), ("sync",)]
    assert pool.tick() == [(a, 2, a * R + 512, a * R + 512)]
    assert [l[0] for l in eng.launches] == ["serial", "sync", "serial", "sync"]
    assert torch.equal(pool.pull(a), x[:4 * 256])


def test_packet_pool_serves_a_backlog_in_a_second_list():
    H, K, R = 256, 8, 16 * 256
    eng = _StubEngine()
    pool = PacketPool(eng, 4, ring_hops=16, T_max=1, backlog_hops=K)
    s, o1, o2 = pool.open(), pool.open(), pool.open()
    sent = []

    def push(slot, hops, seed):
        x = _pcm(hops * H, seed)
        pool.push(slot, x)
        if slot == s:
            sent.append(x)

    # the stream to 13 hops: 3 hops before the ring end
    push(s, 8, 1)
    assert pool.tick() == [(s, 8, s * R, s * R)]
    push(s, 5, 2)
    assert pool.tick() == [(s, 5, s * R + 8 * H, s * R + 8 * H)]
    assert pool._stepped[s] == 13 * H and torch.equal(pool.pull(s), torch.cat(sent))
    assert [l[0] for l in eng.launches] == ["work_floats", "chunk", "sync", "chunk", "sync"]
    assert eng.launches[0] == ("work_floats", 4, K)                          # the work tensor: once, for (capacity, K)
    work_ptr = eng.launches[1][4]
    assert eng.launches[1][2] == K and eng.launches[1][3] == 4 * K * 512 + 4
    del eng.launches[:]
    # eleven hops arrive at once, next to two one-hop streams
    push(s, 11, 3)
    push(o1, 1, 4)
    push(o2, 1, 5)
    pos = s * R + 13 * H
    got = pool.tick()
    assert got == [(o1, 1, o1 * R, o1 * R), (o2, 1, o2 * R, o2 * R), (s, 3, pos, pos)]      # up to the ring end: three hops, on the chunk list
    assert [l[0] for l in eng.launches] == ["serial", "chunk", "sync"]                      # the ordinary launch first, one synchronise
    assert eng.launches[0][1] == got[:2] and eng.launches[0][2] == 1
    assert eng.launches[1][1] == got[2:] and eng.launches[1][2] == K and eng.launches[1][4] == work_ptr
    assert eng.launches[1][5:] == (False, False, False)                                     # no limit, no meters, no banks in this pool
    assert pool._stepped[s] == 16 * H and pool._stepped[o1] == H
    assert torch.equal(pool.pull(s), sent[2][:3 * H]) and pool.pull(o1).numel() == H
    del eng.launches[:]
    assert pool.tick() == [(s, 8, s * R, s * R)]                                            # the next tick: the other eight, from the ring start
    assert [l[0] for l in eng.launches] == ["chunk", "sync"]
    assert pool._stepped[s] == 24 * H and torch.equal(pool.pull(s), sent[2][3 * H:])
    assert pool.tick() == [] and [l[0] for l in eng.launches] == ["chunk", "sync"]
    # a stream with exactly T_max hops stays on the ordinary list
    push(s, 1, 6)
    assert pool.tick() == [(s, 1, s * R + 8 * H, s * R + 8 * H)]
    assert eng.launches[-2][0] == "serial"


def test_packet_pool_backlog_launch_carries_the_pools_tables():
    eng = _StubEngine()
    pool = PacketPool(eng, 2, ring_hops=16, T_max=1, meters=True, backlog_hops=4)
    s = pool.open(bank=1)
    pool.set_suppression_limit(s, -12.0)
    pool.push(s, _pcm(5 * 256, 1))
    assert pool.tick() == [(s, 4, s * 16 * 256, s * 16 * 256)]
    assert eng.launches[1][0] == "chunk" and eng.launches[1][5:] == (True, True, True)
    assert pool._level_samples[s] == 4 * 256
    with pytest.raises(ValueError, match="backlog_hops"):
        PacketPool(eng, 2, ring_hops=16, T_max=1, backlog_hops=3)


def test_packet_pool_catch_up_refuses_a_bank_or_a_limit_and_is_inherited_otherwise():
    eng = _StubEngine()
    pool = PacketPool(eng, 4, ring_hops=8, T_max=1)
    plain, banked, limited = pool.open(), pool.open(bank=1), pool.open()
    pool.set_suppression_limit(limited, -20.0)
    x = torch.ones(5 * 4)
    with pytest.raises(ValueError, match="backlog_hops"):
        pool.catch_up(banked, x, 5)
    with pytest.raises(ValueError, match="backlog_hops"):
        pool.catch_up(limited, x, 5)
    with pytest.raises(ValueError, match="not open"):
        pool.catch_up(3, x, 5)
    assert eng.calls == []
    y = pool.catch_up(plain, x, 5)
    assert eng.calls == [("export", 4, [plain]), ("step_chunk", (1, 20), 5), ("import", 4, [plain])]
    assert torch.equal(y, torch.full((1, 20), 2.0))
    pool.set_suppression_limit(limited, None)                                # the limit lifted: served again
    pool.catch_up(limited, x, 5)
    assert [c[0] for c in eng.calls[3:]] == ["export", "step_chunk", "import"]
    # StreamPool's own catch_up knows neither
    assert StreamPool.catch_up is not PacketPool.catch_up
