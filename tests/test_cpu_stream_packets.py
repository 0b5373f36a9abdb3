"""CPU tests of the packet-audio streaming step (fe_step_streams / fe_step_streams_pinned, Engine.step_streams*, serving.PacketPool):
the descriptor struct of the header against the ctypes one, the argument checks that come before any device work, and PacketPool's ring
bookkeeping with the engine call replaced by a stub that copies the launched input hops to the output."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool, StreamPool

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastenhancer_hip.h")
FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
ENTRY_POINTS = ("fe_step_streams", "fe_step_streams_pinned")


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, NULL)


# ------------------------------------------------------------------ the ABI
def test_stream_desc_of_the_header_is_the_ctypes_struct(tmp_path):
    src = open(HEADER).read()
    body = re.search(r"typedef struct fe_stream_desc \{(.*?)\} fe_stream_desc;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(d.strip().rsplit(None, 1)) for d in body.split(";") if d.strip()]
    assert fields == [("int", "slot"), ("int", "hops"), ("long long", "in_offset"), ("long long", "out_offset")]
    ctype = {"int": ctypes.c_int, "long long": ctypes.c_longlong}
    assert [(ctype[t], n) for t, n in fields] == [(t, n) for n, t in _lib.fe_stream_desc._fields_]
    assert ctypes.sizeof(_lib.fe_stream_desc) == 24
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or next(
        (p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    if cc is not None:
        names = [n for _, n in fields]
        probe = tmp_path / "probe.c"
        probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fastenhancer_hip.h"\nint main(void) {\n'
                         + "".join(f'    printf("{n} %zu\\n", offsetof(fe_stream_desc, {n}));\n' for n in names)
                         + '    printf("sizeof %zu\\n", sizeof(fe_stream_desc));\n'
                         + '    printf("FE_AUDIO_F32 %d\\nFE_AUDIO_S16 %d\\n", FE_AUDIO_F32, FE_AUDIO_S16);\n    return 0;\n}\n')
        exe = tmp_path / "probe"
        subprocess.run([cc, "-I", os.path.dirname(HEADER), str(probe), "-o", str(exe)], check=True, capture_output=True, timeout=120)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
        c = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
        for n in names:
            assert getattr(_lib.fe_stream_desc, n).offset == c[n], n
        assert c["sizeof"] == ctypes.sizeof(_lib.fe_stream_desc) == 24
        assert (c["FE_AUDIO_F32"], c["FE_AUDIO_S16"]) == (_lib.FE_AUDIO_F32, _lib.FE_AUDIO_S16)
    defs = dict(re.findall(r"#define (FE_AUDIO_\w+) (\d+)", src))
    assert {k: int(v) for k, v in defs.items()} == {"FE_AUDIO_F32": _lib.FE_AUDIO_F32, "FE_AUDIO_S16": _lib.FE_AUDIO_S16} == {"FE_AUDIO_F32": 0, "FE_AUDIO_S16": 1}


def test_pack_stream_desc_is_the_memory_image_of_the_struct():
    rows = [(3, 2, 5, 7), (0, 0, -1, 2 ** 40 + 9), (-4, 9, 2 ** 33, -2 ** 35)]
    t = Engine.pack_stream_desc(rows)
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 6)
    back = (_lib.fe_stream_desc * 3).from_buffer_copy(t.numpy().tobytes())
    assert [(d.slot, d.hops, d.in_offset, d.out_offset) for d in back] == rows
    with pytest.raises(ValueError, match="slot, hops, in_offset, out_offset"):
        Engine.pack_stream_desc([(1, 2, 3)])


# ------------------------------------------------------------------ argument checks of the library (no GPU: they come first)
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_stream_entry_points_refuse_a_null_handle(fn):
    lib = _lib.load()
    assert _call(lib, fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_stream_entry_points_check_their_arguments(fn):
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
def test_stream_entry_points_refuse_the_baseline_families_and_the_noncausal_model(fn):
    eng = Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xt"][0]), None)
    assert _call(eng.lib, fn, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "FastEnhancer family" in _err() and "dptransformer" in _err() and fn in _err()
    nc = Engine(product_config("fe_nc"), None)
    assert _call(nc.lib, fn, nc._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err()


def _no_native(monkeypatch, eng):
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


@pytest.mark.parametrize("desc,match", [
    ([(0, 1, 0, 0), (0, 1, 256, 256)], "duplicate"),
    ([(8, 1, 0, 0)], "slot 8 is outside"),
    ([(-1, 1, 0, 0)], "slot -1 is outside"),
    ([(0, 3, 0, 0)], r"hops 3 is outside \[0, 2\]"),
    ([(0, -1, 0, 0)], "hops -1 is outside"),
    ([(0, 2, 513, 0)], "input range"),
    ([(0, 1, -1, 0)], "input range"),
    ([(0, 2, 0, 600)], "output range"),
    ([], "0 streams"),
    (torch.zeros(2, 4, dtype=torch.int32), "int32 tensor"),
    (torch.zeros(2, 6, dtype=torch.int64), "int32 tensor"),
])
def test_host_descriptors_are_checked_before_any_device_call(monkeypatch, desc, match):
    eng = Engine(product_config("fe_b"), None)
    _no_native(monkeypatch, eng)
    with pytest.raises(ValueError, match=match):
        eng._stream_desc_tensor(desc, 8, 2, 1024, 1024)


def test_step_streams_checks_its_buffers_before_any_device_call(monkeypatch):
    eng = Engine(product_config("fe_b"), None)
    _no_native(monkeypatch, eng)
    f, s = torch.zeros(1024), torch.zeros(1024, dtype=torch.int16)
    with pytest.raises(ValueError, match="one format per call"):
        eng.step_streams(f, torch.zeros(1), 8, [(0, 1, 0, 0)], s)
    with pytest.raises(ValueError, match="float32 or int16"):
        eng.step_streams(torch.zeros(1024, dtype=torch.float64), torch.zeros(1), 8, [(0, 1, 0, 0)], f)
    with pytest.raises(ValueError, match="must be a device tensor"):
        eng.step_streams(f, torch.zeros(1), 8, [(0, 1, 0, 0)], f)
    with pytest.raises(ValueError, match="page-locked"):
        eng.step_streams_pinned(s, torch.zeros(1), 8, [(0, 1, 0, 0)], s)


# ------------------------------------------------------------------ PacketPool with the engine stubbed
class _Cfg:
    hop_size = 256


class _StubEngine:
    """what PacketPool needs of an Engine: the launch copies every launched input hop to its output place (an identity "model")"""
    cfg = _Cfg()

    def __init__(self):
        self.launches = []

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        pass

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        pass

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1):
        H = self.cfg.hop_size
        assert wav_in.dtype == wav_out.dtype == torch.int16
        fin, fout = wav_in.view(-1), wav_out.view(-1)
        for slot, hops, i0, o0 in desc:
            assert 1 <= hops <= T_max and 0 <= slot < capacity
            assert 0 <= i0 and i0 + hops * H <= fin.numel() and 0 <= o0 and o0 + hops * H <= fout.numel()
            fout[o0:o0 + hops * H] = fin[i0:i0 + hops * H]
        self.launches.append(list(desc))
        return wav_out


def _pcm(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-32768, 32768, size=n, dtype=np.int16))


@pytest.mark.parametrize("packet", [160, 320, 100, 1000])
def test_packet_pool_returns_exactly_what_was_pushed_delayed_and_in_order(packet):
    """packets of 160 / 320 / 100 / 1000 samples against a hop of 256 over 60 ticks, the ring (8 hops) wrapping many times"""
    eng = _StubEngine()
    pool = PacketPool(eng, 4, ring_hops=8, T_max=4)
    assert isinstance(pool, StreamPool)
    slot = pool.open()
    sent, got = [], []
    pushed = stepped = 0
    for tick in range(60):
        x = _pcm(packet, 1000 * packet + tick)
        pool.push(slot, x if tick % 2 else x.numpy())               # tensors and numpy arrays alike
        sent.append(x)
        pushed += packet
        desc = pool.tick()
        pos = stepped % (8 * 256)
        want = min((pushed - stepped) // 256, (8 * 256 - pos) // 256, 4)
        if want == 0:
            assert desc == []
        else:
            assert desc == [(slot, want, slot * 8 * 256 + pos, slot * 8 * 256 + pos)]
            assert pos + want * 256 <= 8 * 256                       # never across the ring end
        stepped += want * 256
        y = pool.pull(slot)
        assert y.dtype == torch.int16 and y.numel() == want * 256
        got.append(y)
    sent, got = torch.cat(sent), torch.cat(got)
    assert got.numel() == stepped >= 60 * packet - 4 * 256 and stepped % 256 == 0
    assert torch.equal(got, sent[:got.numel()])
    assert sum(len(d) for d in eng.launches) == len(eng.launches)   # one stream, one descriptor per launch
    assert stepped > 2 * 8 * 256                                     # the ring wrapped (at least twice)


def test_packet_pool_caps_hops_at_t_max_and_splits_at_the_ring_end():
    eng = _StubEngine()
    pool = PacketPool(eng, 2, ring_hops=4, T_max=2)
    s = pool.open()
    x = _pcm(4 * 256, 5)
    pool.push(s, x[:3 * 256 + 10])
    assert pool.tick() == [(s, 2, 0, 0)]                             # three hops are complete: T_max caps the launch at two
    assert pool.tick() == [(s, 1, 512, 512)]                         # the third on the next tick
    assert pool.tick() == [] and len(eng.launches) == 2              # 10 samples: no hop, no launch
    assert torch.equal(pool.pull(s), x[:3 * 256])
    pool.push(s, x[3 * 256 + 10:])                                   # completes hop 3, the last one before the ring end
    pool.push(s, x[:300])                                            # wraps on the host: 300 samples at the ring start
    assert pool.tick() == [(s, 1, 3 * 256, 3 * 256)]                 # two hops are complete, one is contiguous to the ring end
    assert pool.tick() == [(s, 1, 0, 0)]
    assert torch.equal(pool.pull(s), torch.cat([x[3 * 256:], x[:256]]))
    assert pool.pull(s).numel() == 0


def test_packet_pool_leaves_zero_hop_streams_out_of_the_launch():
    eng = _StubEngine()
    pool = PacketPool(eng, 8, ring_hops=4, T_max=3)
    a, b, c, d = pool.open(), pool.open(), pool.open(), pool.open()
    pool.close(b)
    pool.push(a, _pcm(255, 1))                                       # no complete hop
    pool.push(c, _pcm(256, 2))                                       # one
    pool.push(d, _pcm(1000, 3))                                      # three (232 left over)
    R = 4 * 256
    assert pool.tick() == [(c, 1, c * R, c * R), (d, 3, d * R, d * R)]
    assert eng.launches == [[(c, 1, c * R, c * R), (d, 3, d * R, d * R)]]
    pool.push(a, _pcm(1, 4))
    assert pool.tick() == [(a, 1, a * R, a * R)]
    assert pool.pull(a).numel() == 256 and pool.pull(c).numel() == 256 and pool.pull(d).numel() == 768
    with pytest.raises(ValueError, match="not open"):
        pool.push(b, _pcm(10, 5))
    with pytest.raises(ValueError, match="not open"):
        pool.pull(b)
    e = pool.open()                                                  # the freed slot, its counters reset
    assert e == b
    pool.push(e, _pcm(256, 6))
    assert pool.tick() == [(e, 1, e * R, e * R)]


def test_packet_pool_refuses_what_would_overwrite_unpulled_samples_and_bad_packets():
    eng = _StubEngine()
    pool = PacketPool(eng, 1, ring_hops=2, T_max=1)
    s = pool.open()
    pool.push(s, _pcm(512, 1))
    with pytest.raises(OverflowError, match="do not fit"):
        pool.push(s, _pcm(1, 2))
    pool.tick()
    with pytest.raises(OverflowError):                              # stepped, but not pulled yet: the output is still in the ring
        pool.push(s, _pcm(1, 2))
    assert pool.pull(s).numel() == 256
    pool.push(s, _pcm(256, 3))
    with pytest.raises(ValueError, match="1-D int16"):
        pool.push(s, torch.zeros(4))
    with pytest.raises(ValueError, match="1-D int16"):
        pool.push(s, torch.zeros(2, 2, dtype=torch.int16))
    with pytest.raises(ValueError):
        PacketPool(eng, 1, ring_hops=0, T_max=1)
    with pytest.raises(ValueError):
        PacketPool(eng, 1, ring_hops=2, T_max=0)
