"""CPU tests of fe_step_pool_streams_ctl[_pinned] - the packet step's suppression limit and level meters for every family with a streaming
state (Engine.step_pool_streams_ctl*, family.packet_ctl_step, serving.FamilyPacketPool): the declarations, the argument checks that come before
any device work, the pool's choice of call and its remaining refusals with the engine calls recorded instead of run, and - on the oracle side -
that the composed reference of the GPU test (tests/pool_ctl_oracle.py) is oracle.step when the limit is off, satisfies the contract's inequality
when it is on, and exercises the floor on the GPU test's inputs."""
import ctypes
import re
from ctypes import c_void_p
from pathlib import Path

import numpy as np
import pytest
import torch

import pool_ctl_oracle as pco
from common import build_named_oracle, hip_engine, product_config, rms
from fastenhancer_amd import _lib
from fastenhancer_amd.family import packet_ctl_step
from fastenhancer_amd.serving import FamilyPacketPool, PacketPool, StreamLevels

FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG = -1, -2
P = c_void_p(0x1000)         # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
HEADER = Path(__file__).resolve().parent.parent / "include" / "fastenhancer_hip.h"
TWINS = {"fe_step_pool_streams_ctl": "fe_step_streams_ctl", "fe_step_pool_streams_ctl_pinned": "fe_step_streams_ctl_pinned"}
HANDLES = ["fe_b", "bsrnn_xxt", "fspen", "lisennet"]
# the argument table of tests/test_cpu_stream_ctl.py
BAD_ARGS = [dict(wav_in=NULL), dict(state=NULL), dict(desc=NULL), dict(wav_out=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0),
            dict(T_max=0), dict(T_max=-2), dict(in_count=0), dict(out_count=0), dict(fmt=2), dict(fmt=-1), dict(fmt=16)]
TABLES = [dict(), dict(min_gain=NULL), dict(levels=NULL), dict(min_gain=NULL, levels=NULL)]


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0, min_gain=P, levels=P):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, min_gain, levels, NULL)


# ------------------------------------------------------------------ the ABI
def test_the_header_declares_both_functions_and_the_binding_types_them_like_fe_step_streams_ctl():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(fe_step_(?:pool_)?streams_ctl(?:_pinned)?)\s*\(([^)]*)\)\s*;", text)}
    assert set(decls) == set(TWINS) | set(TWINS.values())
    lib = _lib.load()
    for fn, twin in TWINS.items():
        assert decls[fn] == decls[twin]                                              # the same parameter list, word for word
        assert _lib.SYMBOLS[fn] == _lib.SYMBOLS[twin] and _lib.SYMBOLS[fn][0] is ctypes.c_int
        assert getattr(lib, fn).argtypes == getattr(lib, twin).argtypes and getattr(lib, fn).restype == getattr(lib, twin).restype
        plain = _lib.SYMBOLS[fn.replace("_ctl", "")][1]
        assert _lib.SYMBOLS[fn][1] == plain[:-1] + [c_void_p, c_void_p] + plain[-1:]  # the two tables before the stream


@pytest.mark.parametrize("fn", TWINS)
def test_pool_streams_ctl_refuses_a_null_handle(fn):
    lib = _lib.load()
    assert _call(lib, fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("fn", TWINS)
@pytest.mark.parametrize("name", HANDLES)
def test_pool_streams_ctl_answers_every_bad_call_as_fe_step_streams_ctl_does(name, fn):
    """code and wording of fe_step_streams_ctl[_pinned] on a FastEnhancer handle in the same condition, under the new function's name, with
    either, both or neither table given (the last call is a good one: these handles have no weights, and that refusal is the same too)"""
    ref, eng = hip_engine("fe_b"), hip_engine(name)
    assert ref.cfg.hop_size == eng.cfg.hop_size == 256
    for tables in TABLES:
        for kw in BAD_ARGS + [dict()]:
            code, text = _call(ref.lib, TWINS[fn], ref._h, **kw, **tables), _err()
            assert code != 0
            if kw:
                assert code == FE_ERR_INVALID_ARG and TWINS[fn] + ":" in text, (kw, text)
            want = (code, text.replace(TWINS[fn] + ":", fn + ":"))
            got = (_call(eng.lib, fn, eng._h, **kw, **tables), _err())
            assert got == want, (kw, tables, got, want)


@pytest.mark.parametrize("fn", TWINS)
@pytest.mark.parametrize("name", HANDLES)
def test_a_level_table_that_is_not_16_byte_aligned_is_refused(name, fn):
    ref, eng = hip_engine("fe_b"), hip_engine(name)
    for off in (4, 8, 12, 1):
        code, text = _call(ref.lib, TWINS[fn], ref._h, levels=c_void_p(0x1000 + off)), _err()
        assert code == FE_ERR_INVALID_ARG and "16-byte aligned" in text
        assert (_call(eng.lib, fn, eng._h, levels=c_void_p(0x1000 + off)), _err()) == (code, text.replace(TWINS[fn] + ":", fn + ":")), off
    assert _call(eng.lib, fn, eng._h, min_gain=c_void_p(0x1004), levels=NULL) != 0                                     # (any float alignment for min_gain)
    assert "16-byte" not in _err()


@pytest.mark.parametrize("fn", TWINS)
def test_pool_streams_ctl_refuses_the_noncausal_model_as_fe_step_does(fn):
    eng = hip_engine("fe_nc")
    assert _call(eng.lib, fn, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
    assert "the noncausal model has no streaming step" in _err() and "use fe_offline" in _err()


# ------------------------------------------------------------------ Engine.step_pool_streams_ctl*: the host checks of step_streams(min_gain=, levels=)
def _no_native(monkeypatch, eng):
    """any call into the library from here on fails the test"""
    class Guard:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    monkeypatch.setattr(eng, "lib", Guard())


class _Pinned(torch.Tensor):
    """a CPU tensor that passes for page-locked memory (no CPU-only process can pin one)"""
    def is_pinned(self, *a, **kw):
        return True


class _Dev(torch.Tensor):
    """... and one that passes for a device tensor"""
    is_cuda = property(lambda self: True)


def _same_refusal(ref_call, new_call, fix=lambda s: s):
    with pytest.raises(ValueError) as want:
        ref_call()
    with pytest.raises(ValueError) as got:
        new_call()
    assert str(got.value) == fix(str(want.value))


@pytest.mark.parametrize("name", ["bsrnn_xxt", "fspen", "lisennet"])
def test_step_pool_streams_ctl_raises_what_step_streams_with_tables_raises(monkeypatch, name):
    ref, eng = hip_engine("fe_b"), hip_engine(name)
    _no_native(monkeypatch, ref)
    _no_native(monkeypatch, eng)
    st = torch.zeros(1)
    gain_ok, lv_ok = torch.zeros(8).as_subclass(_Dev), torch.zeros(8, 4).as_subclass(_Pinned)
    bad_tables = [dict(min_gain=torch.zeros(7).as_subclass(_Dev)), dict(min_gain=torch.zeros(8, dtype=torch.float64).as_subclass(_Dev)),
                  dict(min_gain=[0.0] * 8), dict(levels=torch.zeros(8, 3).as_subclass(_Dev)), dict(levels=torch.zeros(4, 8).t().as_subclass(_Dev)),
                  dict(min_gain=torch.zeros(8)), dict(levels=torch.zeros(8, 4)), dict(min_gain=gain_ok, levels=torch.zeros(8, 4))]
    bad_desc = [[(0, 1, 0, 0), (0, 1, 256, 256)], [(8, 1, 0, 0)], [(0, 3, 0, 0)], [(0, 2, 513, 0)], [(0, 2, 0, 600)], []]
    fix = lambda t: t.replace("fe_step_streams_ctl", "fe_step_pool_streams_ctl")
    for pinned in (False, True):
        old = ref.step_streams_pinned if pinned else ref.step_streams
        new = eng.step_pool_streams_ctl_pinned if pinned else eng.step_pool_streams_ctl
        a = torch.zeros(1024, dtype=torch.int16).as_subclass(_Pinned if pinned else _Dev)
        ok = [(0, 1, 0, 0)]
        for tables in bad_tables:
            _same_refusal(lambda: old(a, st, 8, ok, a, T_max=2, **tables), lambda: new(a, st, 8, ok, a, T_max=2, **tables), fix)
        for desc in bad_desc:
            _same_refusal(lambda: old(a, st, 8, desc, a, T_max=2, min_gain=gain_ok, levels=lv_ok),
                          lambda: new(a, st, 8, desc, a, T_max=2, min_gain=gain_ok, levels=lv_ok), fix)
        f = torch.zeros(1024)
        _same_refusal(lambda: old(f, st, 8, ok, f, min_gain=gain_ok), lambda: new(f, st, 8, ok, f, min_gain=gain_ok), fix)      # unpinned / not on the device
        _same_refusal(lambda: old(a, st, 8, ok, a, T_max=0, levels=lv_ok), lambda: new(a, st, 8, ok, a, T_max=0, levels=lv_ok), fix)
        for tables in (dict(min_gain=gain_ok, levels=lv_ok), dict(levels=lv_ok), dict(min_gain=gain_ok), dict()):
            with pytest.raises(_lib.FEError, match="needs a GPU"):         # a valid call gets as far as the device requirement
                new(a, st, 8, ok, a, T_max=2, **tables)
        for kw in (dict(bank=torch.zeros(8, dtype=torch.int32)), dict(chunk=True)):
            with pytest.raises(TypeError):                                  # no bank or chunk parameters
                new(a, st, 8, ok, a, **kw)


# ------------------------------------------------------------------ FamilyPacketPool with the engine calls recorded
class _Cfg:
    hop_size = 256


class _StubEngine:
    """what a packet pool needs of an Engine: every packet call copies the input hops to their output place, writes the level rows an
    identity model would meter, and is recorded with the tables it was handed"""
    def __init__(self, cfg=None):
        self.cfg = cfg if cfg is not None else _Cfg()
        self.calls = []
        self.record_floats = 1

    def new_state(self, B):
        return torch.zeros(B)

    def reset_slots(self, state, capacity, slots):
        pass

    def new_pinned(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype)

    def synchronize(self):
        pass

    def export_slots(self, state, capacity, slots, out=None):
        return torch.zeros(len(slots), 1)

    def import_slots(self, state, capacity, slots, records):
        pass

    def _packets(self, call, wav_in, state, capacity, desc, wav_out, T_max, ctl):
        assert wav_in.dtype == wav_out.dtype == torch.int16
        H = self.cfg.hop_size
        fin, fout = wav_in.view(-1), wav_out.view(-1)
        for slot, hops, i0, o0 in desc:
            fout[o0:o0 + hops * H] = fin[i0:i0 + hops * H]
            if ctl.get("levels") is not None:
                x = fin[i0:i0 + hops * H].double() / 32768.0
                ctl["levels"][slot] = torch.tensor([float((x * x).sum()), float(x.abs().max())] * 2)
        self.calls.append((call, list(desc), ctl.get("min_gain").clone() if ctl.get("min_gain") is not None else None, sorted(ctl)))
        return wav_out

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, **kw):
        return self._packets("step_streams_pinned", wav_in, state, capacity, desc, wav_out, T_max, kw)

    def step_pool_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, **kw):
        assert not kw, "the plain packet step takes no tables"
        return self._packets("step_pool_streams_pinned", wav_in, state, capacity, desc, wav_out, T_max, kw)

    def step_pool_streams_ctl_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, *, min_gain=None, levels=None):
        return self._packets("step_pool_streams_ctl_pinned", wav_in, state, capacity, desc, wav_out, T_max, dict(min_gain=min_gain, levels=levels))

    def step_streams(self, *a, **kw):
        raise AssertionError("the device-audio step is not a packet pool's")

    step_pool_streams = step_pool_streams_ctl = step_streams


def _pcm(n, seed):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3000).round().to(torch.int16)


BASELINES = [("bsrnn_xxt", "BSRNN"), ("bsrnn_s", "BSRNN"), ("fspen", "FSPEN"), ("lisennet", "LiSenNet")]


@pytest.mark.parametrize("name,call", [(n, "step_pool_streams_ctl_pinned") for n, _ in BASELINES] +
                         [("fe_b", "step_streams_pinned"), ("fe_dpt_t", "step_streams_pinned"), (None, "step_streams_pinned")])
def test_packet_ctl_step_names_the_familys_call(name, call):
    eng = _StubEngine(product_config(name) if name else None)
    assert packet_ctl_step(eng, pinned=True) == getattr(eng, call)
    assert packet_ctl_step(eng, pinned=False) == getattr(eng, call[:-len("_pinned")])


@pytest.mark.parametrize("name,family", BASELINES)
def test_a_baseline_family_pool_ticks_plain_until_a_control_is_in_use(name, family):
    eng = _StubEngine(product_config(name))
    H = eng.cfg.hop_size
    pool = FamilyPacketPool(eng, 3, ring_hops=4, T_max=2)
    a, b = pool.open(), pool.open()
    pool.push(a, _pcm(H, 1))
    pool.push(b, _pcm(2 * H + 3, 2))
    R = 4 * H
    assert pool.tick() == [(a, 1, a * R, a * R), (b, 2, b * R, b * R)]
    assert eng.calls[-1] == ("step_pool_streams_pinned", [(a, 1, a * R, a * R), (b, 2, b * R, b * R)], None, [])
    with pytest.raises(RuntimeError, match="meters=True"):
        pool.levels(a)
    pool.set_suppression_limit(a, None)                                # lifting a limit never set: still no table, still the plain call
    pool.push(a, _pcm(H, 3))
    pool.tick()
    assert eng.calls[-1][0] == "step_pool_streams_pinned" and pool._gain is None
    pool.set_suppression_limit(b, -12.0)
    assert pool.suppression_limit(b) == pytest.approx(-12.0, abs=1e-5) and pool.suppression_limit(a) is None
    pool.push(a, _pcm(H, 4))
    assert pool.tick() == [(a, 1, a * R + 2 * H, a * R + 2 * H)]     # (the return value of tick() is what it was)
    call, _, gains, given = eng.calls[-1]
    assert call == "step_pool_streams_ctl_pinned" and given == ["levels", "min_gain"]
    assert gains.dtype == torch.float32 and gains.tolist() == [0.0, pytest.approx(10 ** (-12 / 20)), 0.0]
    with pytest.raises(ValueError, match="has a suppression limit"):   # catch_up keeps refusing a slot with a limit
        pool.catch_up(b, torch.zeros(1, 4 * H))


@pytest.mark.parametrize("name,family", BASELINES)
def test_a_baseline_family_pool_meters_and_carries_its_tables(name, family):
    eng = _StubEngine(product_config(name))
    H = eng.cfg.hop_size
    pool = FamilyPacketPool(eng, 3, ring_hops=8, T_max=2, meters=True)
    a, b = pool.open(), pool.open()
    assert pool.levels(a) == StreamLevels() and pool.levels(a).samples == 0
    pool.set_suppression_limit(b, -40.0)
    xa = _pcm(2 * H, 5)
    pool.push(a, xa)
    pool.push(b, _pcm(H, 6))
    pool.tick()
    call, _, gains, given = eng.calls[-1]
    assert call == "step_pool_streams_ctl_pinned" and given == ["levels", "min_gain"] and gains.tolist() == [0.0, pytest.approx(0.01), 0.0]
    fa = xa.double() / 32768.0
    la = pool.levels(a)
    assert la.samples == 2 * H and pool.levels(b).samples == H
    assert la.in_sumsq == pytest.approx(float((fa * fa).sum()), rel=1e-6) and la.in_peak == pytest.approx(float(fa.abs().max()), rel=1e-7)
    # meters alone (no limit ever set) is a control in use too
    metered = FamilyPacketPool(eng, 2, ring_hops=4, meters=True)
    s = metered.open()
    metered.push(s, _pcm(H, 7))
    metered.tick()
    assert eng.calls[-1][0] == "step_pool_streams_ctl_pinned" and eng.calls[-1][2] is None and metered.levels(s).samples == H
    # move, resize, adopt and a re-opened slot
    dst = FamilyPacketPool(eng, 4, ring_hops=8, T_max=2)
    dst.open()
    bits = float(pool._gain[b])
    new = pool.move(b, dst)
    assert new == 1 and float(dst._gain[new]) == bits and dst.suppression_limit(new) == pytest.approx(-40.0, abs=1e-5)
    dst.resize(6)
    assert dst._gain.numel() == 6 and float(dst._gain[new]) == bits and dst._gain.tolist()[2:] == [0.0] * 4
    pool.resize(5)
    assert pool._levels.shape == (5, 4) and pool.levels(a) == la
    c = pool.open()
    assert c == b and pool.suppression_limit(c) is None and pool.levels(c) == StreamLevels()
    got = dst.adopt(torch.zeros(1, 1))
    assert dst.suppression_limit(got[0]) is None
    with pytest.raises(ValueError, match=family):                      # a plain PacketPool of the family has no limit to carry the stream's
        dst.move(new, PacketPool(eng, 2, ring_hops=8))
    assert dst.suppression_limit(new) == pytest.approx(-40.0, abs=1e-5)


@pytest.mark.parametrize("name,family", BASELINES)
def test_a_baseline_family_pool_still_refuses_banks_and_the_backlog(name, family):
    eng = _StubEngine(product_config(name))
    with pytest.raises(ValueError, match=family):
        FamilyPacketPool(eng, 4, ring_hops=16, T_max=1, backlog_hops=8)
    pool = FamilyPacketPool(eng, 4, ring_hops=4, meters=True)
    s = pool.open()
    with pytest.raises(ValueError, match=family):
        pool.set_bank(s, 1)
    with pytest.raises(ValueError, match=family):
        pool.open(bank=1)
    assert pool.active == [s] and eng.calls == []
    pool.set_bank(s, 0)
    assert pool.bank(s) == 0
    with pytest.raises(ValueError, match=family):                      # ... and the plain PacketPool keeps refusing both controls
        PacketPool(eng, 4, ring_hops=4, meters=True)
    plain = PacketPool(eng, 4, ring_hops=4)
    with pytest.raises(ValueError, match=family):
        plain.set_suppression_limit(plain.open(), -20.0)


@pytest.mark.parametrize("name", ["fe_b", None])
def test_on_a_fastenhancer_engine_the_family_pool_is_packet_pool_call_for_call(name):
    logs = []
    for cls in (PacketPool, FamilyPacketPool):
        eng = _StubEngine(product_config(name) if name else None)
        H = eng.cfg.hop_size
        pool = cls(eng, 3, ring_hops=8, T_max=2, meters=True)
        a, b = pool.open(), pool.open()
        ticks = []
        for t in range(4):
            if t == 2:
                pool.set_suppression_limit(b, -20.0)
            pool.push(a, _pcm(H + 7, 10 + t))
            pool.push(b, _pcm(2 * H, 20 + t))
            ticks.append(pool.tick())
        logs.append((ticks, [(c[0], c[1], None if c[2] is None else c[2].tolist(), c[3]) for c in eng.calls], pool.levels(a), pool.levels(b)))
    assert logs[0] == logs[1] and all(c[0] == "step_streams_pinned" for c in logs[1][1])
    plain = FamilyPacketPool(_StubEngine(product_config(name) if name else None), 2, ring_hops=4)
    s = plain.open()
    plain.push(s, _pcm(256, 1))
    plain.tick()
    assert plain.engine.calls[-1][2:] == (None, [])


# ------------------------------------------------------------------ the oracle side of the GPU test
ORACLE_MODELS = ["bsrnn_xxt", "fspen", "lisennet"]


@pytest.mark.parametrize("name", ORACLE_MODELS)
def test_with_every_gain_off_the_composed_step_is_oracle_step(name):
    for dt in (np.float32, np.float64):
        cfg, sd, fused, orc = build_named_oracle(name, dt)
        H, B = cfg.hop_size, 3
        x = pco.reference(name)["x"][:, :2 * H].astype(dt)
        for gains in ([0.0] * B, [float("nan"), -1.0, 0.0]):
            comp, plain = orc.initialize_cache(B), orc.initialize_cache(B)
            for t in range(2):
                (o, *comp), share, *_ = pco.step(orc, x[:, t * H:(t + 1) * H], *comp, gains=gains)
                p, *plain = orc.step(x[:, t * H:(t + 1) * H], *plain)
                assert np.array_equal(o, p) and not share.any()
                assert len(comp) == len(plain) and all(np.array_equal(a, b) for a, b in zip(comp, plain))


@pytest.mark.parametrize("name", ORACLE_MODELS)
def test_the_composed_step_holds_the_contract_on_the_gpu_tests_inputs(name):
    ref = pco.reference(name)
    c = ref["compression"]
    m = pco.clamp_gain(pco.GAINS) ** c
    for t, (xc, yc, yl) in enumerate(ref["bins"]):
        xa, ya, la = (np.sqrt(v[..., 0].astype(np.float64) ** 2 + v[..., 1].astype(np.float64) ** 2) for v in (xc, yc, yl))
        assert xc.shape[1] == 257 and xc.shape[2] == 1
        for i, g in enumerate(pco.GAINS):
            assert (la[i] >= m[i] * xa[i] * (1 - 1e-6)).all(), f"{name} hop {t} stream {i}: a bin is below the floor"
            lifted = m[i] * xa[i] > ya[i]
            assert np.array_equal(yl[i][~lifted], yc[i][~lifted]), f"{name} hop {t} stream {i}: a bin the floor does not reach changed"
            assert lifted.mean() == pytest.approx(ref["shares"][t][i])
            if g == 0.0:
                assert not lifted.any()
            else:
                assert 0.10 < lifted.mean() < 0.90, f"{name} hop {t}: {lifted.mean():.0%} of the bins of the stream with gain {g} are lifted"
                # after the un-compress no bin leaves attenuated by more than g: |Y| >= g max(|X|, 1e-5)  (|X_c| = max(|X|, 1e-5)^(c-1) |X|)
                assert (la[i] ** (1.0 / c) >= g * xa[i] ** (1.0 / c) * (1 - 1e-6)).all()
    for i, g in enumerate(pco.GAINS):
        change = rms(ref["out"][i] - ref["plain"][i]) / rms(ref["plain"][i])
        print(f"pool_stream_ctl oracle {name} gain {g}: lifted {ref['shares'][:, i].min():.0%}-{ref['shares'][:, i].max():.0%} per hop, output change {change:.2e}")
        if g == 0.0:
            assert np.array_equal(ref["out"][i], ref["plain"][i])
        else:
            assert change > 1e-3, f"{name}: the limit of stream {i} changes nothing"
    # the limit is on the output path only: the model's caches and cache_stft are the plain step's
    for j, (a, b) in enumerate(zip(ref["caches"], ref["plain_caches"])):
        assert j == 1 or np.array_equal(a, b), f"{name}: cache {j} differs from the plain step's"


def test_the_floor_takes_the_inputs_phase_where_the_output_bin_vanishes_and_clamps_the_gain():
    x = np.array([[[[3.0, 4.0]], [[1.0, 0.0]], [[0.0, 0.0]], [[3.0, 4.0]]]])                  # [1, 4, 1, 2]
    y = np.array([[[[0.0, 0.0]], [[0.0, 2.0]], [[1e-30, 0.0]], [[0.3, -0.4]]]])
    for g, m in ((0.25, 0.5), (4.0, 1.0), (1e9, 1.0)):
        out, lifted = pco.floor(x, y, [g], 0.5 if g == 0.25 else 0.3)
        assert np.allclose(out[0, 0, 0], [m * 3.0, m * 4.0]) and lifted[0, 0, 0]          # |Y| = 0: m X
        assert np.array_equal(out[0, 1, 0], [0.0, 2.0]) and not lifted[0, 1, 0]           # |Y| above m |X|: unchanged
        assert np.array_equal(out[0, 2, 0], [0.0, 0.0]) and not lifted[0, 2, 0]           # |X| = 0: m X = 0
        assert np.allclose(out[0, 3, 0], [m * 5.0 * 0.6, m * 5.0 * -0.8]) and lifted[0, 3, 0]      # lifted to m |X| on Y's phase
    for g in (0.0, -1.0, float("nan")):
        out, lifted = pco.floor(x, y, [g], 0.3)
        assert np.array_equal(out, y) and not lifted.any()
