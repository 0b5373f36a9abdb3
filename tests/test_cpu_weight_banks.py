"""CPU tests of the weight banks (fe_set_weight_banks / fe_weight_banks / fe_load_weights_bank / fe_step_streams_banked[_pinned], Engine's
bank= arguments, serving.PacketPool's open(bank=) / set_bank / bank): the ABI, the argument checks that come before any device work - the
banked steps make those of fe_step_streams_ctl - and PacketPool's bookkeeping of the bank table with the engine call replaced by a stub."""
import ctypes
import os
import re
from ctypes import c_void_p

import pytest
import torch

from common import BSRNN_KWARGS, product_config
from fastenhancer_amd import _lib
from fastenhancer_amd.config import BSRNNConfig
from fastenhancer_amd.engine import Engine
from fastenhancer_amd.serving import PacketPool

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastenhancer_hip.h")
FE_OK, FE_ERR_INVALID_ARG, FE_ERR_UNSUPPORTED_CONFIG, FE_ERR_NO_WEIGHTS = 0, -1, -2, -4
FE_MAX_WEIGHT_BANKS = 64
P = c_void_p(0x1000)         # a non-null, 16-byte aligned pointer that is never dereferenced: every call below fails before touching memory
NULL = c_void_p(0)
ENTRY_POINTS = ("fe_step_streams_banked", "fe_step_streams_banked_pinned")


def _err():
    return _lib.load().fe_last_error().decode()


def _call(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0, min_gain=P, levels=P, bank=P):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, min_gain, levels, bank, NULL)


def _call_ctl(lib, fn, h, wav_in=P, in_count=1024, state=P, capacity=4, desc=P, wav_out=P, out_count=1024, n=1, T_max=1, fmt=0, min_gain=P, levels=P):
    return getattr(lib, fn)(h, wav_in, in_count, state, capacity, desc, wav_out, out_count, n, T_max, fmt, min_gain, levels, NULL)


def _baseline_engines():
    return {"BSRNN": Engine(BSRNNConfig.from_model_kwargs(**BSRNN_KWARGS["bsrnn_xt"][0]), None), "FSPEN": Engine(product_config("fspen"), None),
            "LiSenNet": Engine(product_config("lisennet"), None), "noncausal": Engine(product_config("fe_nc"), None)}


# ------------------------------------------------------------------ the ABI
def test_the_header_declares_the_bank_symbols_and_they_are_bound():
    src = open(HEADER).read()
    assert re.search(r"#define FE_MAX_WEIGHT_BANKS %d\b" % FE_MAX_WEIGHT_BANKS, src)
    lib = _lib.load()
    for fn in ("fe_set_weight_banks", "fe_weight_banks", "fe_load_weights_bank") + ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % fn, src), fn
        assert fn in _lib.SYMBOLS and hasattr(lib, fn)
    for fn in ENTRY_POINTS:           # the bank table sits between the two ctl tables and the stream
        restype, argtypes = _lib.SYMBOLS[fn]
        ctl = _lib.SYMBOLS[fn.replace("_banked", "_ctl")][1]
        assert restype is ctypes.c_int and argtypes == ctl[:-1] + [c_void_p] + ctl[-1:]
    assert _lib.SYMBOLS["fe_load_weights_bank"][1] == [c_void_p, ctypes.c_int] + _lib.SYMBOLS["fe_load_weights"][1][1:]


# ------------------------------------------------------------------ fe_set_weight_banks / fe_weight_banks
def test_a_new_handle_has_one_bank_and_the_count_is_range_checked():
    eng = Engine(product_config("fe_b"), None)
    assert eng.lib.fe_weight_banks(eng._h) == 1 and eng.weight_banks == 1
    assert eng.lib.fe_weight_banks(NULL) == 0
    for bad in (0, -1, FE_MAX_WEIGHT_BANKS + 1):
        assert eng.lib.fe_set_weight_banks(eng._h, bad, NULL) == FE_ERR_INVALID_ARG, bad
        assert "n_banks %d" % bad in _err() and "FE_MAX_WEIGHT_BANKS" in _err(), _err()
        assert eng.weight_banks == 1
    assert eng.lib.fe_set_weight_banks(NULL, 2, NULL) == FE_ERR_INVALID_ARG and "null handle" in _err()
    with pytest.raises(_lib.FEError, match="n_banks 0"):
        eng.set_weight_banks(0)
    # nothing is loaded: changing the count needs no device work
    for n in (3, FE_MAX_WEIGHT_BANKS, 1):
        eng.set_weight_banks(n)
        assert eng.weight_banks == n


@pytest.mark.parametrize("name", ["fe_t", "fe_tk_b", "fe_ln_b", "fe_dprnn_b", "fe_dpt_b"])
def test_every_streaming_model_of_the_family_takes_banks(name):
    eng = Engine(product_config(name), None)
    eng.set_weight_banks(2)
    assert eng.weight_banks == 2


def test_more_than_one_bank_is_refused_for_the_other_families_by_name():
    for family, eng in _baseline_engines().items():
        assert eng.lib.fe_set_weight_banks(eng._h, 1, NULL) == FE_OK, family
        for n in (2, FE_MAX_WEIGHT_BANKS):
            assert eng.lib.fe_set_weight_banks(eng._h, n, NULL) == FE_ERR_UNSUPPORTED_CONFIG, family
            assert family in _err() and "fe_set_weight_banks" in _err(), _err()
        assert eng.weight_banks == 1
        assert eng.lib.fe_set_weight_banks(eng._h, 0, NULL) == FE_ERR_INVALID_ARG, "the range check comes first"


# ------------------------------------------------------------------ fe_load_weights_bank
def test_load_weights_bank_checks_bank_blob_and_size_before_any_device_work():
    eng = Engine(product_config("fe_b"), None)
    n = eng.weight_floats
    load = eng.lib.fe_load_weights_bank
    for bank in (-1, 1, 2 ** 30):
        assert load(eng._h, bank, P, n, NULL) == FE_ERR_INVALID_ARG and "bank %d outside [0, 1)" % bank in _err(), _err()
    eng.set_weight_banks(3)
    for bank in (-1, 3):
        assert load(eng._h, bank, P, n, NULL) == FE_ERR_INVALID_ARG and "bank %d outside [0, 3)" % bank in _err(), _err()
    for bank in (0, 2):
        assert load(eng._h, bank, NULL, n, NULL) == FE_ERR_INVALID_ARG and "null argument" in _err()
        assert load(eng._h, bank, P, n - 1, NULL) == FE_ERR_INVALID_ARG and "blob has %d floats, expected %d" % (n - 1, n) in _err(), _err()
    assert load(NULL, 0, P, n, NULL) == FE_ERR_INVALID_ARG and "null argument" in _err()
    # fe_load_weights is bank 0 of the same function: the same refusals, word for word
    assert eng.lib.fe_load_weights(eng._h, P, n + 4, NULL) == FE_ERR_INVALID_ARG
    text = _err()
    assert load(eng._h, 0, P, n + 4, NULL) == FE_ERR_INVALID_ARG and _err() == text


def test_engine_checks_the_bank_before_it_touches_the_checkpoint():
    eng = Engine(product_config("fe_t"), None)
    eng.set_weight_banks(2)
    for bad in (-1, 2):
        with pytest.raises(ValueError, match=r"bank %d is outside \[0, 2\)" % bad):
            eng.load_state_dict({}, bank=bad)
        with pytest.raises(ValueError, match="outside"):
            eng.load_blob(torch.zeros(1), bank=bad)
    with pytest.raises(TypeError):
        eng.load_blob(torch.zeros(1), bank=0.5)


# ------------------------------------------------------------------ the banked steps: the argument checks of fe_step_streams_ctl
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_banked_entry_points_refuse_a_null_handle(fn):
    assert _call(_lib.load(), fn, NULL) == FE_ERR_INVALID_ARG
    assert "null handle" in _err()


@pytest.mark.parametrize("bank", [P, NULL], ids=["table", "null"])
@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_banked_entry_points_give_the_argument_errors_of_the_ctl_step(fn, bank):
    eng = Engine(product_config("fe_b"), None)
    eng.set_weight_banks(2)
    ctl = fn.replace("_banked", "_ctl")
    bad = [dict(wav_in=NULL), dict(state=NULL), dict(desc=NULL), dict(wav_out=NULL), dict(n=0), dict(n=-1), dict(n=5), dict(capacity=0),
           dict(T_max=0), dict(T_max=-2), dict(in_count=0), dict(out_count=0), dict(fmt=2), dict(fmt=-1), dict(fmt=16),
           dict(levels=c_void_p(0x1004)), dict(levels=c_void_p(0x1008))]
    for kw in bad:
        want = _call_ctl(eng.lib, ctl, eng._h, **kw)
        want_text = _err()
        assert want == FE_ERR_INVALID_ARG
        assert _call(eng.lib, fn, eng._h, bank=bank, **kw) == want, kw
        assert _err() == want_text.replace(ctl + ":", fn + ":"), (kw, _err(), want_text)
    # good arguments, nothing loaded: readiness comes after the arguments, as in the ctl step
    assert _call(eng.lib, fn, eng._h, bank=bank) == FE_ERR_NO_WEIGHTS
    assert _call_ctl(eng.lib, ctl, eng._h) == FE_ERR_NO_WEIGHTS


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_banked_entry_points_give_the_family_refusals_of_the_ctl_step(fn):
    ctl = fn.replace("_banked", "_ctl")
    for family, eng in _baseline_engines().items():
        assert _call_ctl(eng.lib, ctl, eng._h) == FE_ERR_UNSUPPORTED_CONFIG
        want_text = _err()
        assert _call(eng.lib, fn, eng._h) == FE_ERR_UNSUPPORTED_CONFIG, family
        assert _err() == want_text.replace(ctl + ":", fn + ":"), (family, _err())
        assert ("the noncausal model has no streaming step" if family == "noncausal" else "FastEnhancer family") in _err()


def test_engine_checks_the_bank_table_before_any_device_call():
    for t, match in [(torch.zeros(7, dtype=torch.int32), r"bank must be a contiguous int32 tensor \[8\]"),
                     (torch.zeros(8, dtype=torch.int64), "bank must be a contiguous int32"),
                     (torch.zeros(8), "bank must be a contiguous int32"),
                     ([0] * 8, "bank must be a contiguous int32"),
                     (torch.zeros(16, dtype=torch.int32)[::2], "bank must be a contiguous int32"),
                     (torch.zeros(8, dtype=torch.int32), "bank must be a device tensor or a CPU tensor in page-locked memory")]:
        with pytest.raises(ValueError, match=match):
            Engine._bank_table(t, 8)
    assert Engine._bank_table(None, 8) is None


# ------------------------------------------------------------------ PacketPool with the engine stubbed
class _Cfg:
    hop_size = 256


class _StubEngine:
    """what PacketPool needs of an Engine (device None): the launch copies the input hops to their output place and records the tables it got"""
    cfg = _Cfg()
    device = None
    record_floats = 1

    def __init__(self, weight_banks=1):
        self.weight_banks = weight_banks
        self.calls = []

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

    def step_streams_pinned(self, wav_in, state, capacity, desc, wav_out, T_max=1, **ctl):
        H = self.cfg.hop_size
        fin, fout = wav_in.view(-1), wav_out.view(-1)
        for slot, hops, i0, o0 in desc:
            fout[o0:o0 + hops * H] = fin[i0:i0 + hops * H]
        self.calls.append((list(desc), ctl["bank"].clone() if ctl.get("bank") is not None else None, sorted(ctl)))
        return wav_out


def _pcm(n, seed):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3000).round().to(torch.int16)


def test_a_pool_that_names_no_bank_but_0_launches_what_it_launched_before():
    eng = _StubEngine(weight_banks=3)
    pool = PacketPool(eng, 3, ring_hops=4)
    a = pool.open()
    b = pool.open(bank=0)
    pool.set_bank(a, 0)
    assert pool._bank is None and pool.bank(a) == 0 and pool.bank(b) == 0
    pool.push(a, _pcm(256, 1))
    assert pool.tick() == [(a, 1, 0, 0)]
    assert eng.calls[-1][1:] == (None, []), "no bank table, no ctl table: plain fe_step_streams_pinned"
    pool.set_bank(b, 2)
    assert pool._bank.dtype == torch.int32 and pool._bank.tolist() == [0, 2, 0]
    pool.push(a, _pcm(256, 2))
    assert pool.tick() == [(a, 1, 256, 256)]
    assert eng.calls[-1][2] == ["bank"] and eng.calls[-1][1].tolist() == [0, 2, 0]


def test_open_and_set_bank_refuse_banks_the_engine_does_not_have():
    eng = _StubEngine(weight_banks=3)
    pool = PacketPool(eng, 2, ring_hops=4)
    for bad in (-1, 3, 2 ** 30, 1.0, True, None):
        with pytest.raises(ValueError, match=r"outside the engine's banks \[0, 3\)"):
            pool.open(bank=bad)
    assert pool.active == [], "a refused open() opens nothing"
    s = pool.open(bank=2)
    assert pool.bank(s) == 2
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="outside the engine's banks"):
            pool.set_bank(s, bad)
    assert pool.bank(s) == 2
    with pytest.raises(ValueError, match="not open"):
        pool.set_bank(1, 0)
    with pytest.raises(ValueError, match="not open"):
        pool.bank(1)
    # an engine without banks (or a stub that knows nothing of them) has bank 0 only
    one = PacketPool(_StubEngine(), 1, ring_hops=4)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        one.open(bank=1)
    # a slot that is handed out again starts on the bank its open() names
    pool.close(s)
    assert pool.bank(pool.open()) == 0


def test_resize_move_and_adopt_carry_or_reset_the_bank():
    eng = _StubEngine(weight_banks=4)
    pool = PacketPool(eng, 3, ring_hops=4)
    a, b, c = pool.open(bank=1), pool.open(), pool.open(bank=3)
    pool.resize(6)
    assert pool._bank.numel() == 6 and pool._bank.tolist() == [1, 0, 3, 0, 0, 0] and pool._bank.dtype == torch.int32
    assert [pool.bank(s) for s in (a, b, c)] == [1, 0, 3]
    pool.close(b)
    pool.resize(3)
    assert pool._bank.tolist() == [1, 0, 3]
    # move: the bank goes along; a destination engine with fewer banks refuses before anything is copied
    dst = PacketPool(eng, 2, ring_hops=4)
    new = pool.move(c, dst)
    assert dst.bank(new) == 3 and c not in pool.active
    small = PacketPool(_StubEngine(weight_banks=1), 2, ring_hops=4)
    pool.push(a, _pcm(100, 3))
    with pytest.raises(ValueError, match=r"bank 1 is outside the engine's banks \[0, 1\)"):
        pool.move(a, small)
    assert a in pool.active and small.active == [] and pool._pushed[a] == 100, "a refused move changes nothing"
    plain = pool.open()
    assert small.bank(pool.move(plain, small)) == 0 and small._bank is None
    # adopt: on bank 0, also in a slot whose last stream ran elsewhere
    dst.close(new)
    (s,) = dst.adopt(torch.zeros(1, 1))
    assert s == new and dst.bank(s) == 0
