"""The C ABI's host-side size and name queries, pinned to a fixture (no GPU): the state, work-buffer and debug-buffer sizes, the debug
stage table, the flop count and the weight section table of one handle per family and FastEnhancer variant.  These are what a caller
allocates from, so a change to the host code that moves any of them shows here.  Without a GPU a handle counts 256 CUs, the MI355X's
count, so the fixture holds on both kinds of machine.

Regenerate (only when a size is meant to change): python tests/test_cpu_host_queries.py"""
import ctypes
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_queries.json")

FE_NAMES = ("fe_b", "fe_l", "fe_tk_b", "fe_ln_b", "fe_dprnn_b", "fe_dpt_b", "fe_nc", "fe48_b_h480")
BSRNN_NAMES = ("bsrnn_xt", "bsrnn_xxt", "bsrnn_t", "bsrnn_s")
NAMES = FE_NAMES + BSRNN_NAMES + ("fspen", "lisennet")

STATE_B = (1, 3, 256, 257, 2049)
WORK_B = (1, 3, 8, 16, 600)
WORK_HOPS = (1, 4, 37, 250)          # Tw = hops * hop + 7: from below the time pipeline's 4 frames to 4 s at 16 kHz
CHUNK_B = (1, 3, 16, 200)            # streams (fe_step_chunk: B, fe_step_streams_chunk: n) ...
CHUNK_T = (3, 4, 5, 37, 250)         # ... and hops of the time-pipelined streaming chunks: from below the pipeline's 4 frames on


def make_engine(name):
    from common import hip_engine
    return hip_engine(name)


def host_queries(name):
    eng = make_engine(name)
    lib, h, hop = eng.lib, eng._h, eng.cfg.hop_size
    out = {"state_floats": {str(B): lib.fe_state_floats(h, B) for B in STATE_B}, "offline_work_floats": {}, "offline_ragged_work_floats": {}}
    for B in WORK_B:
        for n in WORK_HOPS:
            key = f"{B}x{n * hop + 7}"
            out["offline_work_floats"][key] = lib.fe_offline_work_floats(h, B, n * hop + 7)
            out["offline_ragged_work_floats"][key] = lib.fe_offline_ragged_work_floats(h, B, n * hop + 7)
    out["step_chunk_work_floats"] = {f"{B}x{T}": lib.fe_step_chunk_work_floats(h, B, T) for B in CHUNK_B for T in CHUNK_T}
    out["step_streams_chunk_work_floats"] = {f"{n}x{T}": lib.fe_step_streams_chunk_work_floats(h, n, T) for n in CHUNK_B for T in CHUNK_T}
    out["debug_stages"] = lib.fe_debug_stages(h)
    out["debug_floats"] = lib.fe_debug_floats(h)
    stages = []
    for i in range(out["debug_stages"]):
        nm, r, c, off = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert lib.fe_debug_stage(h, i, ctypes.byref(nm), ctypes.byref(r), ctypes.byref(c), ctypes.byref(off)) == 0
        stages.append([nm.value.decode(), r.value, c.value, off.value])
    out["debug_stage"] = stages
    out["flops_per_frame"] = lib.fe_flops_per_frame(h)
    out["weight_floats"] = lib.fe_weight_floats(h)
    out["sections"] = [[n, off, cnt] for n, off, cnt in eng.sections]
    return out


def write_fixture():
    with open(FIXTURE, "w") as f:
        json.dump({name: host_queries(name) for name in NAMES}, f, indent=0, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("name", NAMES)
def test_host_queries_match_the_fixture(name):
    want = json.load(open(FIXTURE))[name]
    have = json.loads(json.dumps(host_queries(name)))
    for key in want:
        assert have[key] == want[key], (name, key)
    assert set(have) == set(want)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    write_fixture()
