"""The 512-thread per-hop kernel (fe_frame8_kernel, csrc/fe_frame8.hip.h) keeps its bits.

tests/golden/wg8_bits_fe_b.json holds sha256 digests of wav_out and of the whole state buffer after every hop of a few small runs of
FastEnhancer_B on the seeded default checkpoint, one run per instantiation of the kernel: step, step_slots with one empty slot,
step_slots_pinned, step_streams_pinned in float32 and in int16 PCM with one stream that has no hop, two weight banks, and the persistent walk
(more streams than CUs).  tools/gen_wg8_bits.py wrote it with the library of the commit BEFORE the kernel's bookkeeping instructions were cut
("VALU diet"); a change of the kernel that is meant to leave every floating-point operation alone must reproduce every digest.

2 streams x 3 hops: the state is carried from hop to hop, and three hops see both parities of the frame counter.  The kernel is chosen with
set_step_kernel and the name of the instantiation that ran is part of the fixture.  run_cases() below is shared with the generator, so that
fixture and test cannot drift apart."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from common import hip_model
from test_gpu_weight_banks import _checkpoints

pytestmark = pytest.mark.gpu

NAME = "fe_b"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wg8_bits_fe_b.json")
STREAMS, HOPS = 2, 3
PERSIST_EXTRA, PERSIST_HOPS = 3, 2


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _noise(rows, n, seed):
    return torch.from_numpy((0.1 * np.random.default_rng(seed).standard_normal((rows, n))).astype(np.float32))


def _pcm(x):
    return (x * 32768).round().clamp(-32768, 32767).to(torch.int16)


def _engine(banks=0):
    """the seeded default checkpoint; banks > 0: bank k holds the checkpoint of seed + k (bank 0 = the default one)"""
    if not banks:
        return hip_model(NAME, device=_dev()).engine
    _, sds = _checkpoints(NAME)
    eng = hip_model(NAME, device=_dev(), load=False).engine
    eng.set_weight_banks(banks)
    for k in range(banks):
        eng.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sds[k].items()}, bank=k)
    return eng


def _hops(eng, n_hops, cap, launch):
    """n_hops launches from a zero state of `cap` streams: [{"kernel", "wav_out", "state"}] per hop"""
    state, out = eng.new_state(cap), []
    for t in range(n_hops):
        y = launch(t, state)
        torch.cuda.synchronize()
        out.append({"kernel": eng.last_step_kernel(), "wav_out": _sha(y), "state": _sha(state)})
    return out


def run_cases(cus=None):
    """-> {"cus": the CU count the persistent case was sized for, "cases": {name: [per-hop digests]}}"""
    dev = _dev()
    cus = int(cus or torch.cuda.get_device_properties(dev).multi_processor_count)
    eng = _engine()
    H = eng.cfg.hop_size
    cases = {}
    eng.set_step_kernel("wg8")
    try:
        x = _noise(STREAMS, HOPS * H, 1).to(dev)
        cases["step"] = _hops(eng, HOPS, STREAMS, lambda t, st: eng.step(x[:, t * H:(t + 1) * H], st, T=1))

        # three rows, the middle one on no slot: its output row is zero and no state is touched
        cap, slots = 4, torch.tensor([2, -1, 0], dtype=torch.int32, device=dev)
        x3 = _noise(3, HOPS * H, 2).to(dev)
        cases["step_slots"] = _hops(eng, HOPS, cap, lambda t, st: eng.step_slots(x3[:, t * H:(t + 1) * H].contiguous(), st, cap, slots, T=1))

        xp = _noise(STREAMS, HOPS * H, 3)
        def slots_pinned(t, st):
            xi = xp[:, t * H:(t + 1) * H].contiguous().pin_memory()
            return eng.step_slots_pinned(xi, st, cap, [3, 1], T=1)
        cases["step_slots_pinned"] = _hops(eng, HOPS, cap, slots_pinned)

        # packet audio from page-locked memory: slots 3 and 0 advance one hop, slot 1 has no hop (nothing of it is read or written)
        for fmt, dtype in (("f32", torch.float32), ("s16", torch.int16)):
            xs = _noise(3, HOPS * H, 4)
            xs = (_pcm(xs) if dtype == torch.int16 else xs).pin_memory()
            row = HOPS * H
            def streams_pinned(t, st):
                y = torch.zeros(3 * H, dtype=dtype).pin_memory()
                desc = [(3, 1, 0 * row + t * H, 0), (1, 0, 1 * row + t * H, H), (0, 1, 2 * row + t * H, 2 * H)]
                return eng.step_streams_pinned(xs.view(-1), st, cap, desc, y, T_max=1)
            cases[f"step_streams_pinned_{fmt}"] = _hops(eng, HOPS, cap, streams_pinned)

        # the persistent walk: more streams than CUs, every workgroup's first stream and three second streams
        n = cus + PERSIST_EXTRA
        eng.set_step_kernel("wg8_persist")
        eng.set_option("low_lds_companion", 0)
        xl = _noise(n, PERSIST_HOPS * H, 5).to(dev)
        cases["persistent"] = _hops(eng, PERSIST_HOPS, n, lambda t, st: eng.step(xl[:, t * H:(t + 1) * H], st, T=1))
    finally:
        eng.set_step_kernel("wg8")
        eng.set_option("low_lds_companion", 1)

    # two weight banks: streams of one launch on two checkpoints
    engb = _engine(banks=2)
    engb.set_step_kernel("wg8")
    cap = 4
    table = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device=dev)
    xb = _noise(STREAMS, HOPS * H, 6).to(dev).contiguous()
    row = HOPS * H
    def banked(t, st):
        y = torch.zeros(STREAMS * H, device=dev)
        desc = [(0, 1, 0 * row + t * H, 0), (2, 1, 1 * row + t * H, H)]
        return engb.step_streams(xb.view(-1), st, cap, desc, y, T_max=1, bank=table)
    cases["two_banks"] = _hops(engb, HOPS, cap, banked)
    return {"cus": cus, "cases": cases}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(golden):
    return run_cases(cus=golden["cus"])["cases"]


CASES = ["step", "step_slots", "step_slots_pinned", "step_streams_pinned_f32", "step_streams_pinned_s16", "two_banks", "persistent"]


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    for name in CASES:
        assert len(golden["cases"][name]) == (PERSIST_HOPS if name == "persistent" else HOPS)


@pytest.mark.parametrize("case", CASES)
def test_wg8_kernel_reproduces_the_recorded_bits(case, golden, got):
    want, have = golden["cases"][case], got[case]
    assert len(want) == len(have)
    for t, (w, h) in enumerate(zip(want, have)):
        assert "fe_frame8_kernel" in h["kernel"], f"{case}, hop {t}: {h['kernel']} is not the 512-thread per-hop kernel"
        if case == "persistent":
            assert "persistent" in h["kernel"], f"{case}, hop {t}: {h['kernel']}"
        assert h["kernel"] == w["kernel"], f"{case}, hop {t}: ran {h['kernel']}, the fixture was written by {w['kernel']}"
        assert h["wav_out"] == w["wav_out"], f"{case}, hop {t}: wav_out differs from the recorded bits"
        assert h["state"] == w["state"], f"{case}, hop {t}: the state differs from the recorded bits"
    # the digests move from hop to hop: the runs are not silent
    assert len({h["wav_out"] for h in have}) == len(have) and len({h["state"] for h in have}) == len(have)
