#!/usr/bin/env python3
"""Digests of what the time-pipelined entry points compute, on the GPU: one line per (configuration, call) with the sha256 of every
output and of the final state where the call has one.  The pipelined launches are reproducible bit for bit, so two builds compute the
same exactly when their lines agree - run it on both (FASTENHANCER_HIP_LIB selects a side build):

    python tools/pipe_digests.py                          # fe_b, fe_tk_b, fe_dpt_b, bsrnn_xt, fspen, lisennet
    FASTENHANCER_HIP_LIB=ab/lib_parent.so python tools/pipe_digests.py

Calls: fe_offline on the frame walk (2 x 40 frames), fe_spec_step (2 x 16 frames), fe_step_chunk (2 x 16 hops) and, for fe_b,
fe_step_streams_chunk (hops 16 and 9 of 16).  Each line ends with what fe_last_step_kernel reported."""
import hashlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import product_config  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from fastenhancer_amd.family import family_of  # noqa: E402

NAMES = ("fe_b", "fe_tk_b", "fe_dpt_b", "bsrnn_xt", "fspen", "lisennet")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:32]


def main():
    names = sys.argv[1:] or NAMES
    dev = torch.device("cuda:0")
    for name in names:
        cfg = product_config(name)
        eng = Engine(cfg, dev)
        eng.load_state_dict(family_of(cfg).default_state_dict(cfg, torch.Generator().manual_seed(7)))
        if hasattr(cfg, "rf_blocks"):       # FastEnhancer: the frame walk and its time pipeline, not the time-batched engine
            eng.set_offline_engine("frame_walk")
        g = torch.Generator().manual_seed(11)
        B, H, T = 2, cfg.hop_size, 16

        def line(call, tensors):
            torch.cuda.synchronize()
            print(f"{name:<9} {call:<22} {' '.join(sha(t) for t in tensors)}  {eng.last_step_kernel()}", flush=True)

        wav, spec = eng.offline(0.1 * torch.randn(B, 39 * H + 7, generator=g).to(dev))
        line("fe_offline", (wav, spec))
        h = torch.zeros(eng.model_state_floats(B), device=dev)
        eng.spec_step(0.1 * torch.randn(B, cfg.F0 + 1, 3, 2, generator=g).to(dev), h)       # (caches that are not all zeros)
        out = eng.spec_step(0.1 * torch.randn(B, cfg.F0 + 1, T, 2, generator=g).to(dev), h)
        line("fe_spec_step", (out, h))
        state = eng.new_state(B)
        eng.step(0.1 * torch.randn(B, 2 * H, generator=g).to(dev), state, T=2)
        y = eng.step_chunk(0.1 * torch.randn(B, T * H, generator=g).to(dev), state, T=T)
        line("fe_step_chunk", (y, state))
        if name == "fe_b":
            cap, count = 3, 2 * T * H
            state = eng.new_state(cap)
            eng.step(0.1 * torch.randn(cap, 2 * H, generator=g).to(dev), state, T=2)
            x, y = 0.1 * torch.randn(count, generator=g).to(dev), torch.zeros(count, device=dev)
            eng.step_streams_chunk(x, state, cap, [(2, 16, 0, 0), (0, 9, T * H, T * H)], y, T_max=T)
            line("fe_step_streams_chunk", (y, state))


if __name__ == "__main__":
    main()
