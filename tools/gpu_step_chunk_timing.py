#!/usr/bin/env python3
"""Few streams x many hops, wav -> wav with carried state: fe_step(B, T) (one workgroup walks a stream's T frames) against fe_step_chunk
(the frames on the time pipeline + one overlap-add launch), next to fe_spec_step walked and pipelined in the same run.
HIP events around each call, warm-up first (clocks ramped), median of the repeats.
usage: tools/gpu_step_chunk_timing.py [hops per call] [repeats] [shape ...]      (writes a table to stdout)"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import product_config  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from fastenhancer_amd.weights import default_state_dict  # noqa: E402


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 251
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 21
    names = sys.argv[3:] or ["fe_b", "fe_t", "fe_l", "fe_dpt_b"]
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}; T = {T} hops per call; median (min .. max) of {repeats} calls after 5 warm-up calls, HIP events, ms")
    print(f"# {'shape':9s} {'B':>2s} {'fe_step walk':>24s} {'fe_step_chunk':>24s} {'speed-up':>8s} | {'spec walk':>10s} {'spec pipe':>10s} {'speed-up':>8s} | chunk kernel")
    for name in names:
        cfg = product_config(name)
        eng = Engine(cfg, dev)
        eng.load_state_dict(default_state_dict(cfg, torch.Generator().manual_seed(1)))
        eng.set_offline_engine("frame_walk")          # (fe_spec_step: the frame walk and its time pipeline, not the time-batched engine)
        H = cfg.hop_size
        for B in (1, 8):
            x = 0.1 * torch.randn(B, T * H, device=dev)
            y = torch.empty_like(x)
            state = eng.new_state(B)
            work = torch.empty(eng.chunk_work_floats(B, T), device=dev)
            spec = 0.1 * torch.randn(B, cfg.F0 + 1, T, 2, device=dev)
            h = torch.zeros(eng.model_state_floats(B), device=dev)
            walk = median_ms(lambda: eng.step(x, state, y, T=T), 5, repeats)
            chunk = median_ms(lambda: eng.step_chunk(x, state, y, T=T, work=work), 5, repeats)
            kern = eng.last_step_kernel()
            eng.set_time_pipeline(0)
            swalk = median_ms(lambda: eng.spec_step(spec, h), 5, repeats)
            eng.set_time_pipeline(-1)
            spipe = median_ms(lambda: eng.spec_step(spec, h), 5, repeats)
            fmt = lambda r: f"{r[0]:8.3f} ({r[1]:.3f} .. {r[2]:.3f})"      # noqa: E731
            print(f"  {name:9s} {B:2d} {fmt(walk):>24s} {fmt(chunk):>24s} {walk[0] / chunk[0]:7.2f}x | {swalk[0]:10.3f} {spipe[0]:10.3f} {swalk[0] / spipe[0]:7.2f}x | {kern}")


if __name__ == "__main__":
    main()
