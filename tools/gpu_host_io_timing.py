#!/usr/bin/env python3
"""Streaming steps whose audio lives in host memory, against the device-resident step, in one run on one GPU:
  dev     fe_step, audio already on the device (what bench.py measures);
  host    fe_step_host, one call of T hops: copy-in, kernel and copy-out on the handle's copy streams (pinned buffers);
  pinned  fe_step_pinned: one launch whose kernel reads and writes the pinned host audio itself;
  copies  the caller's own pinned H2D copy, fe_step_slots on a state of the same size (what StreamPool.step runs, with the slot list
          already on the device), and the D2H copy back.
A second table steps n of 1024 slots: fe_step_slots_pinned against copies + fe_step_slots and fe_step_slots on device audio.
Device events around `--iters` calls after `--warmup` calls of each form; the forms alternate in rounds (`--rounds`), each cell is the median
over rounds, in us per call and M frames/s (frames = streams x T).  Writes the tables to stdout and to `--out`.
   python tools/gpu_host_io_timing.py [--out profiles/host_io_timing.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import build_oracle, product_config  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from fastenhancer_amd.serving import StreamPool  # noqa: E402

CASES = [("fe_b", 256, 1), ("fe_b", 256, 4), ("fe_b", 2048, 1), ("fe_b", 2048, 4), ("fe_t", 256, 1)]


def _time(forms, args):
    """forms: [callable] -> (median us per call, spread %) of each, alternating in rounds"""
    times = [[] for _ in forms]
    for _ in range(args.rounds):
        for i, f in enumerate(forms):
            for _ in range(args.warmup):
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            e1.synchronize()
            times[i].append(1000.0 * e0.elapsed_time(e1) / args.iters)
    return [(float(np.median(t)), 100.0 * (max(t) - min(t)) / float(np.median(t))) for t in times]


def _cell(us_spread, frames):
    us, sp = us_spread
    return f"{us:>9.2f} ({sp:>2.0f}%) {frames / us:>6.2f}"


def _engine(name, dev, cache={}):
    if name not in cache:
        cfg, sd, fused, orc = build_oracle(name)
        eng = Engine(product_config(name), dev)
        eng.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        cache[name] = eng
    return cache[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1024)
    ap.add_argument("--n", default="64,256,512")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = [f"# host-audio streaming steps: median over {args.rounds} alternating rounds of {args.iters} calls (device events, {args.warmup} warm-up "
             f"calls per form and round); each cell: us per call (spread of the rounds), M frames/s (streams x T per call)",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'model':>6} {'B':>5} {'T':>2} {'dev: fe_step':>24} {'host: fe_step_host':>24} {'pinned: fe_step_pinned':>24} {'copies + step_slots':>24}"
             f"   kernels dev | pinned"]
    print("\n".join(lines), flush=True)
    for name, B, T in CASES:
        eng = _engine(name, dev)
        H = eng.cfg.hop_size
        xh = (0.1 * torch.randn(B, T * H, generator=gen)).pin_memory()
        yh = torch.empty(B, T * H).pin_memory()
        xd, yd = xh.to(dev), torch.empty(B, T * H, device=dev)
        state = eng.new_state(B)
        pool = StreamPool(eng, B)
        slots_d = torch.tensor([pool.open() for _ in range(B)], dtype=torch.int32, device=dev)
        xp, yp = torch.empty(B, T * H, device=dev), torch.empty(B, T * H, device=dev)

        def f_dev():
            eng.step(xd, state, wav_out=yd, T=T)

        def f_host():
            eng.step_host(xh, state, wav_out=yh, T=T)

        def f_pinned():
            eng.step_pinned(xh, state, wav_out=yh, T=T)

        def f_pool():
            xp.copy_(xh, non_blocking=True)
            eng.step_slots(xp, pool.state, B, slots_d, wav_out=yp, T=T)
            yh.copy_(yp, non_blocking=True)

        forms = [f_dev, f_host, f_pinned, f_pool]
        kn = []
        for f in forms:
            f()
            kn.append(eng.last_step_kernel())
        torch.cuda.synchronize()
        res = _time(forms, args)
        lines.append(f"{name:>6} {B:>5} {T:>2} " + " ".join(_cell(r, B * T) for r in res) + f"   {kn[0]} | {kn[2]}")
        print(lines[-1], flush=True)
    lines.append("")
    lines.append(f"# fe_b, n of {args.capacity} slots, T = 1: same cells")
    lines.append(f"{'n':>5} {'slots_pinned':>24} {'copies + step_slots':>24} {'dev: step_slots':>24}   kernel of slots_pinned")
    print("\n".join(lines[-3:]), flush=True)
    eng = _engine("fe_b", dev)
    H, cap = eng.cfg.hop_size, args.capacity
    pool = StreamPool(eng, cap)
    for _ in range(cap):
        pool.open()
    rng = np.random.default_rng(1)
    for n in [int(v) for v in args.n.split(",")]:
        slots_d = torch.tensor([int(s) for s in rng.permutation(cap)[:n]], dtype=torch.int32, device=dev)
        xh = (0.1 * torch.randn(n, H, generator=gen)).pin_memory()
        yh = torch.empty(n, H).pin_memory()
        xd, yd = xh.to(dev), torch.empty(n, H, device=dev)

        def f_pinned():
            eng.step_slots_pinned(xh, pool.state, cap, slots_d, wav_out=yh)

        def f_pool():
            xd.copy_(xh, non_blocking=True)
            eng.step_slots(xd, pool.state, cap, slots_d, wav_out=yd)
            yh.copy_(yd, non_blocking=True)

        def f_dev():
            eng.step_slots(xd, pool.state, cap, slots_d, wav_out=yd)

        f_pinned()
        kname = eng.last_step_kernel()
        torch.cuda.synchronize()
        res = _time([f_pinned, f_pool, f_dev], args)
        lines.append(f"{n:>5} " + " ".join(_cell(r, n) for r in res) + f"   {kname}")
        print(lines[-1], flush=True)
    lines.append("# (x%): spread (max - min) / median of the rounds")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
