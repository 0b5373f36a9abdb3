#!/usr/bin/env python3
"""Per-hop step of n active streams out of a state of 1024 (FastEnhancer_B), three ways:
  (a) fe_step_slots on the named slots of the 1024-stream state;
  (b) torch gather of the active streams' state into a compact buffer + fe_step(n) + scatter back;
  (c) fe_step over all 1024 streams.
Device events around `--iters` steps after `--warmup` steps of each form; the three forms alternate in rounds (`--rounds`) and each cell
is the median over rounds.  Writes a table (and the kernel each form ran, from fe_last_step_kernel) to stdout and to `--out`.
   python tools/gpu_slot_step_timing.py [--out profiles/slot_step_timing_fe_b.txt] [--n 64,128,256,512]"""
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


def _views(eng, state, B):
    """per-stream views of every state tensor (stream on dim 0): what a caller without fe_step_slots gathers and scatters"""
    return [t.reshape(B, -1) if t.is_contiguous() else t for t in eng.split_state(state, B, head0=True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="fe_b")
    ap.add_argument("--capacity", type=int, default=1024)
    ap.add_argument("--n", default="64,128,256,512")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    cfg, sd, fused, orc = build_oracle(args.name)
    eng = Engine(product_config(args.name), dev)
    eng.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    assert not eng.cfg.dpt, "(b) gathers split_state views: rings with their heads are not covered here"
    cap, H = args.capacity, eng.cfg.hop_size
    state = eng.new_state(cap)
    x_all = 0.1 * torch.randn(cap, H, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    y_all = torch.empty(cap, H, device=dev)
    for _ in range(3):
        eng.step(x_all, state, wav_out=y_all)
    rng = np.random.default_rng(1)
    lines = [f"# {args.name}: per-hop step of n active streams, state capacity {cap}; median over {args.rounds} alternating rounds of "
             f"{args.iters} steps (device events, {args.warmup} warm-up steps per form and round); us per step",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'n':>5} {'(a) step_slots':>15} {'(b) gather+step+scatter':>24} {'(c) step all':>13}   kernels (a) | (b) | (c)"]
    for n in [int(v) for v in args.n.split(",")]:
        slots = [int(s) for s in rng.permutation(cap)[:n]]
        slots_d = torch.tensor(slots, dtype=torch.int32, device=dev)
        idx = slots_d.long()
        x = x_all[:n].contiguous()
        y = torch.empty(n, H, device=dev)
        comp = eng.new_state(n)
        full_v, comp_v = _views(eng, state, cap), _views(eng, comp, n)

        def form_a():
            eng.step_slots(x, state, cap, slots_d, wav_out=y)

        def form_b():
            for vc, vf in zip(comp_v, full_v):
                torch.index_select(vf, 0, idx, out=vc) if vc.is_contiguous() else vc.copy_(vf[idx])
            eng.step(x, comp, wav_out=y)
            for vc, vf in zip(comp_v, full_v):
                vf.index_copy_(0, idx, vc)

        def form_c():
            eng.step(x_all, state, wav_out=y_all)

        forms = [form_a, form_b, form_c]
        names = []
        for f in forms:
            f()
            names.append(eng.last_step_kernel())
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
        med = [float(np.median(t)) for t in times]
        spread = [100.0 * (max(t) - min(t)) / float(np.median(t)) for t in times]
        lines.append(f"{n:>5} {med[0]:>10.2f} ({spread[0]:.0f}%) {med[1]:>18.2f} ({spread[1]:.0f}%) {med[2]:>8.2f} ({spread[2]:.0f}%)   "
                     f"{names[0]} | {names[1]} | {names[2]}")
        print(lines[-1], flush=True)
    lines.append("# (x%): spread (max - min) / median of the rounds")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
