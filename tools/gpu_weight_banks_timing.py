#!/usr/bin/env python3
"""What weight banks cost: fe_b, 256 streams, one hop per tick, device audio, level table on (the ctl step), in one run on one GPU:
  ctl       fe_step_streams_ctl, no bank table - the call every tree has (run this tool from a checkout of the parent commit with
            `--forms ctl` to compare the two trees: the NULL path must cost nothing);
  banked-k  fe_step_streams_banked with the streams spread over k of the engine's 8 banks (k = 1: a table of zeros);
  8x32      eight one-bank engines at 32 streams each, their eight launches back to back on one stream: what a caller with eight
            checkpoints does without banks.
Each form is captured into a graph of `--steps` ticks, so that the device and not the Python caller is timed; a round is `--replays` replays
between two device events after `--warmup` replays (the clock ramp); the forms alternate in `--rounds` rounds.  Reported: the median over the
rounds in us per tick, the spread (max - min) / median of the rounds, and the ratios.  Writes to stdout and to `--out`.
   python tools/gpu_weight_banks_timing.py [--forms ctl] [--out profiles/weight_banks_timing.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import MODEL_KWARGS, MODEL_MODULE, product_config  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from oracle.fe_oracle import FEConfig  # noqa: E402
from oracle.weightgen import make_training_state_dict  # noqa: E402

NAME, STREAMS, BANKS = "fe_b", 256, 8


def _checkpoint(k):
    kw, _, seed = MODEL_KWARGS[NAME]
    cfg = FEConfig.from_model_kwargs(kw, variant=MODEL_MODULE[NAME].split(".")[-1])
    return {key: torch.from_numpy(np.asarray(v)) for key, v in make_training_state_dict(cfg, seed + k).items()}


def _graph(dev, tick, steps):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            tick()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            tick()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="ctl,banked-1,banked-2,banked-8,8x32")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--replays", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    want = args.forms.split(",")
    sds = [_checkpoint(k) for k in range(BANKS if any(f != "ctl" for f in want) else 1)]
    eng = Engine(product_config(NAME), dev)
    if len(sds) > 1:
        eng.set_weight_banks(BANKS)
    for k, sd in enumerate(sds):
        eng.load_state_dict(sd, **({"bank": k} if k else {}))
    H = eng.cfg.hop_size
    gen = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(STREAMS, H, generator=gen)).to(dev)
    y = torch.empty(STREAMS, H, device=dev)
    lv = torch.zeros(STREAMS, 4, device=dev)
    desc = Engine.pack_stream_desc([(i, 1, i * H, i * H) for i in range(STREAMS)]).to(dev)
    state = eng.new_state(STREAMS)
    forms, kernels, ticks = [], [], []          # (ticks: the graphs read the closures' tables for as long as they are replayed)

    def one(bank):
        kw = {} if bank is None else {"bank": bank}
        return lambda: eng.step_streams(x.view(-1), state, STREAMS, desc, y.view(-1), T_max=1, levels=lv, **kw)

    for f in want:
        if f == "ctl":
            tick = one(None)
        elif f.startswith("banked-"):
            k = int(f.split("-")[1])
            tick = one(torch.tensor([i % k for i in range(STREAMS)], dtype=torch.int32, device=dev))
        else:
            n = STREAMS // BANKS
            parts = []
            for k in range(BANKS):
                e = Engine(product_config(NAME), dev)
                e.load_state_dict(sds[k])
                parts.append((e, e.new_state(n), Engine.pack_stream_desc([(i, 1, (k * n + i) * H, (k * n + i) * H) for i in range(n)]).to(dev),
                              torch.zeros(n, 4, device=dev)))

            def tick(parts=parts):
                for e, st, d, l in parts:
                    e.step_streams(x.view(-1), st, n, d, y.view(-1), T_max=1, levels=l)
        ticks.append(tick)
        tick()
        kernels.append((parts[0][0] if f == "8x32" else eng).last_step_kernel())
        torch.cuda.synchronize()
        forms.append(_graph(dev, tick, args.steps))
    times = [[] for _ in forms]
    for _ in range(args.rounds):
        for i, g in enumerate(forms):
            for _ in range(args.warmup):
                g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                g.replay()
            e1.record()
            e1.synchronize()
            times[i].append(1000.0 * e0.elapsed_time(e1) / (args.replays * args.steps))
    med = {f: float(np.median(t)) for f, t in zip(want, times)}
    lines = [f"# weight banks: {NAME}, {STREAMS} streams, one hop per tick, device audio, level table on; graphs of {args.steps} ticks, per round "
             f"{args.warmup} warm-up and {args.replays} timed replays (device events), {args.rounds} alternating rounds",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'form':>9} {'us per tick':>12} {'spread':>7}   rounds (us)   kernel"]
    for f, t, k in zip(want, times, kernels):
        lines.append(f"{f:>9} {med[f]:>12.2f} {100.0 * (max(t) - min(t)) / med[f]:>6.1f}%   {' '.join('%.2f' % v for v in t)}   {k}")
    if "ctl" in med:
        for f in want:
            if f.startswith("banked-"):
                lines.append(f"# {f} / ctl = {med[f] / med['ctl']:.3f}")
    if "8x32" in med:
        for f in want:
            if f.startswith("banked-"):
                lines.append(f"# 8x32 / {f} = {med['8x32'] / med[f]:.2f}")
    lines.append("# spread: (max - min) / median of the rounds")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
