#!/usr/bin/env python3
"""The packet-audio step against the pinned slot step it extends, FastEnhancer_B, 256 streams, one hop per call, in one run on one GPU:
  (a) fe_step_slots_pinned on float rows (the path before fe_step_streams);
  (b) fe_step_streams_pinned, float32, every stream one hop;
  (c) fe_step_streams_pinned, int16 PCM, every stream one hop;
  (d) fe_step_streams_pinned, int16 PCM, a third of the streams with no hop.
Three blocks of each form, alternating (a b c d a b c d ...): device events around `--iters` calls after `--warmup` calls.  Each row: the
three block times in us per call, their median and their spread (max - min).  (b) is to be read against (a) with (a)'s own block-to-block
spread as the margin; (c) against (a) shows what half the PCIe bytes buy at this batch.
   python tools/gpu_stream_packets_timing.py [--out profiles/stream_packets_timing_fe_b.txt]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    cfg, sd, fused, orc = build_oracle("fe_b")
    eng = Engine(product_config("fe_b"), dev)
    eng.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    n, H = args.streams, eng.cfg.hop_size
    gen = torch.Generator().manual_seed(0)
    xf = (0.1 * torch.randn(n, H, generator=gen)).pin_memory()
    yf = torch.empty(n, H).pin_memory()
    xs = (xf * 32768).round().to(torch.int16).pin_memory()
    ys = torch.empty(n, H, dtype=torch.int16).pin_memory()
    state = eng.new_state(n)
    slots_d = torch.arange(n, dtype=torch.int32, device=dev)
    d_all = Engine.pack_stream_desc([(i, 1, i * H, i * H) for i in range(n)]).to(dev)
    d_third = Engine.pack_stream_desc([(i, 0 if i % 3 == 2 else 1, i * H, i * H) for i in range(n)]).to(dev)
    forms = [
        ("(a) fe_step_slots_pinned, float rows", lambda: eng.step_slots_pinned(xf, state, n, slots_d, wav_out=yf)),
        ("(b) fe_step_streams_pinned f32, all 1 hop", lambda: eng.step_streams_pinned(xf.view(-1), state, n, d_all, yf.view(-1))),
        ("(c) fe_step_streams_pinned s16, all 1 hop", lambda: eng.step_streams_pinned(xs.view(-1), state, n, d_all, ys.view(-1))),
        ("(d) fe_step_streams_pinned s16, 1/3 at 0 hops", lambda: eng.step_streams_pinned(xs.view(-1), state, n, d_third, ys.view(-1))),
    ]
    kernels = []
    for _, f in forms:
        f()
        kernels.append(eng.last_step_kernel())
    torch.cuda.synchronize()
    times = [[] for _ in forms]
    for _ in range(args.blocks):
        for i, (_, f) in enumerate(forms):
            for _ in range(args.warmup):
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            e1.synchronize()
            times[i].append(1000.0 * e0.elapsed_time(e1) / args.iters)
    lines = [f"# packet-audio step, fe_b, {n} streams, 1 hop per call: {args.blocks} alternating blocks of {args.iters} calls (device events, "
             f"{args.warmup} warm-up calls per block); us per call",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'form':<48} {'blocks (us)':<30} {'median':>8} {'spread':>7}   kernel"]
    for (label, _), t, k in zip(forms, times, kernels):
        lines.append(f"{label:<48} {' '.join(f'{v:8.2f}' for v in t):<30} {float(np.median(t)):>8.2f} {max(t) - min(t):>7.2f}   {k}")
    med = [float(np.median(t)) for t in times]
    spread_a = max(times[0]) - min(times[0])
    lines.append(f"# (b) - (a) = {med[1] - med[0]:+.2f} us against a block-to-block spread of (a) of {spread_a:.2f} us; "
                 f"(c) - (a) = {med[2] - med[0]:+.2f} us; (d) - (c) = {med[3] - med[2]:+.2f} us")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
