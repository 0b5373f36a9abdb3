#!/usr/bin/env python3
"""What the packet form costs the slotted per-stream kernels of BSRNN, FSPEN and LiSenNet: one tick of `--streams` streams, four ways:
  (a) fe_step_pool with identity slots on dense float32 rows (the slotted kernels are the parent commit's, instruction for instruction:
      profiles/pool_streams_device_code.txt);
  (b) fe_step_pool_streams on the same dense layout, float32 device audio, one hop each;
  (c) fe_step_pool_streams_pinned, int16 PCM in page-locked host memory at scattered ring offsets (a ring of 8 hops per slot, each stream at
      a hop position of its own), scattered slots on a state of twice the capacity;
  (d) (b) with every fourth stream at 0 hops.
(b) gives the bits of (a) (checked before anything is timed).  Device events around `--iters` ticks after `--warmup` ticks of each form; the
forms alternate in rounds (`--rounds`); each cell is the median over the rounds, the spread (max - min) / median.
   python tools/gpu_pool_streams_timing.py [--out profiles/pool_streams_timing.txt] [--models bsrnn_xt,fspen,lisennet] [--streams 256]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import hip_model  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="bsrnn_xt,fspen,lisennet")
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    n = args.streams
    lines = [f"# one tick of {n} streams, one hop each; median over {args.rounds} alternating rounds of {args.iters} ticks (device events, {args.warmup} warm-up "
             "ticks per form and round); spread = (max - min) / median over the rounds",
             "# (a) fe_step_pool, identity slots; (b) fe_step_pool_streams, dense f32 device audio; (c) fe_step_pool_streams_pinned, int16 at scattered ring "
             "offsets, scattered slots; (d) = (b) with a quarter of the streams at 0 hops",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'model':>10} {'(a) us':>8} {'spread %':>9} {'(b) us':>8} {'spread %':>9} {'(b)/(a)':>8} {'(c) us':>8} {'spread %':>9} {'(c)/(a)':>8} "
             f"{'(d) us':>8} {'spread %':>9} {'(d)/(a)':>8}   kernels of (c)"]
    for name in args.models.split(","):
        eng = hip_model(name, device=dev).engine
        H = eng.cfg.hop_size
        R = 8 * H
        gen = torch.Generator(device="cpu").manual_seed(0)
        x = (0.1 * torch.randn(n, H, generator=gen)).to(dev)
        y = torch.zeros(n, H, device=dev)
        y_b = torch.zeros(n, H, device=dev)
        rng = np.random.default_rng(1)
        scattered = [int(s) for s in rng.permutation(2 * n)[:n]]
        ident_d = torch.arange(n, dtype=torch.int32, device=dev)
        desc_b = Engine.pack_stream_desc([(i, 1, i * H, i * H) for i in range(n)]).to(dev)
        desc_d = Engine.pack_stream_desc([(i, 0 if i % 4 == 1 else 1, i * H, i * H) for i in range(n)]).to(dev)
        pos = rng.integers(0, 8, size=n)
        desc_c = Engine.pack_stream_desc([(scattered[i], 1, scattered[i] * R + int(pos[i]) * H, scattered[i] * R + int(pos[i]) * H) for i in range(n)]).to(dev)
        ring_in = (0.1 * torch.randn(2 * n, R, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
        ring_out = torch.zeros(2 * n, R, dtype=torch.int16).pin_memory()
        # states seeded by four hops (fe_state_init on the largest sizes the step scratch: the steps below allocate nothing)
        st_c = eng.init_state(eng.new_state(2 * n), 2 * n)
        st_a = eng.new_state(n)
        for t in range(4):
            eng.step((0.1 * torch.randn(n, H, generator=gen)).to(dev), st_a, T=1)
        st_b, st_d = st_a.clone(), st_a.clone()
        eng.import_slots(st_c, 2 * n, scattered, eng.export_slots(st_a, n, list(range(n))))

        def form_a():
            eng.step_pool(x, st_a, n, ident_d, wav_out=y)

        def form_b():
            eng.step_pool_streams(x.view(-1), st_b, n, desc_b, y_b.view(-1), T_max=1)

        def form_c():
            eng.step_pool_streams_pinned(ring_in, st_c, 2 * n, desc_c, ring_out, T_max=1)

        def form_d():
            eng.step_pool_streams(x.view(-1), st_d, n, desc_d, y_b.view(-1), T_max=1)

        forms = [form_a, form_b, form_c, form_d]
        form_a()
        form_b()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), y_b.view(torch.int32)), f"{name}: (b) differs from (a)"
        assert torch.equal(st_a.view(torch.int32), st_b.view(torch.int32)), f"{name}: (b) leaves another state than (a)"
        form_c()
        kern_c = eng.last_step_kernel()
        form_d()
        torch.cuda.synchronize()
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
        cells = f"{med[0]:>8.2f} {spread[0]:>9.2f}" + "".join(f" {med[i]:>8.2f} {spread[i]:>9.2f} {med[i] / med[0]:>8.3f}" for i in (1, 2, 3))
        lines.append(f"{name:>10} {cells}   {kern_c}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
