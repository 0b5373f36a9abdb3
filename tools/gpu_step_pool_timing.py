#!/usr/bin/env python3
"""What slot indexing costs the per-stream kernels of BSRNN, FSPEN and LiSenNet: one hop of `--streams` streams, three ways:
  (a) fe_step(B = streams) on a dense state;
  (b) fe_step_pool with identity slots on a state of the same capacity (the same state addresses as (a), taken through the slot list);
  (c) fe_step_pool with a scattered permutation on a state of twice the capacity.
(b) and (c) give the bits of (a) on the same records (checked before anything is timed).  Device events around `--iters` hops after `--warmup`
hops of each form; the forms alternate in rounds (`--rounds`); each cell is the median over the rounds, the spread (max - min) / median.
   python tools/gpu_step_pool_timing.py [--out profiles/step_pool_timing.txt] [--models bsrnn_xt,fspen,lisennet] [--streams 256]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import hip_model  # noqa: E402


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
    lines = [f"# one hop of {n} streams; median over {args.rounds} alternating rounds of {args.iters} hops (device events, {args.warmup} warm-up hops "
             "per form and round); spread = (max - min) / median over the rounds",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'model':>10} {'(a) fe_step us':>15} {'spread %':>9} {'(b) pool, identity us':>22} {'spread %':>9} {'(b)/(a)':>8} "
             f"{'(c) pool, scattered us':>23} {'spread %':>9} {'(c)/(a)':>8}   kernels of (c)"]
    for name in args.models.split(","):
        eng = hip_model(name, device=dev).engine
        H = eng.cfg.hop_size
        gen = torch.Generator(device="cpu").manual_seed(0)
        x = (0.1 * torch.randn(n, H, generator=gen)).to(dev)
        y = torch.zeros(n, H, device=dev)
        rng = np.random.default_rng(1)
        scattered = [int(s) for s in rng.permutation(2 * n)[:n]]
        ident_d = torch.arange(n, dtype=torch.int32, device=dev)
        scat_d = torch.tensor(scattered, dtype=torch.int32, device=dev)
        # states seeded by four hops; (b) and (c) hold (a)'s records in their slots (fe_state_init on the largest sizes the step scratch)
        st_c = eng.init_state(eng.new_state(2 * n), 2 * n)
        st_a = eng.new_state(n)
        for t in range(4):
            eng.step((0.1 * torch.randn(n, H, generator=gen)).to(dev), st_a, T=1)
        st_b = st_a.clone()
        eng.import_slots(st_c, 2 * n, scattered, eng.export_slots(st_a, n, list(range(n))))

        def form_a():
            eng.step(x, st_a, wav_out=y, T=1)

        def form_b():
            eng.step_pool(x, st_b, n, ident_d, wav_out=y)

        def form_c():
            eng.step_pool(x, st_c, 2 * n, scat_d, wav_out=y)

        forms = [form_a, form_b, form_c]
        outs = []
        for f in forms:
            f()
            torch.cuda.synchronize()
            outs.append(y.clone())
        kern_c = eng.last_step_kernel()
        assert all(torch.equal(o.view(torch.int32), outs[0].view(torch.int32)) for o in outs), f"{name}: the three forms' outputs differ"
        assert torch.equal(eng.export_slots(st_c, 2 * n, scattered).view(torch.int32), eng.export_slots(st_a, n, list(range(n))).view(torch.int32))
        assert torch.equal(st_a.view(torch.int32), st_b.view(torch.int32)), f"{name}: identity slots leave another state"
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
        lines.append(f"{name:>10} {med[0]:>15.2f} {spread[0]:>9.2f} {med[1]:>22.2f} {spread[1]:>9.2f} {med[1] / med[0]:>8.3f} "
                     f"{med[2]:>23.2f} {spread[2]:>9.2f} {med[2] / med[0]:>8.3f}   {kern_c}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
