#!/usr/bin/env python3
"""What the polyphase resampler costs, next to the model tick it would sit beside:
  (a) fe_step_streams_pinned of FastEnhancer_B: `--streams` streams, one hop each, int16 PCM in page-locked rings - the packet tick;
  (b) fe_resample_streams_pinned 48 -> 16 kHz: the same number of streams, one 20 ms packet each (960 int16 samples in, 320 out), page-locked;
  (c) fe_resample_streams_pinned 16 -> 48 kHz: 20 ms packets the other way (320 in, 960 out);
  (d) fe_resample, 64 whole signals of 4 s, 48 -> 16 kHz, float32 device memory;  (e) the same, 16 -> 48 kHz.
Device events around `--iters` calls after `--warmup` calls of each form; the forms alternate in rounds (`--rounds`); each cell is the median
over the rounds, the spread (max - min) / median.  Before anything is timed the tool records the largest error of the whole-signal call
against the float64 oracle (tests/resample_oracle.py) as a fraction of the contract's bound, for the five pairs of the tests.
   python tools/gpu_resample_timing.py [--out profiles/resample_timing.txt] [--streams 256]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import resample_oracle as ro  # noqa: E402
from common import hip_model  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from fastenhancer_amd.resample import Resampler  # noqa: E402

PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (16000, 48000), (16000, 44100)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    n = args.streams
    gen = torch.Generator(device="cpu").manual_seed(0)
    lines = [f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             "# observed error of fe_resample against the float64 oracle, 3 rows of 4001 samples uniform in [-1, 1): max |err|, the contract's bound "
             "(K + 2) 2^-24 S peak, their ratio",
             f"{'pair':>16} {'K':>4} {'max err':>10} {'bound':>10} {'ratio':>6}"]
    for a, b in PAIRS:
        rs = Resampler(a, b, dev)
        x = 2.0 * torch.rand(3, 4001, generator=gen) - 1.0
        y = rs(x.to(dev)).cpu().double().numpy()
        h = rs.taps().numpy()
        err = float(np.abs(y - ro.resample(x.double().numpy(), rs.up, rs.down, h=h)).max())
        bound = ro.error_bound(rs.up, rs.down, float(x.abs().max()), h=h)
        lines.append(f"{f'{a}->{b}':>16} {rs.taps_per_output:>4} {err:>10.3e} {bound:>10.3e} {err / bound:>6.3f}")
        print(lines[-1], flush=True)

    eng = hip_model("fe_b", device=dev).engine
    H = eng.cfg.hop_size
    R = 8 * H
    ring_in = (0.1 * torch.randn(n, R, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
    ring_out = torch.zeros(n, R, dtype=torch.int16).pin_memory()
    state = eng.new_state(n)
    desc_m = Engine.pack_stream_desc([(i, 1, i * R, i * R) for i in range(n)]).to(dev)
    down, up = Resampler(48000, 16000, dev), Resampler(16000, 48000, dev)
    pk48 = (0.1 * torch.randn(n, 960, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
    pk16 = (0.1 * torch.randn(n, 320, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
    o16 = torch.zeros(n, 321, dtype=torch.int16).pin_memory()
    o48 = torch.zeros(n, 961, dtype=torch.int16).pin_memory()
    made = torch.zeros(n, dtype=torch.int32).pin_memory()
    st_down, st_up = down.new_state(n), up.new_state(n)
    desc_down = Resampler.pack_desc([(i, 960, i * 960, i * 321) for i in range(n)]).to(dev)
    desc_up = Resampler.pack_desc([(i, 320, i * 320, i * 961) for i in range(n)]).to(dev)
    sig48 = (0.1 * torch.randn(64, 4 * 48000, generator=gen)).to(dev)
    sig16 = (0.1 * torch.randn(64, 4 * 16000, generator=gen)).to(dev)

    forms = [("(a) fe_b packet tick, pinned s16", lambda: eng.step_streams_pinned(ring_in, state, n, desc_m, ring_out, T_max=1)),
             ("(b) 48->16 kHz, 20 ms packets, pinned s16", lambda: down.step_streams_pinned(pk48, st_down, n, desc_down, o16, 960, produced=made)),
             ("(c) 16->48 kHz, 20 ms packets, pinned s16", lambda: up.step_streams_pinned(pk16, st_up, n, desc_up, o48, 320, produced=made)),
             ("(d) 48->16 kHz, 64 x 4 s whole, f32 device", lambda: down(sig48)),
             ("(e) 16->48 kHz, 64 x 4 s whole, f32 device", lambda: up(sig16))]
    for _, f in forms:
        f()
    torch.cuda.synchronize()
    kernels = [eng.last_step_kernel(), down.last_kernel()]
    times = [[] for _ in forms]
    for _ in range(args.rounds):
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
    med = [float(np.median(t)) for t in times]
    lines += ["", f"# {n} streams ((a) - (c)); median over {args.rounds} alternating rounds of {args.iters} calls (device events, {args.warmup} warm-up calls per form "
              "and round); spread = (max - min) / median over the rounds; ratio = to the model tick (a).  (d), (e) include the allocation of the output tensor",
              f"{'form':>44} {'us':>9} {'spread %':>9} {'/ (a)':>7}"]
    for i, (what, _) in enumerate(forms):
        spread = 100.0 * (max(times[i]) - min(times[i])) / med[i]
        lines.append(f"{what:>44} {med[i]:>9.2f} {spread:>9.2f} {med[i] / med[0]:>7.3f}")
    lines.append(f"# kernels: (a) {kernels[0]}; the resampler's last: {kernels[1]}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
