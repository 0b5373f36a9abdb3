#!/usr/bin/env python3
"""The packet-audio step against the pinned slot step it extends, FastEnhancer_B, 256 streams, one hop per call, in one run on one GPU:
  (a) fe_step_slots_pinned on float rows (the path before fe_step_streams);
  (b) fe_step_streams_pinned, float32, every stream one hop;
  (c) fe_step_streams_pinned, int16 PCM, every stream one hop;
  (d) fe_step_streams_pinned, int16 PCM, a third of the streams with no hop;
  (e) fe_step_streams_ctl_pinned, float32, both tables null - the same kernel as (b) through the other entry point;
  (f) fe_step_streams_ctl_pinned, float32, level meters on (a pinned level table);
  (g) fe_step_streams_ctl_pinned, float32, level meters on and a suppression limit of -20 dB on every stream.
Three blocks of each form, alternating (a b c d ... a b c d ...): device events around `--iters` calls after `--warmup` calls.  Each row: the
three block times in us per call, their median and their spread (max - min), and the host's time to enqueue one call (wall clock over the
block's calls before the wait: what the device events cannot see, the table lookups of the ctl entry points among it).  (b) is to be read
against (a) with (a)'s own block-to-block spread as the margin; (c) against (a) shows what half the PCIe bytes buy at this batch; (e), (f),
(g) against (b) with (b)'s own spread.  --model / --streams: another FastEnhancer shape or batch; --no-ctl: forms (a) - (d) only (a library
from before the ctl entry points, for an A/B of two builds).
   python tools/gpu_stream_packets_timing.py [--out profiles/stream_packets_timing_fe_b.txt]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import build_oracle, product_config  # noqa: E402
from fastenhancer_amd import _lib  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--model", default="fe_b")
    ap.add_argument("--no-ctl", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    cfg, sd, fused, orc = build_oracle(args.model)
    eng = Engine(product_config(args.model), dev)
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
    if not args.no_ctl:
        lv = eng.new_pinned(n, 4)
        gain = torch.full((n,), 0.1, device=dev)
        ctl = lambda **kw: eng.step_streams_pinned(xf.view(-1), state, n, d_all, yf.view(-1), **kw)
        # (both tables null is not reachable through Engine.step_streams_pinned, which then calls fe_step_streams_pinned: the entry point itself)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        null = ctypes.c_void_p(0)
        forms += [
            ("(e) fe_step_streams_ctl_pinned f32, tables null", lambda: _lib.check(eng.lib.fe_step_streams_ctl_pinned(
                eng._h, vp(xf), xf.numel(), vp(state), n, vp(d_all), vp(yf), yf.numel(), n, 1, _lib.FE_AUDIO_F32, null, null,
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "(e)")),
            ("(f) fe_step_streams_ctl_pinned f32, levels", lambda: ctl(levels=lv)),
            ("(g) fe_step_streams_ctl_pinned f32, levels + limit", lambda: ctl(levels=lv, min_gain=gain)),
        ]
    kernels = []
    for _, f in forms:
        f()
        kernels.append(eng.last_step_kernel())
    torch.cuda.synchronize()
    times = [[] for _ in forms]
    host = [[] for _ in forms]
    for _ in range(args.blocks):
        for i, (_, f) in enumerate(forms):
            for _ in range(args.warmup):
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            w0 = time.perf_counter()
            for _ in range(args.iters):
                f()
            w1 = time.perf_counter()
            e1.record()
            e1.synchronize()
            host[i].append(1e6 * (w1 - w0) / args.iters)
            times[i].append(1000.0 * e0.elapsed_time(e1) / args.iters)
    lines = [f"# packet-audio step, {args.model}, {n} streams, 1 hop per call: {args.blocks} alternating blocks of {args.iters} calls (device events, "
             f"{args.warmup} warm-up calls per block); us per call",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'form':<48} {'blocks (us)':<30} {'median':>8} {'spread':>7} {'host':>7}   kernel"]
    for (label, _), t, hw, k in zip(forms, times, host, kernels):
        lines.append(f"{label:<48} {' '.join(f'{v:8.2f}' for v in t):<30} {float(np.median(t)):>8.2f} {max(t) - min(t):>7.2f} {float(np.median(hw)):>7.2f}   {k}")
    med = [float(np.median(t)) for t in times]
    spread_a = max(times[0]) - min(times[0])
    lines.append(f"# (b) - (a) = {med[1] - med[0]:+.2f} us against a block-to-block spread of (a) of {spread_a:.2f} us; "
                 f"(c) - (a) = {med[2] - med[0]:+.2f} us; (d) - (c) = {med[3] - med[2]:+.2f} us")
    if not args.no_ctl:
        lines.append(f"# (e) - (b) = {med[4] - med[1]:+.2f} us, (f) - (b) = {med[5] - med[1]:+.2f} us, (g) - (b) = {med[6] - med[1]:+.2f} us against a "
                     f"block-to-block spread of (b) of {max(times[1]) - min(times[1]):.2f} us")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
