#!/usr/bin/env python3
"""What the packet step's time-pipelined form buys a LiSenNet pool (opt-in: Engine.set_time_pipeline(P >= 2)): int16 rings in page-locked host
memory, a level table on the device, in one run on one GPU, after tools/gpu_pool_streams_chunk_timing.py:
  (i)  one stream with a backlog of 64 and of 251 hops: fe_step_pool_streams_ctl_pinned(T_max = hops) - one workgroup walks the hops -
       against fe_step_pool_streams_chunk_pinned(T_max = hops) at P = 8 and P = 16;
  (ii) a tick of 255 one-hop streams plus one stream with 64 hops: the single launch with T_max = 64 against the ordinary launch
       (T_max = 1, 255 streams) followed by the chunk launch (one stream, T_max = 64) on the same stream, at P = 8 and P = 16.
The serial call is the same code before and after this tool's subject was added, so it is the baseline.  Each form is captured into a graph
of `--steps` calls (the pipeline's width is that of the capture), so that the device and not the Python caller is timed; a round is
`--replays` replays between two device events after `--warmup` replays; the forms of a case alternate in `--rounds` rounds.  Reported: the
median over the rounds in ms per call, the spread (max - min) / median of the rounds, and the ratios.  Writes to stdout and to `--out`.
   python tools/gpu_lisennet_pool_streams_chunk_timing.py [--out profiles/lisennet_pool_streams_chunk_timing.txt] [--widths 8,16]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from common import hip_model  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from gpu_pool_streams_chunk_timing import _graph, _time  # noqa: E402

NAME = "lisennet"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--widths", default="8,16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    widths = [int(w) for w in args.widths.split(",")]
    lines = [f"# packet step on the time pipeline for LiSenNet pools (opt-in, fe_set_time_pipeline(P)): int16 rings in page-locked host memory, level table on "
             f"the device, no limit; graphs of {args.steps} calls, per round {args.warmup} warm-up and {args.replays} timed replays (device events), "
             f"{args.rounds} alternating rounds",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'model':>10} {'case':>30} {'ms per call':>12} {'spread':>7}   rounds (ms)   kernel"]
    keep = []

    def pcm(n):
        return ((0.1 * torch.randn(n, generator=gen)) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()

    def flush():
        text = "\n".join(lines) + "\n"
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write(text)
        return text

    def report(label, t, kernel):
        med = float(np.median(t))
        lines.append(f"{NAME:>10} {label:>30} {med:>12.4f} {100.0 * (max(t) - min(t)) / med:>6.1f}%   {' '.join('%.4f' % v for v in t)}   {kernel}")
        return med, (max(t) - min(t))

    eng = hip_model(NAME, device=dev).engine
    H = eng.cfg.hop_size
    try:
        # (i) one stream, a backlog of T hops
        for T in (64, 251):
            cap = 1
            x, y = pcm(T * H), torch.zeros(T * H, dtype=torch.int16).pin_memory()
            lv = torch.zeros(cap, 4, device=dev)
            d = Engine.pack_stream_desc([(0, T, 0, 0)]).to(dev)
            work = torch.empty(eng.lisennet_pool_streams_chunk_work_floats(1, T), dtype=torch.float32, device=dev)
            st = [eng.new_state(cap) for _ in range(1 + len(widths))]
            serial = lambda: eng.step_pool_streams_ctl_pinned(x, st[0], cap, d, y, T_max=T, levels=lv)                     # noqa: E731
            serial()
            names = [eng.last_step_kernel()]
            torch.cuda.synchronize()
            assert "time-pipelined" not in names[0], names
            forms = [(f"(i) 1 x {T} serial", _graph(dev, serial, args.steps))]
            for i, P in enumerate(widths):
                eng.set_time_pipeline(P)
                chunk = lambda i=i: eng.step_pool_streams_chunk_pinned(x, st[1 + i], cap, d, y, T_max=T, levels=lv, work=work)      # noqa: E731
                chunk()
                names.append(eng.last_step_kernel())
                torch.cuda.synchronize()
                assert "time-pipelined" in names[-1], names
                forms.append((f"(i) 1 x {T} chunk P={P}", _graph(dev, chunk, args.steps)))
            keep.append((x, y, lv, d, work, st, forms))
            t = _time(forms, args)
            a, a_range = report(forms[0][0], t[forms[0][0]], names[0])
            for (label, _), k in zip(forms[1:], names[1:]):
                b, _ = report(label, t[label], k)
                lines.append(f"# {NAME} {label}: serial / chunk = {a / b:.2f}; serial - chunk = {a - b:.4f} ms, the serial call's own range {a_range:.4f} ms")
            print(flush().splitlines()[-1], flush=True)

        # (ii) 255 one-hop streams and one stream with 64 hops
        cap, T = 256, 64
        ring = T * H
        eng.set_time_pipeline(-1)
        eng.init_state(eng.new_state(cap), cap)            # (the scratch of the three-launch step holds the ordinary tick's streams)
        x, y = pcm(cap * ring), torch.zeros(cap * ring, dtype=torch.int16).pin_memory()
        lv = torch.zeros(cap, 4, device=dev)
        rows = [(s, T if s == 0 else 1, s * ring, s * ring) for s in range(cap)]
        d_all = Engine.pack_stream_desc(rows).to(dev)
        d_one = Engine.pack_stream_desc(rows[1:]).to(dev)
        d_late = Engine.pack_stream_desc(rows[:1]).to(dev)
        work = torch.empty(eng.lisennet_pool_streams_chunk_work_floats(1, T), dtype=torch.float32, device=dev)
        st = [eng.new_state(cap) for _ in range(1 + len(widths))]
        single = lambda: eng.step_pool_streams_ctl_pinned(x, st[0], cap, d_all, y, T_max=T, levels=lv)                     # noqa: E731
        single()
        names = [eng.last_step_kernel()]
        torch.cuda.synchronize()
        forms = [("(ii) one launch T_max=64", _graph(dev, single, args.steps))]
        for i, P in enumerate(widths):
            eng.set_time_pipeline(P)

            def split(i=i):
                eng.step_pool_streams_ctl_pinned(x, st[1 + i], cap, d_one, y, T_max=1, levels=lv)
                eng.step_pool_streams_chunk_pinned(x, st[1 + i], cap, d_late, y, T_max=T, levels=lv, work=work)

            eng.step_pool_streams_ctl_pinned(x, st[1 + i], cap, d_one, y, T_max=1, levels=lv)
            k = eng.last_step_kernel()
            eng.step_pool_streams_chunk_pinned(x, st[1 + i], cap, d_late, y, T_max=T, levels=lv, work=work)
            assert "time-pipelined" in eng.last_step_kernel(), eng.last_step_kernel()
            names.append(k + " then " + eng.last_step_kernel())
            torch.cuda.synchronize()
            forms.append((f"(ii) T_max=1 + chunk P={P}", _graph(dev, split, args.steps)))
        keep.append((x, y, lv, d_all, d_one, d_late, work, st, forms))
        t = _time(forms, args)
        a, a_range = report(forms[0][0], t[forms[0][0]], names[0])
        for (label, _), k in zip(forms[1:], names[1:]):
            b, _ = report(label, t[label], k)
            lines.append(f"# {NAME} {label}: one launch / (ordinary launch + chunk launch) = {a / b:.2f}; difference {a - b:.4f} ms, "
                         f"the single launch's own range {a_range:.4f} ms")
        print(flush().splitlines()[-1], flush=True)
    finally:
        eng.set_time_pipeline(-1)
    lines.append("# spread: (max - min) / median of the rounds; range: max - min of the rounds")
    print(flush(), end="", flush=True)


if __name__ == "__main__":
    main()
