#!/usr/bin/env python3
"""What the packet step's time-pipelined form buys a BSRNN or FSPEN pool: bsrnn_xxt, bsrnn_xt, bsrnn_s and fspen, int16 rings in page-locked
host memory, a level table on the device, in one run on one GPU:
  (i)  one stream with a backlog of 64 and of 251 hops: fe_step_pool_streams_ctl_pinned(T_max = hops) - one workgroup walks the hops -
       against fe_step_pool_streams_chunk_pinned(T_max = hops);
  (ii) a tick of 255 one-hop streams plus one stream with 64 hops: today's single launch with T_max = 64 against the ordinary launch
       (T_max = 1, 255 streams) followed by the chunk launch (one stream, T_max = 64) on the same stream.
The serial call is the same code before and after this tool's subject was added, so it is the baseline.  Each form is captured into a graph
of `--steps` calls, so that the device and not the Python caller is timed; a round is `--replays` replays between two device events after
`--warmup` replays; the forms of a case alternate in `--rounds` rounds.  Reported: the median over the rounds in ms per call, the spread
(max - min) / median of the rounds, and the ratios.  Writes to stdout and to `--out`.
   python tools/gpu_pool_streams_chunk_timing.py [--out profiles/pool_streams_chunk_timing.txt] [--models bsrnn_xxt,fspen]"""
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

MODELS = ["bsrnn_xxt", "bsrnn_xt", "bsrnn_s", "fspen"]


def _graph(dev, call, steps):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            call()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(steps):
            call()
    return g


def _time(forms, args):
    """forms: [(label, graph)] -> {label: [ms per call, one per round]}, the forms alternating"""
    times = {label: [] for label, _ in forms}
    for _ in range(args.rounds):
        for label, g in forms:
            for _ in range(args.warmup):
                g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.replays):
                g.replay()
            e1.record()
            e1.synchronize()
            times[label].append(e0.elapsed_time(e1) / (args.replays * args.steps))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = [f"# packet step on the time pipeline for BSRNN and FSPEN pools: int16 rings in page-locked host memory, level table on the device, no limit; "
             f"graphs of {args.steps} calls, per round {args.warmup} warm-up and {args.replays} timed replays (device events), {args.rounds} alternating rounds",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'model':>10} {'case':>26} {'ms per call':>12} {'spread':>7}   rounds (ms)   kernel"]
    keep = []

    def pcm(n):
        return ((0.1 * torch.randn(n, generator=gen)) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()

    def flush():
        text = "\n".join(lines) + "\n"
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write(text)
        return text

    for name in args.models.split(","):
        eng = hip_model(name, device=dev).engine
        H = eng.cfg.hop_size

        def report(label, t, kernel):
            med = float(np.median(t))
            lines.append(f"{name:>10} {label:>26} {med:>12.4f} {100.0 * (max(t) - min(t)) / med:>6.1f}%   {' '.join('%.4f' % v for v in t)}   {kernel}")
            return med

        # (i) one stream, a backlog of T hops
        for T in (64, 251):
            cap = 1
            x, y = pcm(T * H), torch.zeros(T * H, dtype=torch.int16).pin_memory()
            lv = torch.zeros(cap, 4, device=dev)
            d = Engine.pack_stream_desc([(0, T, 0, 0)]).to(dev)
            work = torch.empty(eng.pool_streams_chunk_work_floats(1, T), dtype=torch.float32, device=dev)
            st = [eng.new_state(cap), eng.new_state(cap)]
            serial = lambda: eng.step_pool_streams_ctl_pinned(x, st[0], cap, d, y, T_max=T, levels=lv)                     # noqa: E731
            chunk = lambda: eng.step_pool_streams_chunk_pinned(x, st[1], cap, d, y, T_max=T, levels=lv, work=work)         # noqa: E731
            names = []
            for call in (serial, chunk):
                call()
                names.append(eng.last_step_kernel())
                torch.cuda.synchronize()
            assert "time-pipelined" in names[1] and "time-pipelined" not in names[0], names
            forms = [(f"(i) 1 x {T} serial", _graph(dev, serial, args.steps)), (f"(i) 1 x {T} chunk", _graph(dev, chunk, args.steps))]
            keep.append((x, y, lv, d, work, st, forms))
            t = _time(forms, args)
            a = report(forms[0][0], t[forms[0][0]], names[0])
            b = report(forms[1][0], t[forms[1][0]], names[1])
            lines.append(f"# {name} (i) 1 stream x {T} hops: serial / chunk = {a / b:.2f}")
            print(flush().splitlines()[-1], flush=True)

        # (ii) 255 one-hop streams and one stream with 64 hops
        cap, T = 256, 64
        ring = T * H
        eng.init_state(eng.new_state(cap), cap)            # (the scratch of BSRNN's three-launch step holds the ordinary tick's streams)
        x, y = pcm(cap * ring), torch.zeros(cap * ring, dtype=torch.int16).pin_memory()
        lv = torch.zeros(cap, 4, device=dev)
        rows = [(s, T if s == 0 else 1, s * ring, s * ring) for s in range(cap)]
        d_all = Engine.pack_stream_desc(rows).to(dev)
        d_one = Engine.pack_stream_desc(rows[1:]).to(dev)
        d_late = Engine.pack_stream_desc(rows[:1]).to(dev)
        work = torch.empty(eng.pool_streams_chunk_work_floats(cap, T), dtype=torch.float32, device=dev)
        st = [eng.new_state(cap), eng.new_state(cap)]
        single = lambda: eng.step_pool_streams_ctl_pinned(x, st[0], cap, d_all, y, T_max=T, levels=lv)                     # noqa: E731

        def split():
            eng.step_pool_streams_ctl_pinned(x, st[1], cap, d_one, y, T_max=1, levels=lv)
            eng.step_pool_streams_chunk_pinned(x, st[1], cap, d_late, y, T_max=T, levels=lv, work=work)

        single()
        k_single = eng.last_step_kernel()
        torch.cuda.synchronize()
        eng.step_pool_streams_ctl_pinned(x, st[1], cap, d_one, y, T_max=1, levels=lv)
        k_split = eng.last_step_kernel()
        eng.step_pool_streams_chunk_pinned(x, st[1], cap, d_late, y, T_max=T, levels=lv, work=work)
        assert "time-pipelined" in eng.last_step_kernel(), eng.last_step_kernel()
        k_split += " then " + eng.last_step_kernel()
        torch.cuda.synchronize()
        forms = [("(ii) one launch T_max=64", _graph(dev, single, args.steps)), ("(ii) T_max=1 + chunk", _graph(dev, split, args.steps))]
        keep.append((x, y, lv, d_all, d_one, d_late, work, st, forms))
        t = _time(forms, args)
        a = report(forms[0][0], t[forms[0][0]], k_single)
        b = report(forms[1][0], t[forms[1][0]], k_split)
        lines.append(f"# {name} (ii) 255 x 1 hop + 1 x 64 hops: one launch / (ordinary launch + chunk launch) = {a / b:.2f}")
        print(flush().splitlines()[-1], flush=True)
    lines.append("# spread: (max - min) / median of the rounds")
    print(flush(), end="", flush=True)


if __name__ == "__main__":
    main()
