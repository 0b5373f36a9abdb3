#!/usr/bin/env python3
"""What the packet step's time-pipelined form buys: fe_b, int16 rings in page-locked host memory, a (one-entry) bank table, in one run on
one GPU:
  (i)  one stream with a backlog of 64 and of 251 hops: fe_step_streams_banked_pinned(T_max = hops) - one workgroup walks the hops -
       against fe_step_streams_chunk_pinned(T_max = hops);
  (ii) a tick of 255 one-hop streams plus one stream with 64 hops: today's single launch with T_max = 64 against the ordinary launch
       (T_max = 1, 255 streams) followed by the chunk launch (one stream, T_max = 64) on the same stream.
Each form is captured into a graph of `--steps` calls, so that the device and not the Python caller is timed; a round is `--replays` replays
between two device events after `--warmup` replays; the forms of a case alternate in `--rounds` rounds.  Reported: the median over the rounds
in ms per call, the spread (max - min) / median of the rounds, and the ratios.  Writes to stdout and to `--out`.
   python tools/gpu_streams_chunk_timing.py [--out profiles/streams_chunk_timing.txt]"""
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

NAME = "fe_b"


def _graph(dev, call, steps):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
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
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--replays", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    eng = hip_model(NAME, device=dev).engine
    H = eng.cfg.hop_size
    gen = torch.Generator().manual_seed(0)
    lines = [f"# packet step on the time pipeline: {NAME}, int16 rings in page-locked host memory, bank table of zeros; graphs of {args.steps} calls, "
             f"per round {args.warmup} warm-up and {args.replays} timed replays (device events), {args.rounds} alternating rounds",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'case':>24} {'ms per call':>12} {'spread':>7}   rounds (ms)   kernel"]
    keep = []

    def pcm(n):
        return ((0.1 * torch.randn(n, generator=gen)) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()

    def report(label, t, kernel):
        med = float(np.median(t))
        lines.append(f"{label:>24} {med:>12.4f} {100.0 * (max(t) - min(t)) / med:>6.1f}%   {' '.join('%.4f' % v for v in t)}   {kernel}")
        return med

    # (i) one stream, a backlog of T hops
    for T in (64, 251):
        cap = 1
        x, y = pcm(T * H), torch.zeros(T * H, dtype=torch.int16).pin_memory()
        bank = torch.zeros(cap, dtype=torch.int32, device=dev)
        d = Engine.pack_stream_desc([(0, T, 0, 0)]).to(dev)
        work = torch.empty(eng.streams_chunk_work_floats(1, T), dtype=torch.float32, device=dev)
        st = [eng.new_state(cap), eng.new_state(cap)]
        serial = lambda: eng.step_streams_pinned(x, st[0], cap, d, y, T_max=T, bank=bank)              # noqa: E731
        chunk = lambda: eng.step_streams_chunk_pinned(x, st[1], cap, d, y, T_max=T, bank=bank, work=work)   # noqa: E731
        names = []
        for call in (serial, chunk):
            call()
            names.append(eng.last_step_kernel())
            torch.cuda.synchronize()
        forms = [(f"(i) 1 x {T} serial", _graph(dev, serial, args.steps)), (f"(i) 1 x {T} chunk", _graph(dev, chunk, args.steps))]
        keep.append((x, y, bank, d, work, st, forms))
        t = _time(forms, args)
        a = report(forms[0][0], t[forms[0][0]], names[0])
        b = report(forms[1][0], t[forms[1][0]], names[1])
        lines.append(f"# (i) 1 stream x {T} hops: serial / chunk = {a / b:.2f}")

    # (ii) 255 one-hop streams and one stream with 64 hops
    cap, T = 256, 64
    ring = T * H
    x, y = pcm(cap * ring), torch.zeros(cap * ring, dtype=torch.int16).pin_memory()
    bank = torch.zeros(cap, dtype=torch.int32, device=dev)
    rows = [(s, T if s == 0 else 1, s * ring, s * ring) for s in range(cap)]
    d_all = Engine.pack_stream_desc(rows).to(dev)
    d_one = Engine.pack_stream_desc(rows[1:]).to(dev)
    d_late = Engine.pack_stream_desc(rows[:1]).to(dev)
    work = torch.empty(eng.streams_chunk_work_floats(cap, T), dtype=torch.float32, device=dev)
    st = [eng.new_state(cap), eng.new_state(cap)]
    single = lambda: eng.step_streams_pinned(x, st[0], cap, d_all, y, T_max=T, bank=bank)              # noqa: E731

    def split():
        eng.step_streams_pinned(x, st[1], cap, d_one, y, T_max=1, bank=bank)
        eng.step_streams_chunk_pinned(x, st[1], cap, d_late, y, T_max=T, bank=bank, work=work)

    single()
    k_single = eng.last_step_kernel()
    torch.cuda.synchronize()
    eng.step_streams_pinned(x, st[1], cap, d_one, y, T_max=1, bank=bank)
    k_split = eng.last_step_kernel()
    eng.step_streams_chunk_pinned(x, st[1], cap, d_late, y, T_max=T, bank=bank, work=work)
    k_split += " then " + eng.last_step_kernel()
    torch.cuda.synchronize()
    forms = [("(ii) one launch T_max=64", _graph(dev, single, args.steps)), ("(ii) T_max=1 + chunk", _graph(dev, split, args.steps))]
    t = _time(forms, args)
    a = report(forms[0][0], t[forms[0][0]], k_single)
    b = report(forms[1][0], t[forms[1][0]], k_split)
    lines.append(f"# (ii) 255 x 1 hop + 1 x 64 hops: one launch / (ordinary launch + chunk launch) = {a / b:.2f}")
    lines.append("# spread: (max - min) / median of the rounds")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
