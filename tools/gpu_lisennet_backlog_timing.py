#!/usr/bin/env python3
"""LiSenNet, few streams x many hops, wav -> wav with carried state: fe_step(B, T) (one workgroup walks a stream's T frames) against
fe_step_backlog under an explicit fe_set_time_pipeline(P) with the family's work buffer (lisennet_frame_kernel<time-pipelined, streaming> +
stream_ola_kernel), at 1 x 64, 1 x 251 and 4 x 64 hops and several widths.
HIP events around each call; the two forms alternate round by round in one process (walk, pipelined at every width, walk, ...), a round's
figure is the median of the calls after warm-up calls, the reported figure the median of the round medians (min .. max of them).
usage: tools/gpu_lisennet_backlog_timing.py [--out FILE] [--rounds 3] [--calls 15] [--widths 8,16,32,64]
(writes the table to FILE, default profiles/lisennet_backlog_timing.txt, and to stdout)"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import product_config  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402

CASES = [(1, 64), (1, 251), (4, 64)]


def median_ms(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def _option(argv, flag, default):
    if flag not in argv:
        return default
    i = argv.index(flag)
    val = argv[i + 1]
    del argv[i:i + 2]
    return val


def main():
    argv = sys.argv[1:]
    out_path = _option(argv, "--out", os.path.join(REPO, "profiles", "lisennet_backlog_timing.txt"))
    rounds = int(_option(argv, "--rounds", "3"))
    calls = int(_option(argv, "--calls", "15"))
    widths = [int(w) for w in _option(argv, "--widths", "8,16,32,64").split(",")]
    dev = torch.device("cuda:0")
    cfg = product_config("lisennet")
    eng = Engine(cfg, dev)
    eng.load_state_dict(eng.family.default_state_dict(cfg, torch.Generator().manual_seed(1)))
    H = cfg.hop_size
    lines = ["fe_step_backlog of LiSenNet on the time pipeline (opt-in: fe_set_time_pipeline(P >= 2) and a work buffer of",
             "fe_lisennet_backlog_work_floats) against the fe_step walk: chunks of many hops of few streams, wav -> wav with carried state",
             "(tools/gpu_lisennet_backlog_timing.py)", "",
             f"# {torch.cuda.get_device_name(0)}; ms per call, HIP events; each figure the median of {rounds} alternating rounds (walk, then the pipelined call at",
             f"# every width, in one process), a round's figure the median of {calls} calls after 5 warm-up calls.  (rounds: min .. max of the round medians)",
             f"# {'B':>2s} {'T':>4s} {'P':>3s} {'walk':>9s} {'(rounds)':>22s} {'pipelined':>10s} {'(rounds)':>20s} {'walk / pipelined':>17s} | kernel"]
    for B, T in CASES:
        x = 0.1 * torch.randn(B, T * H, device=dev)
        y = torch.empty_like(x)
        state = eng.new_state(B)
        work = torch.empty(eng.lisennet_backlog_work_floats(B, T), device=dev)
        walk, pipe, kern = [], {w: [] for w in widths}, {}
        for _ in range(rounds):
            eng.set_time_pipeline(-1)
            walk.append(median_ms(lambda: eng.step(x, state, y, T=T), 5, calls))
            for w in widths:
                eng.set_time_pipeline(w)
                pipe[w].append(median_ms(lambda: eng.step_backlog(x, state, y, T=T, work=work), 5, calls))
                kern[w] = eng.last_step_kernel()
            eng.set_time_pipeline(-1)
        wm = statistics.median(walk)
        for w in widths:
            pm = statistics.median(pipe[w])
            lines.append(f"  {B:2d} {T:4d} {w:3d} {wm:9.3f} {f'({min(walk):.3f} .. {max(walk):.3f})':>22s} {pm:10.3f} "
                         f"{f'({min(pipe[w]):.3f} .. {max(pipe[w]):.3f})':>20s} {wm / pm:16.2f}x | {kern[w]}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
