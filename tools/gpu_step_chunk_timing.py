#!/usr/bin/env python3
"""Few streams x many hops, wav -> wav with carried state: fe_step(B, T) (one workgroup walks a stream's T frames) against the chunk on the
time pipeline + one overlap-add launch - fe_step_chunk for the FastEnhancer shapes, next to fe_spec_step walked and pipelined in the same
run; fe_step_backlog for bsrnn_xxt / bsrnn_xt / bsrnn_t / bsrnn_s / fspen.
HIP events around each call, warm-up first (clocks ramped), median of the repeats.
usage: tools/gpu_step_chunk_timing.py [hops per call] [repeats] [shape ...] [--streams 1,8] [--only walk|chunk] [--json]
(writes a table to stdout; --json: one JSON line per row instead, for a driver that alternates builds.  --only walk with
FASTENHANCER_HIP_LIB=<side build of an older commit> times that build's fe_step: symbols it does not have are not bound.)"""
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import product_config  # noqa: E402
from fastenhancer_amd import _lib  # noqa: E402
from fastenhancer_amd.config import FEConfig  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402

BASELINES = ["bsrnn_xxt", "bsrnn_xt", "bsrnn_t", "bsrnn_s", "fspen"]


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def _option(argv, flag, default=None):
    if flag not in argv:
        return default
    i = argv.index(flag)
    val = argv[i + 1]
    del argv[i:i + 2]
    return val


def main():
    argv = sys.argv[1:]
    streams = [int(s) for s in _option(argv, "--streams", "1,8").split(",")]
    only = _option(argv, "--only")
    as_json = "--json" in argv
    if as_json:
        argv.remove("--json")
    T = int(argv[0]) if len(argv) > 0 else 251
    repeats = int(argv[1]) if len(argv) > 1 else 21
    names = argv[2:] or ["fe_b", "fe_t", "fe_l", "fe_dpt_b"] + BASELINES
    side = os.environ.get("FASTENHANCER_HIP_LIB")
    if side:          # a side build, possibly of an older commit: bind what it has
        have = ctypes.CDLL(side)
        for sym in [s for s in _lib.SYMBOLS if not hasattr(have, s)]:
            del _lib.SYMBOLS[sym]
    dev = torch.device("cuda:0")
    if not as_json:
        print(f"# {torch.cuda.get_device_name(0)}; T = {T} hops per call; median (min .. max) of {repeats} calls after 5 warm-up calls, HIP events, ms")
        print(f"# {'shape':9s} {'B':>2s} {'fe_step walk':>24s} {'chunk / backlog':>24s} {'speed-up':>8s} | {'spec walk':>10s} {'spec pipe':>10s} {'speed-up':>8s} | chunk kernel")
    for name in names:
        cfg = product_config(name)
        eng = Engine(cfg, dev)
        eng.load_state_dict(eng.family.default_state_dict(cfg, torch.Generator().manual_seed(1)))
        fe = isinstance(cfg, FEConfig)
        if fe:
            eng.set_offline_engine("frame_walk")      # (fe_spec_step: the frame walk and its time pipeline, not the time-batched engine)
        H = cfg.hop_size
        for B in streams:
            x = 0.1 * torch.randn(B, T * H, device=dev)
            y = torch.empty_like(x)
            state = eng.new_state(B)
            walk = chunk = swalk = spipe = None
            kern = ""
            if only != "chunk":
                walk = median_ms(lambda: eng.step(x, state, y, T=T), 5, repeats)
            if only != "walk":
                # (FastEnhancer: step_chunk, which step_backlog is; the baselines: step_backlog)
                step, floats = (eng.step_chunk, eng.chunk_work_floats) if fe else (eng.step_backlog, eng.backlog_work_floats)
                work = torch.empty(floats(B, T), device=dev)
                chunk = median_ms(lambda: step(x, state, y, T=T, work=work), 5, repeats)
                kern = eng.last_step_kernel()
            if fe and only is None:
                spec = 0.1 * torch.randn(B, cfg.F0 + 1, T, 2, device=dev)
                h = torch.zeros(eng.model_state_floats(B), device=dev)
                eng.set_time_pipeline(0)
                swalk = median_ms(lambda: eng.spec_step(spec, h), 5, repeats)
                eng.set_time_pipeline(-1)
                spipe = median_ms(lambda: eng.spec_step(spec, h), 5, repeats)
            if as_json:
                print(json.dumps({"shape": name, "B": B, "T": T, "walk_ms": walk and list(walk), "chunk_ms": chunk and list(chunk), "kernel": kern}), flush=True)
                continue
            fmt = lambda r: f"{r[0]:8.3f} ({r[1]:.3f} .. {r[2]:.3f})" if r else "-"      # noqa: E731
            ratio = lambda a, b: f"{a[0] / b[0]:7.2f}x" if a and b else f"{'-':>8s}"     # noqa: E731
            one = lambda r: f"{r[0]:10.3f}" if r else f"{'-':>10s}"                       # noqa: E731
            print(f"  {name:9s} {B:2d} {fmt(walk):>24s} {fmt(chunk):>24s} {ratio(walk, chunk)} | {one(swalk)} {one(spipe)} {ratio(swalk, spipe)} | {kern}")


if __name__ == "__main__":
    main()
