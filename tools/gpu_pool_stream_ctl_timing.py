#!/usr/bin/env python3
"""What the suppression limit and the level meters cost the packet step of BSRNN, FSPEN and LiSenNet: one tick of `--streams` streams, one hop
each, int16 PCM in page-locked host rings at scattered ring offsets and scattered slots (form (c) of tools/gpu_pool_streams_timing.py), four ways:
  (a) fe_step_pool_streams_pinned of the PARENT commit: a side build of the library, `--parent-lib` (loaded through FASTENHANCER_HIP_LIB);
  (b) fe_step_pool_streams_ctl_pinned of this build, both tables NULL;
  (c) levels on, every gain zero;
  (d) levels on and every stream limited (min_gain 0.2).
Two worker processes - one per library - hold their engines for the whole run and take turns, round by round, so the forms alternate as in
tools/gpu_pool_streams_timing.py: device events around `--iters` ticks after `--warmup` ticks of each form; each cell is the median over the
rounds, the spread (max - min) / median.  (b)/(a) is to be read against the spread (a) shows against itself.  Before anything is timed, (b) of
this build is checked to give the bits of its own fe_step_pool_streams_pinned.
   python tools/gpu_pool_stream_ctl_timing.py --parent-lib <libfastenhancer_hip.so of the parent commit> [--out profiles/pool_stream_ctl_timing.txt]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fe_step_pool_streams_ctl", "fe_step_pool_streams_ctl_pinned")


def worker(args):
    """one library, its engines built once; a line on stdin = one round of this worker's forms of one model, answered by a line of JSON"""
    import torch
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from fastenhancer_amd import _lib
    if args.worker == "parent":                  # (the parent's library does not export what this commit adds; nothing here calls it)
        for s in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(s, None)
    from common import hip_model
    from fastenhancer_amd.engine import Engine
    dev = torch.device("cuda:0")
    n = args.streams
    setups = {}

    def setup(name):
        eng = hip_model(name, device=dev).engine
        H = eng.cfg.hop_size
        R = 8 * H
        gen = torch.Generator(device="cpu").manual_seed(0)
        rng = np.random.default_rng(1)
        scattered = [int(s) for s in rng.permutation(2 * n)[:n]]
        pos = rng.integers(0, 8, size=n)
        desc = Engine.pack_stream_desc([(scattered[i], 1, scattered[i] * R + int(pos[i]) * H, scattered[i] * R + int(pos[i]) * H) for i in range(n)]).to(dev)
        ring_in = (0.1 * torch.randn(2 * n, R, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
        ring_out = torch.zeros(2 * n, R, dtype=torch.int16).pin_memory()
        st = eng.init_state(eng.new_state(2 * n), 2 * n)
        seed = eng.new_state(n)
        for t in range(4):
            eng.step((0.1 * torch.randn(n, H, generator=gen)).to(dev), seed, T=1)
        eng.import_slots(st, 2 * n, scattered, eng.export_slots(seed, n, list(range(n))))
        levels = torch.zeros(2 * n, 4, device=dev)
        zeros, limited = torch.zeros(2 * n, device=dev), torch.full((2 * n,), 0.2, device=dev)
        if args.worker == "parent":
            forms = {"a": lambda: eng.step_pool_streams_pinned(ring_in, st, 2 * n, desc, ring_out, T_max=1)}
        else:
            forms = {"b": lambda: eng.step_pool_streams_ctl_pinned(ring_in, st, 2 * n, desc, ring_out, T_max=1),
                     "c": lambda: eng.step_pool_streams_ctl_pinned(ring_in, st, 2 * n, desc, ring_out, T_max=1, min_gain=zeros, levels=levels),
                     "d": lambda: eng.step_pool_streams_ctl_pinned(ring_in, st, 2 * n, desc, ring_out, T_max=1, min_gain=limited, levels=levels)}
            # (b) is this build's plain packet step, bit for bit
            s0, s1, o1 = st.clone(), st.clone(), torch.zeros_like(ring_out).pin_memory()
            eng.step_pool_streams_pinned(ring_in, s0, 2 * n, desc, ring_out, T_max=1)
            eng.step_pool_streams_ctl_pinned(ring_in, s1, 2 * n, desc, o1, T_max=1)
            torch.cuda.synchronize()
            assert torch.equal(ring_out, o1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)), f"{name}: (b) is not fe_step_pool_streams_pinned"
        for f in forms.values():
            f()
        torch.cuda.synchronize()
        return forms, eng

    for line in sys.stdin:
        name = line.strip()
        if not name:
            break
        if name not in setups:
            setups[name] = setup(name)
        forms, eng = setups[name]
        out = {}
        for key, f in forms.items():
            for _ in range(args.warmup):
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f()
            e1.record()
            e1.synchronize()
            out[key] = 1000.0 * e0.elapsed_time(e1) / args.iters
        out["kernels"] = eng.last_step_kernel()
        print("RESULT " + json.dumps(out), flush=True)


def ask(proc, name):
    proc.stdin.write(name + "\n")
    proc.stdin.flush()
    while True:
        line = proc.stdout.readline()
        if not line:
            raise RuntimeError(f"a worker ended early (exit status {proc.poll()})")
        if line.startswith("RESULT "):
            return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="bsrnn_xt,fspen,lisennet")
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="", choices=["", "parent", "this"])
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: the parent commit's libfastenhancer_hip.so (a side build)"
    common = [sys.executable, os.path.abspath(__file__), "--streams", str(args.streams), "--iters", str(args.iters), "--warmup", str(args.warmup)]
    env_parent = dict(os.environ, FASTENHANCER_HIP_LIB=os.path.abspath(args.parent_lib))
    env_this = {k: v for k, v in os.environ.items() if k != "FASTENHANCER_HIP_LIB"}
    procs = [subprocess.Popen(common + ["--worker", w], env=e, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
             for w, e in (("parent", env_parent), ("this", env_this))]
    n = args.streams
    lines = [f"# one tick of {n} streams, one hop each, int16 PCM in pinned host rings, scattered slots and ring offsets; median over {args.rounds} alternating "
             f"rounds of {args.iters} ticks (device events, {args.warmup} warm-up ticks per form and round); spread = (max - min) / median over the rounds",
             "# (a) the parent commit's fe_step_pool_streams_pinned (side build, its own process); (b) fe_step_pool_streams_ctl_pinned, tables NULL; "
             "(c) levels on, gains zero; (d) levels on, every stream limited (min_gain 0.2)",
             f"{'model':>10} {'(a) us':>8} {'spread %':>9} {'(b) us':>8} {'spread %':>9} {'(b)/(a)':>8} {'(c) us':>8} {'spread %':>9} {'(c)/(a)':>8} "
             f"{'(d) us':>8} {'spread %':>9} {'(d)/(a)':>8}   kernels"]
    try:
        for name in args.models.split(","):
            times = {k: [] for k in "abcd"}
            kern = ""
            for _ in range(args.rounds):
                for proc in procs:
                    res = ask(proc, name)
                    kern = res.pop("kernels")
                    for k, v in res.items():
                        times[k].append(v)
            med = {k: float(np.median(v)) for k, v in times.items()}
            spread = {k: 100.0 * (max(v) - min(v)) / float(np.median(v)) for k, v in times.items()}
            cells = f"{med['a']:>8.2f} {spread['a']:>9.2f}" + "".join(f" {med[k]:>8.2f} {spread[k]:>9.2f} {med[k] / med['a']:>8.3f}" for k in "bcd")
            lines.append(f"{name:>10} {cells}   {kern}")
            print(lines[-1], flush=True)
    finally:
        for proc in procs:
            proc.stdin.close()
        for proc in procs:
            proc.wait(timeout=60)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
