#!/usr/bin/env python3
"""What G.711 clients cost next to int16 clients, and what the 16-byte store body of the G.711 output helper buys over page-locked memory.

Table 1 - one process, one FastEnhancer_B engine, three serving.RingResampledPacketPool (client_format s16, ulaw, alaw) with `--streams`
streams at 8 kHz, one hop (128 client samples) per stream and tick.  Host: the wall time of tick(), which ends in its synchronise; the
pushes and pulls are outside the timed region.  Kernels: the pool's two resampler launches on their own - fe_resample_rings_pinned from
the flat page-locked client staging into page-locked int16 rings and back, the shapes and descriptors of the pool's tick, descriptors
already on the device - `--iters` launches between two events: that is the time from one launch to the next, the host's enqueue
included, an upper bound of the kernel's duration (table 2 has the durations).  The three formats ALTERNATE: a block of one, then of the next, and the
whole alternation is run `--repeats` times; a format is compared with the s16 block of the same round, and the spread of the s16 rounds
is what a difference has to exceed.

Table 2 - kernel durations from a rocprofv3 kernel trace, each in a run of its own (a trace slows the host: nothing of table 1 is taken
under it).  `--trace-worker` launches, format by format, the launch to the model's rate and the launch back `--iters` times each;
`--trace-report DIR...` reads the traces' kernel rows in launch order and prints mean and median per block.  One trace is taken under
this library and one under a side build whose G.711 store body is single-byte stores, which shows what the 16-byte body buys:
    FE_BUILD_TAG=bytebody FE_EXTRA_DEFS=-DFE_G711_BYTE_BODY python -m fastenhancer_amd.build        # -> ab/lib_bytebody.so
    python tools/gpu_g711_timing.py --out profiles/g711_timing.txt
    rocprofv3 --kernel-trace --output-format csv -d prof_main -o t -- python tools/gpu_g711_timing.py --trace-worker
    FASTENHANCER_HIP_LIB=ab/lib_bytebody.so rocprofv3 --kernel-trace --output-format csv -d prof_bytebody -o t -- python tools/gpu_g711_timing.py --trace-worker
    python tools/gpu_g711_timing.py --trace-report prof_main prof_bytebody >> profiles/g711_timing.txt
(tools/ab_libs.sh alternates side builds for bench.py workloads; this launch is no bench workload, hence the two traces.)
   python tools/gpu_g711_timing.py [--out profiles/g711_timing.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

FORMATS = ("s16", "ulaw", "alaw")
CLIENT_RATE, MODEL_RATE, HOP = 8000, 16000, 256
PACKET = HOP * CLIENT_RATE // MODEL_RATE           # client samples of one hop
RING_HOPS = 8


def _law(fmt):
    return None if fmt == "s16" else fmt


def _client_dtype(fmt):
    return torch.int16 if fmt == "s16" else torch.uint8


def _packets(n, fmt, gen):
    from fastenhancer_amd import g711
    pcm = [(0.1 * torch.randn(n, PACKET, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16) for _ in range(8)]
    return pcm if fmt == "s16" else [g711.encode(x, fmt) for x in pcm]


def _run_ticks(pool, slots, packets, ticks, timed):
    total, k = 0.0, len(packets)
    for t in range(ticks):
        x = packets[t % k]
        for s in slots:
            pool.push(s, x[s])
        t0 = time.perf_counter()
        pool.tick()
        t1 = time.perf_counter()
        if timed:
            total += t1 - t0
        for s in slots:
            pool.pull(s)
    return total


class _Launches:
    """the pool's two resampler launches on their own, for one client format: page-locked buffers of the pool's shapes, ring descriptors
    already on the device, a state table per direction"""
    def __init__(self, n, fmt, dev, gen):
        from fastenhancer_amd import g711
        from fastenhancer_amd.resample import Resampler
        self.n, self.law = n, _law(fmt)
        ring = RING_HOPS * HOP
        self.to_model, self.to_client = Resampler(CLIENT_RATE, MODEL_RATE, dev), Resampler(MODEL_RATE, CLIENT_RATE, dev)
        cap = self.to_client.out_count(HOP) + 1
        pcm = (0.1 * torch.randn(n, PACKET, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16)
        self.cin = (pcm if self.law is None else g711.encode(pcm, self.law)).pin_memory()
        self.ring_in = torch.zeros(n, ring, dtype=torch.int16).pin_memory()
        self.ring_out = (0.1 * torch.randn(n, ring, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16).pin_memory()
        self.cout = torch.zeros(n, cap, dtype=_client_dtype(fmt)).pin_memory()
        # the ring side at a position that wraps, as a pool's does every ring_hops ticks
        self.desc_in = self.to_model.pack_ring_desc([(s, PACKET, s * PACKET, s * ring, PACKET, 0, ring, ring - 100) for s in range(n)]).to(dev)
        self.desc_out = self.to_client.pack_ring_desc([(s, HOP, s * ring, s * cap, ring, ring - 100, cap, 0) for s in range(n)]).to(dev)
        self.state_in, self.state_out = self.to_model.new_state(n), self.to_client.new_state(n)

    def model(self):
        kw = {} if self.law is None else {"in_format": self.law}
        self.to_model.step_rings_pinned(self.cin, self.state_in, self.n, self.desc_in, self.ring_in, PACKET, **kw)

    def client(self):
        kw = {} if self.law is None else {"out_format": self.law}
        self.to_client.step_rings_pinned(self.ring_out, self.state_out, self.n, self.desc_out, self.cout, HOP, **kw)


def _time_launch(fn, iters, warm=20):
    """us per launch: `iters` launches between two events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / iters


TRACE_WARM = 20


def trace_worker(args):
    """Table 2's worker, run under rocprofv3: per format the launch to the model's rate, then the launch back, TRACE_WARM + iters each"""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(1)
    for fmt in FORMATS:
        lc = _Launches(args.streams, fmt, dev, gen)
        for fn in (lc.model, lc.client):
            for _ in range(TRACE_WARM + args.iters):
                fn()
            torch.cuda.synchronize()


def trace_report(args):
    """the resampler's kernel rows of each trace directory, in launch order, cut into the worker's six blocks"""
    import csv
    import glob
    blocks = [(fmt, side) for fmt in FORMATS for side in ("to the model's rate", "to the client's rate")]
    per = TRACE_WARM + args.iters
    print("# Table 2: kernel durations in us from rocprofv3 --kernel-trace (a run of its own per library), %d launches per block after %d warm ones,"
          % (args.iters, TRACE_WARM))
    print("# %d streams, the buffers and descriptors of table 1's launches.  bytebody: a side build whose G.711 row goes out as single-byte stores" % args.streams)
    print("# (-DFE_G711_BYTE_BODY) instead of head / 16-byte body / tail; its other kernels are this library's.")
    print(f"{'library':>10} {'format':>6} {'launch':>22} {'mean':>8} {'median':>8} {'min':>8} {'max':>8}  kernel")
    for d in args.trace_report:
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        assert len(files) == 1, (d, files)
        rows = [r for r in csv.DictReader(open(files[0])) if "fe_resample_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        assert len(rows) == per * len(blocks), (d, len(rows), per * len(blocks))
        for i, (fmt, side) in enumerate(blocks):
            blk = rows[i * per + TRACE_WARM:(i + 1) * per]
            us = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in blk])
            names = {r["Kernel_Name"].split("(")[0] for r in blk}
            assert len(names) == 1, names
            tag = os.path.basename(os.path.normpath(d)).replace("prof_", "")
            print(f"{tag:>10} {fmt:>6} {side:>22} {us.mean():>8.2f} {float(np.median(us)):>8.2f} {us.min():>8.2f} {us.max():>8.2f}  {names.pop()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-worker", action="store_true", help="the launches of table 2, to be run under rocprofv3 --kernel-trace")
    ap.add_argument("--trace-report", nargs="+", default=None, metavar="DIR", help="print table 2 from rocprofv3 output directories")
    args = ap.parse_args()
    if args.trace_report:
        return trace_report(args)
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    if args.trace_worker:
        return trace_worker(args)
    from common import hip_model
    from fastenhancer_amd.serving import RingResampledPacketPool
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    n = args.streams
    eng = hip_model("fe_b", device=dev).engine
    pools, launches = {}, {}
    for fmt in FORMATS:
        pool = RingResampledPacketPool(eng, capacity=n, ring_hops=RING_HOPS, client_rate=CLIENT_RATE, T_max=1, max_packet=2 * PACKET, client_format=fmt)
        slots = [pool.open() for _ in range(n)]
        pools[fmt] = (pool, slots, _packets(n, fmt, gen))
        launches[fmt] = _Launches(n, fmt, dev, gen)
    host = {f: [] for f in FORMATS}
    k_in = {f: [] for f in FORMATS}
    k_out = {f: [] for f in FORMATS}
    for rep in range(args.repeats):
        for fmt in FORMATS:
            pool, slots, packets = pools[fmt]
            _run_ticks(pool, slots, packets, args.warmup, timed=False)
            host[fmt].append(1e6 * _run_ticks(pool, slots, packets, args.ticks, timed=True) / args.ticks)
        for fmt in FORMATS:
            k_in[fmt].append(_time_launch(launches[fmt].model, args.iters))
        for fmt in FORMATS:
            k_out[fmt].append(_time_launch(launches[fmt].client, args.iters))
        print(rep, {f: round(host[f][-1], 1) for f in FORMATS}, {f: round(k_in[f][-1], 2) for f in FORMATS}, {f: round(k_out[f][-1], 2) for f in FORMATS}, flush=True)
    # the three pools ran the G.711 kernels where they should, and consumed the same number of samples
    back = {}
    for fmt in FORMATS:
        pool, slots, packets = pools[fmt]
        assert pool.to_model.last_kernel() == pool.to_client.last_kernel() == ("fe_resample_kernel<ring,pinned>" if fmt == "s16" else "fe_resample_kernel<ring,pinned,g711>")
        back[fmt] = sum(int(pool._consumed[s]) for s in slots)
    assert len(set(back.values())) == 1

    def table(title, rows):
        lines = [title, f"{'format':>8} " + " ".join(f"{f'#{r + 1}':>9}" for r in range(args.repeats)) + " " + " ".join(f"{f'/s16 #{r + 1}':>9}" for r in range(args.repeats))
                 + f" {'mean /s16':>10}"]
        for fmt in FORMATS:
            ratios = [a / b for a, b in zip(rows[fmt], rows["s16"])]
            lines.append(f"{fmt:>8} " + " ".join(f"{v:>9.2f}" for v in rows[fmt]) + " " + " ".join(f"{v:>9.3f}" for v in ratios) + f" {float(np.mean(ratios)):>10.3f}")
        s = rows["s16"]
        lines.append(f"# spread of the s16 rounds: (max - min) / mean = {100.0 * (max(s) - min(s)) / float(np.mean(s)):.2f} %")
        return lines

    lines = [f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"# RingResampledPacketPool, FastEnhancer_B, {n} streams, clients at 8 kHz, one hop ({PACKET} client samples) per stream and tick, T_max = 1,",
             f"# ring_hops = {RING_HOPS}.  The three client formats alternate in one process, {args.repeats} rounds; /s16 = the format's figure over the s16 figure of the",
             f"# same round."]
    lines += table(f"# Table 1a: host wall time of tick() in us ({args.warmup} untimed, {args.ticks} timed ticks per block; each tick ends in its synchronise)", host)
    lines += table(f"# Table 1b: the launch to the model's rate, fe_resample_rings_pinned client staging -> int16 rings, us from launch to launch ({args.iters} launches between two events, the host's enqueue included)", k_in)
    lines += table(f"# Table 1c: the launch to the client's rate, fe_resample_rings_pinned int16 rings -> client staging, us from launch to launch ({args.iters} launches between two events, the host's enqueue included)", k_out)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
