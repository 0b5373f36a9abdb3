#!/usr/bin/env python3
"""What a tick of serving.RingResampledPacketPool costs on the host, next to ResampledPacketPool's: the wall time of tick() - which ends in its
(last) synchronise - with every stream fed one 20 ms int16 packet before each tick (the pushes and pulls are outside the timed region).
Both pools live in one process, on one engine, and ALTERNATE: a block of `--ticks` timed ticks of one (after `--warmup` untimed ones), then of
the other, for each configuration; the whole alternation is then run `--repeats` times and the spread of a configuration is the largest
relative difference of its per-run ratio.  FastEnhancer_B with clients at 8 kHz and at 48 kHz at 1, 32 and 256 streams, and FSPEN
(FamilyPacketPool, meters on) with clients at 48 kHz at 256 streams.
   python tools/gpu_ring_resample_timing.py [--out profiles/ring_resample_timing.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import hip_model  # noqa: E402
from fastenhancer_amd.serving import FamilyPacketPool, ResampledPacketPool, RingResampledPacketPool  # noqa: E402


class _FamilyOracle(ResampledPacketPool):
    """ResampledPacketPool over a FamilyPacketPool with meters, by its hook"""
    @staticmethod
    def _make_pool(engine, capacity, ring_hops, T_max):
        return FamilyPacketPool(engine, capacity, ring_hops, T_max=T_max, meters=True)


def _pools(eng, family, n, client_rate):
    kw = dict(capacity=n, ring_hops=8, client_rate=client_rate, T_max=2, max_packet=2 * (client_rate // 50))
    if family:
        return _FamilyOracle(eng, **kw), RingResampledPacketPool(eng, pool=FamilyPacketPool, meters=True, **kw)
    return ResampledPacketPool(eng, **kw), RingResampledPacketPool(eng, **kw)


def _run(pool, slots, packets, ticks, timed):
    """`ticks` ticks, a packet per stream before each; the summed wall time of the tick() calls in seconds (0.0 when not timed)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    engines = {"fe_b": hip_model("fe_b", device=dev).engine, "fspen": hip_model("fspen", device=dev).engine}
    configs = [("fe_b", False, rate, n) for rate in (8000, 48000) for n in (1, 32, 256)] + [("fspen", True, 48000, 256)]
    built = []
    for name, family, rate, n in configs:
        old, new = _pools(engines[name], family, n, rate)
        slots = [old.open() for _ in range(n)]
        assert [new.open() for _ in range(n)] == slots
        packets = [(0.1 * torch.randn(n, rate // 50, generator=gen) * 32768).round().clamp(-32768, 32767).to(torch.int16) for _ in range(8)]
        built.append((old, new, slots, packets))
    results = [[] for _ in configs]          # per configuration: (us per tick old, new) per repeat
    for rep in range(args.repeats):
        for i, (old, new, slots, packets) in enumerate(built):
            us = []
            for pool in (old, new):
                _run(pool, slots, packets, args.warmup, timed=False)
                us.append(1e6 * _run(pool, slots, packets, args.ticks, timed=True) / args.ticks)
            results[i].append(tuple(us))
            print(configs[i], rep, "%.1f %.1f" % tuple(us), flush=True)
    # the two pools were fed the same packets in the same order: the same audio must have come back
    for (name, family, rate, n), (old, new, slots, packets) in zip(configs, built):
        for pool in (old, new):
            for s in slots:
                pool.push(s, packets[0][s])
            pool.tick()
        assert all(torch.equal(old.pull(s), new.pull(s)) for s in slots), (name, rate, n)
    lines = [f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"# host wall time of tick() in us (time.perf_counter around the call; each tick ends in its synchronise), a 20 ms int16 packet per stream",
             f"# before every tick, pushes and pulls outside the timed region; T_max = 2, ring_hops = 8.  Per configuration the two pools alternate in the",
             f"# same process: {args.warmup} untimed and {args.ticks} timed ticks of ResampledPacketPool (old), then of RingResampledPacketPool (ring); the whole",
             f"# alternation over all configurations is run {args.repeats} times.  ratio = old / ring per run; spread = (max - min) / mean of the runs' ratios.",
             f"{'model':>6} {'inner pool':>22} {'client':>7} {'streams':>7} " + " ".join(f"{f'old #{r + 1}':>9} {f'ring #{r + 1}':>9} {f'ratio #{r + 1}':>9}" for r in range(args.repeats))
             + f" {'ratio':>7} {'spread %':>9}"]
    for (name, family, rate, n), res in zip(configs, results):
        ratios = [a / b for a, b in res]
        mean = float(np.mean(ratios))
        spread = 100.0 * (max(ratios) - min(ratios)) / mean
        cells = " ".join(f"{a:>9.1f} {b:>9.1f} {a / b:>9.3f}" for a, b in res)
        lines.append(f"{name:>6} {'FamilyPacketPool+meters' if family else 'PacketPool':>22} {rate:>7} {n:>7} {cells} {mean:>7.3f} {spread:>9.2f}")
    lines.append(f"# kernels of the ring pool's last tick: {built[0][1].to_model.last_kernel()}, {engines['fe_b'].last_step_kernel()}, {built[0][1].to_client.last_kernel()}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
