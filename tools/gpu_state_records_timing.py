#!/usr/bin/env python3
"""Moving n of 256 streams from one state buffer to another (export + import of their state records), two ways:
  (a) fe_state_export_slots + fe_state_import_slots: one launch each;
  (b) the mover a user could write without them: per state tensor of the documented layout (include/fastenhancer_hip.h), torch.index_select
      on a [rows, capacity, len] view into the records and index_copy_ from them into the destination's view.
Both produce the same records and the same destination state (checked on the bits before anything is timed).  Device events around
`--iters` moves after `--warmup` moves of each form; the forms alternate in rounds (`--rounds`) and each cell is the median over rounds.
Bytes moved = the records' bytes, once out and once in (every byte is read once and written once on each leg); GB/s = that over the time.
   python tools/gpu_state_records_timing.py [--out profiles/state_records_timing.txt] [--models fe_b,fe_dpt_b,bsrnn_xt] [--n 64,256]"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import BSRNN_KWARGS, hip_engine, product_config  # noqa: E402


def regions(name):
    """[(rows, len)]: the state of B streams is these tensors back to back, each [rows][B][len] (the header's layout)"""
    if name in BSRNN_KWARGS:
        kw = BSRNN_KWARGS[name][0]
        return [(1, 256), (1, 256), (2 * kw["num_layers"], 31 * 2 * kw["num_channels"])]
    c = product_config(name)
    r = [(1, c.n_fft - c.hop_size)] * 2
    if c.dpt:
        r += [(2 * c.rf_blocks, c.rf_freq * c.rf_channels * c.lookbehind), (1, 1)]
    else:
        r += [(c.rf_blocks, c.rf_freq * c.rf_channels)]
    if c.time_kernel:
        r += [(2 * c.n_layers, (c.kernel_size_time - 1) * c.F1 * c.channels)]
    return r


def views(name, state, cap):
    out, off = [], 0
    for rows, ln in regions(name):
        out.append(state[off:off + rows * cap * ln].view(rows, cap, ln))
        off += rows * cap * ln
    assert off == state.numel()
    return out


def record_views(name, rec):
    """the same tensors inside n records [n, record_floats]: [rows, n, len] views (a record is the capacity-1 layout)"""
    out, off = [], 0
    for rows, ln in regions(name):
        out.append(rec[:, off:off + rows * ln].view(rec.shape[0], rows, ln).transpose(0, 1))
        off += rows * ln
    assert off == rec.shape[1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="fe_b,fe_dpt_b,bsrnn_xt")
    ap.add_argument("--capacity", type=int, default=256)
    ap.add_argument("--n", default="64,256")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU timing is reported"
    dev = torch.device("cuda:0")
    cap = args.capacity
    lines = [f"# export + import of n of {cap} streams' state records; median over {args.rounds} alternating rounds of {args.iters} moves "
             f"(device events, {args.warmup} warm-up moves per form and round)",
             f"# device: {torch.cuda.get_device_name(dev)}, {torch.cuda.get_device_properties(dev).multi_processor_count} CUs",
             f"{'model':>10} {'n':>4} {'record KB':>10} {'MB moved':>9} {'(a) two launches us':>20} {'GB/s':>7} {'(b) torch mover us':>19} {'GB/s':>7} {'(b)/(a)':>8}"]
    for name in args.models.split(","):
        eng = hip_engine(name, dev)     # (no weights: state does not depend on them)
        rf = eng.record_floats
        gen = torch.Generator(device=dev).manual_seed(0)
        src = torch.randn(eng.state_floats(cap), device=dev, generator=gen)
        dst_a, dst_b = torch.zeros_like(src), torch.zeros_like(src)
        rng = np.random.default_rng(1)
        for n in [int(v) for v in args.n.split(",")]:
            frm = torch.tensor(rng.permutation(cap)[:n], dtype=torch.int32, device=dev)
            to = torch.tensor(rng.permutation(cap)[:n], dtype=torch.int32, device=dev)
            frm_l, to_l = frm.long(), to.long()
            rec_a, rec_b = torch.zeros(n, rf, device=dev), torch.zeros(n, rf, device=dev)
            src_v, dst_v, rec_v = views(name, src, cap), views(name, dst_b, cap), record_views(name, rec_b)

            def form_a():
                eng.export_slots(src, cap, frm, out=rec_a)
                eng.import_slots(dst_a, cap, to, rec_a)

            def form_b():
                for sv, rv in zip(src_v, rec_v):
                    rv.copy_(torch.index_select(sv, 1, frm_l))
                for dv, rv in zip(dst_v, rec_v):
                    dv.index_copy_(1, to_l, rv)

            forms = [form_a, form_b]
            dst_a.zero_(), dst_b.zero_()
            for f in forms:
                f()
            torch.cuda.synchronize()
            assert torch.equal(rec_a.view(torch.int32), rec_b.view(torch.int32)), f"{name} n={n}: the two movers' records differ"
            assert torch.equal(dst_a.view(torch.int32), dst_b.view(torch.int32)), f"{name} n={n}: the two movers' destinations differ"
            assert float(dst_a.abs().max()) > 0
            times = [[] for _ in forms]
            for _ in range(args.rounds):
                for i, f in enumerate(forms):
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
            spread = [100.0 * (max(t) - min(t)) / float(np.median(t)) for t in times]
            moved = 2 * n * rf * 4
            lines.append(f"{name:>10} {n:>4} {rf * 4 / 1024:>10.1f} {moved / 1e6:>9.2f} {med[0]:>14.1f} ({spread[0]:.0f}%) {moved / med[0] / 1e3:>7.1f} "
                         f"{med[1]:>13.1f} ({spread[1]:.0f}%) {moved / med[1] / 1e3:>7.1f} {med[1] / med[0]:>8.2f}")
            print(lines[-1], flush=True)
        del src, dst_a, dst_b
    lines.append("# (x%): spread (max - min) / median of the rounds; (b)/(a) > 1: the two launches are the faster")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
