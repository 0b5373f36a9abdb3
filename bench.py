#!/usr/bin/env python3
"""bench.py — enhanced audio frames/s of the FastEnhancer streaming forward path on MI355X.

One "step" = one pass of the hot path (scripts/export_onnx.py:48-58 of the reference: STFT ->
model -> iSTFT with all caches) over one batch of synthetic input: ONE hop of H new samples for
each of the B concurrent streams of this GPU (`--frames-per-step T` makes a step T hops per
stream in one launch).  Workload = BASELINE.json configs[1]: FastEnhancer_B, 16 kHz, N=512,
H=256, B=256 concurrent streams per GPU.  Multi-GPU: one process per GPU, the streams are
sharded (256 per rank, weak scaling), the fused weight blob is broadcast once from rank 0 over
RCCL, and there is no per-step collective (streams are independent).

Prints ONE JSON line on rank 0 (contract in the task statement) with `roofline` and
`cpu_baseline` objects.  Inputs are resident in HBM before the timed region.  `--steps K` is the
number of timed steps (one block of K unless `--blocks` asks for more); `--dump-outputs DIR`
writes what the last timed step returned, for comparing two builds output for output."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from fastenhancer_amd import _lib  # noqa: E402
from fastenhancer_amd.config import FEConfig  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from fastenhancer_amd.parallel import broadcast_blob, shard_range, synthetic_streams  # noqa: E402

PEAK_FP32_TFLOPS = 157.3   # MI355X_MICROARCH.md: fp32 vector == fp32-input MFMA peak (256 CU x 2.4 GHz)

WORKLOADS = {
    # name: (model_kwargs builder args, sampling rate, description)
    "fe_b": dict(C1=48, ks=(8, 3, 3), C2=36, F2=24, K=3, N=512, H=256, sr=16000, init="linear_fixed",
                 desc="FastEnhancer_B 16kHz"),
    "fe_t": dict(C1=24, ks=(8, 3, 3), C2=20, F2=16, K=2, N=512, H=256, sr=16000, init="linear_fixed",
                 desc="FastEnhancer_T 16kHz"),
    "fe_s": dict(C1=64, ks=(8, 3, 3, 3), C2=48, F2=36, K=3, N=512, H=256, sr=16000, init="linear_fixed",
                 desc="FastEnhancer_S 16kHz"),
    "fe48_b": dict(C1=48, ks=(8, 3, 3), C2=36, F2=36, K=3, N=1024, H=512, sr=48000, init="linear",
                   desc="FastEnhancer_B 48kHz"),
    "fe48_b_h480": dict(C1=48, ks=(8, 3, 3), C2=36, F2=36, K=3, N=1024, H=480, sr=48000, init="linear",
                        desc="FastEnhancer_B 48kHz at a 10 ms hop (BASELINE config 4 wording)"),
    "fe48_l": dict(C1=128, ks=(8, 3, 3, 3, 3), C2=96, F2=96, K=5, N=1024, H=200, sr=48000, init="linear",
                   desc="FastEnhancer_L 48kHz"),
    "fe48_t": dict(C1=24, ks=(8, 3, 3), C2=20, F2=24, K=2, N=1024, H=512, sr=48000, init="linear",
                   desc="FastEnhancer_T 48kHz"),
    "fe48_s": dict(C1=64, ks=(8, 3, 3, 3), C2=48, F2=48, K=3, N=1024, H=512, sr=48000, init="linear",
                   desc="FastEnhancer_S 48kHz"),
    "fe48_m": dict(C1=96, ks=(8, 3, 3, 3), C2=72, F2=72, K=4, N=1024, H=320, sr=48000, init="linear",
                   desc="FastEnhancer_M 48kHz"),
    "bsrnn_xt": dict(bsrnn=True, C=16, L=6, N=512, H=256, sr=16000, desc="BSRNN (xt) 16kHz"),
    "bsrnn_xxt": dict(bsrnn=True, C=16, L=2, N=512, H=256, sr=16000, desc="BSRNN (xxt) 16kHz"),
    "bsrnn_t": dict(bsrnn=True, C=32, L=6, N=512, H=256, sr=16000, desc="BSRNN (t) 16kHz"),
    "bsrnn_s": dict(bsrnn=True, C=64, L=6, N=512, H=256, sr=16000, desc="BSRNN (s) 16kHz"),
    "fspen": dict(fspen=True, N=512, H=256, sr=16000, desc="FSPEN 16kHz (configs/others/fspen.yaml)"),
    "lisennet": dict(lisennet=True, N=512, H=256, sr=16000, desc="LiSenNet 16kHz (configs/others/lisennet.yaml)"),
    "fe_m": dict(C1=96, ks=(8, 3, 3, 3), C2=72, F2=48, K=4, N=512, H=160, sr=16000, init="linear_fixed",
                 desc="FastEnhancer_M 16kHz"),
    "fe_l": dict(C1=128, ks=(8, 3, 3, 3, 3), C2=96, F2=64, K=5, N=512, H=100, sr=16000, init="linear_fixed",
                 desc="FastEnhancer_L 16kHz"),
    "fe_tk_b": dict(C1=48, ks=(8, 3, 3), kt=3, C2=36, F2=24, K=3, N=512, H=256, sr=16000, init="linear_fixed",
                    desc="FastEnhancer_B with a 3-frame causal time kernel (configs/ablation/time_kernel_b.yaml)"),
    # the dprnn ablation (configs/ablation/dprnn_{t,b,l}.yaml): a bidirectional GRU over the sub-bands instead of the attention
    "fe_dprnn_t": dict(C1=24, ks=(8, 3, 3), frnn=10, C2=20, F2=16, K=2, N=512, H=256, sr=16000, init="linear_fixed", desc="FastEnhancer_T, dprnn blocks"),
    "fe_dprnn_b": dict(C1=48, ks=(8, 3, 3), frnn=18, C2=36, F2=24, K=3, N=512, H=256, sr=16000, init="linear_fixed", desc="FastEnhancer_B, dprnn blocks"),
    # the dptransformer ablation (configs/ablation/dpt_{t,b,s,m}.yaml): causal attention over the last 31 frames instead of the time GRU;
    # its K / V caches make the step HBM-bound (`roofline.hbm_frac`)
    "fe_dpt_t": dict(C1=24, ks=(8, 3, 3), dpt=31, C2=20, F2=16, K=2, N=512, H=256, sr=16000, init="linear_fixed", desc="FastEnhancer_T, dual-path transformer blocks"),
    "fe_dpt_b": dict(C1=48, ks=(8, 3, 3), dpt=31, C2=36, F2=24, K=3, N=512, H=256, sr=16000, init="linear_fixed", desc="FastEnhancer_B, dual-path transformer blocks"),
    "fe_dpt_s": dict(C1=64, ks=(8, 3, 3, 3), dpt=31, C2=48, F2=36, K=3, N=512, H=256, sr=16000, init="linear_fixed", desc="FastEnhancer_S, dual-path transformer blocks"),
    "fe_dpt_m": dict(C1=96, ks=(8, 3, 3, 3), dpt=31, C2=72, F2=48, K=4, N=512, H=160, sr=16000, init="linear_fixed", desc="FastEnhancer_M, dual-path transformer blocks"),
    # model: fastenhancer.noncausal (configs/fastenhancer_dns/huge_noncausal.yaml, configs/fastenhancer_48khz/huge_noncausal.yaml): bidirectional
    # GRU over time, offline Model.forward only (--offline-seconds is implied), time-batched engine
    "fe_nc": dict(C1=128, ks=(8, 3, 3, 3, 3, 3), nc=True, C2=128, F2=64, K=6, N=512, H=100, sr=16000, init="linear_fixed",
                  desc="FastEnhancer huge noncausal 16kHz"),
    "fe48_nc": dict(C1=128, ks=(8, 3, 3, 3, 3, 3), nc=True, C2=128, F2=64, K=6, N=1024, H=200, sr=48000, init="linear",
                    desc="FastEnhancer huge noncausal 48kHz"),
    "fe_ln_b": dict(C1=48, ks=(8, 3, 3), ln=True, C2=36, F2=24, K=3, N=512, H=256, sr=16000, init="linear_fixed",
                    desc="FastEnhancer_B with GroupNorm / LayerNorm (configs/ablation/ln_b.yaml)"),
    "fe_dprnn_s": dict(C1=64, ks=(8, 3, 3, 3), frnn=24, C2=48, F2=36, K=3, N=512, H=256, sr=16000, init="linear_fixed", desc="FastEnhancer_S, dprnn blocks"),
    "fe_dprnn_m": dict(C1=96, ks=(8, 3, 3, 3), frnn=36, C2=72, F2=48, K=4, N=512, H=160, sr=16000, init="linear_fixed", desc="FastEnhancer_M, dprnn blocks"),
    "fe_dprnn_l": dict(C1=128, ks=(8, 3, 3, 3, 3), frnn=48, C2=96, F2=64, K=5, N=512, H=100, sr=16000, init="linear_fixed",
                       desc="FastEnhancer_L, dprnn blocks"),
}


def model_kwargs(w):
    if w.get("lisennet"):
        return dict(num_channels=16, n_blocks=2, n_fft=w["N"], hop_size=w["H"], win_size=w["N"], input_compression=0.3)
    if w.get("fspen"):
        return dict(channels=[4, 16, 32], kernel_size=[6, 8, 6], stride=[2, 2, 2],
                    dpe_kwargs=dict(num_blocks=3, channels=16, freq=32, groups=8, norm="LayerNorm-FreqChannels"),
                    n_fft=w["N"], hop_size=w["H"], win_size=w["N"], window="hann", input_compression=0.3)
    if w.get("bsrnn"):
        return dict(num_channels=w["C"], num_layers=w["L"], bias=True, affine=True, n_fft=w["N"], hop_size=w["H"], win_size=w["N"],
                    window="hann", input_compression=0.3)
    if w.get("ln"):
        kw = model_kwargs({k: v for k, v in w.items() if k != "ln"})
        kw.update(final_scale=True, final_scale_init="one")
        return kw
    if w.get("nc"):
        return model_kwargs({k: v for k, v in w.items() if k != "nc"})
    if w.get("dpt"):
        kw = model_kwargs({k: v for k, v in w.items() if k != "dpt"})
        rk = kw.pop("rnnformer_kwargs")
        del kw["resnet"]
        kw.update(dpt_kwargs=dict(rk, lookbehind=w["dpt"]), final_scale=True, final_scale_init="one")
        return kw
    if w.get("frnn"):
        kw = model_kwargs({k: v for k, v in w.items() if k != "frnn"})
        del kw["rnnformer_kwargs"], kw["resnet"]
        kw.update(dprnn_kwargs=dict(num_blocks=w["K"], channels=w["C2"], channels_frnn=w["frnn"], freq=w["F2"], eps=1e-5, pre_norm=False), final_scale=True)
        return kw
    if w.get("kt"):
        kw = model_kwargs({k: v for k, v in w.items() if k != "kt"})
        del kw["kernel_size"], kw["resnet"]
        kw.update(kernel_size_freq=list(w["ks"]), kernel_size_time=w["kt"], final_scale=True)
        return kw
    return dict(channels=w["C1"], kernel_size=list(w["ks"]), stride=4,
                rnnformer_kwargs=dict(num_blocks=w["K"], channels=w["C2"], freq=w["F2"], num_heads=4, eps=1e-5,
                                      positional_embedding="train", attn_bias=False, post_act=False, pre_norm=False),
                pre_post_init=w["init"], n_fft=w["N"], hop_size=w["H"], win_size=w["N"], window="hann",
                stft_normalized=False, mask=None, activation="SiLU", activation_kwargs=dict(inplace=True),
                input_compression=0.3, normalize_final_conv=True, weight_norm=True, resnet=False)


def cpu_baseline(workload: str, kw: dict, sr: int, B: int, budget_s: float):
    """The C/OpenMP oracle (oracle/fe_oracle.c, a port of the reference algorithm pinned on the reference's golden
    vectors) timed on the host cores of this box on a bounded sample of the same workload: the same B streams, one
    OpenMP thread per logical core, as many hops as fit in the budget."""
    from oracle.c_oracle import COracle
    from oracle.fe_oracle import FEConfig as OCfg, fold_state_dict
    from oracle.weightgen import make_input, make_training_state_dict
    cfg = OCfg.from_model_kwargs(kw)
    fused = fold_state_dict(make_training_state_dict(cfg, 2), cfg)
    H = cfg.hop_size
    x = make_input(B, 64 * H, 1236, sr)
    avail, quota = host_cpus()
    # the OpenMP width is bounded by the container's CPU quota (cgroup cpu.max), not by the logical cores the host shows:
    # on the round-2 GPU boxes 256 logical cores are visible but the quota is 16 CPUs - the oracle scales 14.9x from 1 to
    # 16 threads and is throttled beyond (tools/cpu_scaling_probe.py); try the widths up to the quota, report the fastest
    cap = avail if quota is None else max(1, min(avail, int(quota + 0.5)))
    cands = sorted({min(cap, c) for c in (max(1, cap // 2), cap)} | ({min(avail, 2 * cap)} if quota is not None else set()))
    best = None
    for threads in cands:
        co = COracle(cfg, fused, threads=threads)
        cs, ci, h = co.initialize_cache(B)
        co.step(x[:, :H], cs, ci, h)                      # warm-up hop
        t0 = time.perf_counter()
        hops = 0
        while (time.perf_counter() - t0) < budget_s / len(cands):
            t = hops % 64
            co.step(x[:, t * H:(t + 1) * H], cs, ci, h)
            hops += 1
        dt = time.perf_counter() - t0
        rate = B * hops / dt
        if best is None or rate > best[0]:
            best = (rate, threads, hops, dt)
    rate, threads, hops, dt = best
    return {"value": rate, "unit": "frames/s", "cores": int(threads), "kind": "port",
            "sample": f"{hops} hops x {B} streams of {workload} through the C/OpenMP oracle (oracle/fe_oracle.c) in {dt:.1f} s with "
                      f"{threads} OpenMP threads (fastest of {cands}; the host shows {avail} logical cores, the container's "
                      f"cgroup CPU quota is {'unlimited' if quota is None else f'{quota:g} CPUs'})"}


def host_cpus():
    """(logical cores this process may run on, cgroup CPU quota in CPUs or None)"""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = float(q) / float(period)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / period
        except Exception:
            pass
    return avail, quota


def cpu_baseline_variant(kw: dict, sr: int, B: int, budget_s: float, variant=None):
    """The time_kernel / dprnn / dptransformer variants: the numpy oracle (oracle/fe_oracle.py, pinned on the reference's golden
    vectors of each variant; the C/OpenMP oracle restates the default model only) on ONE host core."""
    from oracle.fe_oracle import FEConfig as OCfg, FEOracle, fold_state_dict
    from oracle.weightgen import make_input, make_training_state_dict
    cfg = OCfg.from_model_kwargs(kw, variant=variant)
    orc = FEOracle(cfg, fold_state_dict(make_training_state_dict(cfg, 2), cfg), np.float32)
    Bs = min(B, 16)
    H = cfg.hop_size
    x = make_input(Bs, 64 * H, 5, sr)
    caches = orc.initialize_cache(Bs)
    t0 = time.perf_counter()
    hops = 0
    while hops < 64 and (hops < 2 or time.perf_counter() - t0 < budget_s):
        _, *caches = orc.step(x[:, hops * H:(hops + 1) * H], *caches)
        hops += 1
    dt = time.perf_counter() - t0
    return {"value": hops * Bs / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"{hops} hops x {Bs} streams through the numpy oracle (oracle/fe_oracle.py) in {dt:.1f} s on one core"}


def cpu_baseline_fspen(kw: dict, sr: int, B: int, budget_s: float, lisennet: bool = False):
    """FSPEN / LiSenNet: the numpy oracle (oracle/fspen_oracle.py, oracle/lisennet_oracle.py, pinned on the reference's golden vectors)
    on ONE host core."""
    from oracle.weightgen import make_input
    try:
        torch.set_num_threads(1)
    except Exception:
        pass
    if lisennet:
        from oracle import lisennet_oracle as lo
        cfg = lo.LiSenNetConfig.from_model_kwargs(kw)
        orc = lo.LiSenNetOracle(cfg, lo.make_state_dict(cfg, 2), np.float32)
    else:
        from oracle import fspen_oracle as fo
        cfg = fo.FSPENConfig.from_model_kwargs(kw)
        orc = fo.FSPENOracle(cfg, fo.fold_state_dict(fo.make_training_state_dict(cfg, 2), cfg), np.float32)
    Bs = min(B, 16)
    H = cfg.hop_size
    x = make_input(Bs, 64 * H, 5, sr)
    caches = orc.initialize_cache(Bs)
    t0 = time.perf_counter()
    hops = 0
    while hops < 64 and (hops < 2 or time.perf_counter() - t0 < budget_s):
        _, *caches = orc.step(x[:, hops * H:(hops + 1) * H], *caches)
        hops += 1
    dt = time.perf_counter() - t0
    return {"value": hops * Bs / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"{hops} hops x {Bs} streams of {'lisennet' if lisennet else 'fspen'} through the numpy oracle "
                      f"(oracle/{'lisennet' if lisennet else 'fspen'}_oracle.py) in {dt:.1f} s on one host core"}


def cpu_baseline_bsrnn(workload: str, kw: dict, sr: int, B: int, budget_s: float):
    """BSRNN workloads: the numpy oracle (oracle/bsrnn_oracle.py, pinned on the reference's golden vectors) on ONE host
    core (BLAS threads limited to 1: a scalar port, stated as such), on a bounded sample of the same workload."""
    from oracle import bsrnn_oracle as bo
    from oracle.weightgen import make_input
    try:
        from threadpoolctl import threadpool_limits
    except Exception:
        threadpool_limits = None
    cfg = bo.BSRNNConfig.from_model_kwargs(kw)
    orc = bo.BSRNNOracle(cfg, bo.fold_state_dict(bo.make_training_state_dict(cfg, 2), cfg), np.float32)
    H = cfg.hop_size
    Bs = min(B, 64)                                   # a 64-stream sample keeps a hop under a second
    x = make_input(Bs, 8 * H, 1236, sr)
    ctx = threadpool_limits(limits=1) if threadpool_limits else None
    try:
        caches = orc.initialize_cache(Bs)
        _, *caches = orc.step(x[:, :H], *caches)
        t0 = time.perf_counter()
        hops = 0
        while (time.perf_counter() - t0) < budget_s:
            t = hops % 8
            _, *caches = orc.step(x[:, t * H:(t + 1) * H], *caches)
            hops += 1
        dt = time.perf_counter() - t0
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return {"value": Bs * hops / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"{hops} hops x {Bs} streams of {workload} through the numpy oracle (oracle/bsrnn_oracle.py) in {dt:.1f} s on one "
                      f"core (BLAS limited to 1 thread{'' if threadpool_limits else ' - threadpoolctl missing, not enforced'})"}


def cpu_baseline_offline_numpy(kw: dict, sr: int, budget_s: float):
    """The numpy oracle's offline Model.forward (oracle/fe_oracle.py, pinned on the reference's golden vectors) of the noncausal model,
    on the host cores numpy's BLAS uses, on a bounded sample: one utterance whose length is doubled until a call takes a few seconds."""
    from oracle.fe_oracle import FEConfig as OCfg, FEOracle, fold_state_dict
    from oracle.weightgen import make_input, make_training_state_dict
    cfg = OCfg.from_model_kwargs(kw, variant="noncausal")
    orc = FEOracle(cfg, fold_state_dict(make_training_state_dict(cfg, 2), cfg))
    secs, best = 0.25, None
    t_all = time.perf_counter()
    while True:
        x = make_input(1, int(secs * sr), 1236, sr)
        t0 = time.perf_counter()
        orc.offline_forward(x)
        dt = time.perf_counter() - t0
        best = ((1 + x.shape[1] // cfg.hop_size) / dt, secs, dt)
        if dt > budget_s / 4 or time.perf_counter() - t_all > budget_s / 2:
            break
        secs *= 2
    return {"value": best[0], "unit": "frames/s", "cores": os.cpu_count(), "kind": "port",
            "sample": f"numpy oracle (oracle/fe_oracle.py::offline_forward, BLAS threads as configured), one utterance of {best[1]:g} s in {best[2]:.2f} s"}


def parity_after_timed_region(workload: str, w: dict, kw: dict, sd: dict, eng, B: int, x_hop: np.ndarray, caches_in, out_gpu: np.ndarray, caches_out):
    """Outside the timed blocks: the launch the bench times (same handle, same kernel, same B, per-hop) is issued ONCE more from the state the
    timed run left behind; the oracle steps ALL B streams from that same state on the same input hop.  Returns the relative rms error of the
    enhanced hop and the largest one over the returned caches.  The oracle (oracle/: test infrastructure) is the checker here, nothing else."""
    def rms(a):
        return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))
    caches_in = [np.ascontiguousarray(c, dtype=np.float32) for c in caches_in]
    if w.get("bsrnn"):
        from oracle import bsrnn_oracle as bo
        orc = bo.BSRNNOracle(bo.BSRNNConfig.from_model_kwargs(kw), {k: v.numpy() for k, v in sd.items()}, np.float32)
        what = "oracle/bsrnn_oracle.py"
    elif w.get("fspen"):
        from oracle import fspen_oracle as fo
        orc = fo.FSPENOracle(fo.FSPENConfig.from_model_kwargs(kw), {k: v.numpy() for k, v in sd.items()}, np.float32)
        what = "oracle/fspen_oracle.py"
    elif w.get("lisennet"):
        from oracle import lisennet_oracle as lo
        orc = lo.LiSenNetOracle(lo.LiSenNetConfig.from_model_kwargs(kw), {k: v.numpy() for k, v in sd.items()}, np.float32)
        what = "oracle/lisennet_oracle.py"
    else:
        from oracle.fe_oracle import FEConfig as OCfg, FEOracle
        variant = "time_kernel" if w.get("kt") else "dprnn" if w.get("frnn") else "dptransformer" if w.get("dpt") else "ln" if w.get("ln") else None
        ocfg = OCfg.from_model_kwargs(kw, variant=variant)
        fused = {k: v.numpy() for k, v in sd.items()}
        if variant is None:
            from oracle.c_oracle import COracle
            co = COracle(ocfg, fused, threads=max(1, min(8, host_cpus()[0])))
            cs, ci = caches_in[0].copy(), caches_in[1].copy()
            h = np.ascontiguousarray(np.concatenate(caches_in[2:], axis=0))          # K x [1, B*F2, C2] -> [K, B*F2, C2]
            ref_out = co.step(x_hop, cs, ci, h)                                       # (in place on the caches)
            ref_caches = [cs, ci] + [h[k:k + 1] for k in range(h.shape[0])]
            what = "oracle/fe_oracle.c"
            orc = None
        else:
            orc = FEOracle(ocfg, fused, np.float32)
            what = "oracle/fe_oracle.py"
    if orc is not None:
        ref_out, *ref_caches = orc.step(x_hop, *caches_in)
    r_out = rms(out_gpu - ref_out) / max(rms(ref_out), 1e-12)
    r_cache = max(rms(np.asarray(a).reshape(-1) - np.asarray(b).reshape(-1)) / max(rms(b), 1e-3) for a, b in zip(caches_out, ref_caches))
    return r_out, r_cache, what


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(arrays: dict, out_dir: str, limit: int = DUMP_LIMIT_BYTES, seed: int = 0) -> dict:
    """--dump-outputs: every array as <out_dir>/<name>.npy in float32.  When they hold more than `limit` bytes in all, every array keeps the
    same fraction of its elements, flattened: one seeded random index in each of k equal strata of its flat indices (ascending, distinct) -
    the same elements for the same arguments."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
    budget = limit - 4096 * len(arrays)                       # (room for the .npy headers)
    total = sum(a.nbytes for a in arrays.values())
    frac = 1.0 if total <= budget else budget / total
    shapes = {}
    for i, name in enumerate(sorted(arrays)):
        a = arrays[name]
        if frac < 1.0:
            k = int(a.size * frac)
            stride = a.size / max(k, 1)
            idx = ((np.arange(k) + np.random.default_rng([seed, i]).random(k)) * stride).astype(np.int64)
            a = a.reshape(-1)[np.minimum(idx, a.size - 1)]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        shapes[name] = list(arrays[name].shape)
    return {"dir": out_dir, "arrays": shapes, "sampled_fraction": None if frac >= 1.0 else frac}


# rocprofv3's FETCH_SIZE on gfx950 reports HALF of the bytes read, at every access width the kernels use and for cache-resident as
# well as HBM-sourced data; WRITE_SIZE is exact, partial lines included (profiles/r5_hbm_counter_calib.txt: known byte counts in the
# kernels' own access patterns, tools/micro/hbm_counter_calib.hip).  Traffic = 2 x FETCH_SIZE + WRITE_SIZE.
FETCH_SIZE_FACTOR, WRITE_SIZE_FACTOR = 2.0, 1.0


def measured_traffic(workload: str, B: int, T: int):
    """(HBM-side bytes per launch, source text) from the PMC passes committed under profiles/ (FETCH_SIZE / WRITE_SIZE) for exactly this
    configuration - the newest round's file wins - with the calibrated counter factors applied; (None, None) if there is none."""
    best = None
    pdir = os.path.join(REPO, "profiles")
    for name in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        if name.startswith("pmc_") and name.endswith(".json"):
            try:
                d = json.load(open(os.path.join(pdir, name)))
            except Exception:
                continue
            if d.get("workload") == workload and d.get("streams_per_gpu") == B and d.get("frames_per_step") == T:
                if best is None or d.get("round", 0) >= best[1].get("round", 0):
                    best = (name, d)
    if best is None:
        return None, None
    name, d = best
    if "FETCH_SIZE_KiB" in d and "WRITE_SIZE_KiB" in d:
        t = int(round((FETCH_SIZE_FACTOR * d["FETCH_SIZE_KiB"] + WRITE_SIZE_FACTOR * d["WRITE_SIZE_KiB"]) * 1024))
        return t, (f"profiles/{name}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this configuration, {FETCH_SIZE_FACTOR:g} x FETCH_SIZE + "
                   f"{WRITE_SIZE_FACTOR:g} x WRITE_SIZE (factors calibrated on known byte counts: profiles/r5_hbm_counter_calib.txt)")
    return d.get("hbm_bytes_per_launch"), f"profiles/{name}: counters as reported (no per-counter values kept: uncalibrated)"


def pin_rank(local_rank: int, world: int) -> None:
    """One contiguous slice of the allowed logical cores per rank (its launch thread stops migrating between the other ranks' cores);
    the cores of the GPU's own NUMA node when the driver exposes it.  Best effort: any failure leaves the affinity alone."""
    try:
        allowed = sorted(os.sched_getaffinity(0))
        if len(allowed) < 2 * world or os.environ.get("FE_BENCH_NO_PIN"):
            return
        local = None
        try:      # /sys/class/drm/card*/device/numa_node + /sys/devices/system/node/nodeK/cpulist
            cards = sorted(c for c in os.listdir("/sys/class/drm") if c.startswith("card") and c[4:].isdigit()
                           and os.path.exists(f"/sys/class/drm/{c}/device/numa_node"))
            if local_rank < len(cards):
                node = int(open(f"/sys/class/drm/{cards[local_rank]}/device/numa_node").read())
                if node >= 0:
                    cpus = set()
                    for part in open(f"/sys/devices/system/node/node{node}/cpulist").read().strip().split(","):
                        lo, _, hi = part.partition("-")
                        cpus.update(range(int(lo), int(hi or lo) + 1))
                    local = sorted(cpus & set(allowed))
        except Exception:
            local = None
        per = len(allowed) // world
        mine = allowed[local_rank * per:(local_rank + 1) * per]
        if local and len(local) >= per:      # the slice of the GPU's node that this rank's position among the node's ranks selects
            k = (local_rank * per) % max(1, len(local) - per + 1)
            mine = local[k:k + per]
        if mine:
            os.sched_setaffinity(0, mine)
    except Exception:
        pass


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` (no launcher): start N ranks of this script, one per GPU, under torch.distributed.run
    (the command line the driver itself uses), rendezvous on 127.0.0.1; rank 0 prints the JSON line.  Never falls
    back to fewer ranks: fewer than N devices, or a rank that fails to come up, is a non-zero exit."""
    import socket
    import subprocess
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if "--cpu-dry-run" in sys.argv or (have >= 1 and ("--share-gpu" in sys.argv or os.environ.get("FE_BENCH_SHARE_GPU") == "1")):
        have = n                                      # (no devices involved / the contention probe: every rank on cuda:0)
    if have < n:
        print(f"bench.py: --gpus {n} needs {n} visible MI355X devices, this box has {have}; refusing to measure fewer ranks "
              f"under an n_gpus={n} label", file=sys.stderr, flush=True)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this driver (RCCL needs it)
    # host threads per rank: the container's CPU quota (cgroup cpu.max: 16 CPUs on the r2 / r3 boxes, whatever the host shows) shared by
    # the N ranks - 8 ranks x 4 OpenMP threads on a 16-CPU quota would throttle the launch threads themselves
    avail, quota = host_cpus()
    cap = avail if quota is None else max(1, min(avail, int(quota + 0.5)))
    env.setdefault("OMP_NUM_THREADS", str(max(1, min(4, cap // n))))
    env.setdefault("MKL_NUM_THREADS", env["OMP_NUM_THREADS"])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def dry_run(args, launched: bool, world: int, rank: int):
    """--cpu-dry-run: everything around the kernels, on CPU tensors over gloo - so that the first real N-GPU run is not also the first
    run of this code.  Same steps as main(): process group, rank 0 builds the blob, broadcast, every rank checks the checksums agree,
    R blocks of K (empty) steps each bracketed by barriers with a MAX reduction, per-rank gather, rank 0 prints ONE JSON line."""
    if launched:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    w = WORKLOADS[args.workload]
    kw = model_kwargs(w)
    cfg = FEConfig.from_model_kwargs(**kw)
    eng = Engine(cfg, None)
    from fastenhancer_amd.weights import default_state_dict
    blob = torch.zeros(eng.weight_floats, dtype=torch.float32)
    if rank == 0:
        blob.copy_(eng.make_blob(default_state_dict(cfg, torch.Generator().manual_seed(2))))
    broadcast_blob(blob, src=0)
    chk = torch.stack([blob.double().sum(), blob.double().abs().sum()])
    assert float(chk[1]) > 0.0
    if launched:
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert torch.equal(lo, hi), "weight broadcast: ranks disagree"
    b0, b1 = shard_range(args.streams * world, world, rank)
    times = []
    for _ in range(max(1, min(args.blocks, 3))):
        if launched:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            pass
        own = time.perf_counter() - t0
        tt = torch.tensor([own, -own], dtype=torch.float64)
        if launched:
            dist.barrier()
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)      # (slowest rank, and - negated - the fastest: the spread main() reports)
        times.append((float(tt[0]), -float(tt[1])))
    per_rank = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
    if launched:
        dist.all_gather(per_rank, torch.tensor([float(b1 - b0)], dtype=torch.float64))
    else:
        per_rank = [torch.tensor([float(b1 - b0)])]
    if rank == 0:
        print(json.dumps({"dry_run": True, "metric": "none (launch path only: no kernels ran)", "value": None, "n_gpus": world, "world_size": world,
                          "backend": "gloo", "steps": args.steps, "warmup": args.warmup, "blocks": len(times),
                          # what main() would do with these flags: one HIP graph of the K steps at world > 1 unless --no-graph
                          "launch_mode": "hip_graph" if ((args.graph or world > 1) and not args.no_graph and args.offline_seconds <= 0) else "eager",
                          "eager_ms_per_step": None,
                          "rank_spread_ms_per_step": {"min": min(t[1] for t in times) / max(args.steps, 1) * 1e3, "max": max(t[0] for t in times) / max(args.steps, 1) * 1e3,
                                                      "widest_block_max_over_min": max(t[0] / max(t[1], 1e-12) for t in times)},
                          "streams_per_rank": [int(v) for v in per_rank], "weight_blob_floats": int(blob.numel()),
                          "weight_checksum": float(chk[0])}), flush=True)
    if launched:
        dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default="fe_b", choices=sorted(WORKLOADS))
    ap.add_argument("--streams", type=int, default=256, help="concurrent streams per GPU")
    ap.add_argument("--frames-per-step", type=int, default=1, help="hops per stream per launch (1 = per-hop streaming)")
    ap.add_argument("--offline-seconds", type=float, default=0.0,
                    help="> 0: a step is ONE offline Model.forward (fe_offline) over `--streams` utterances of this many seconds each "
                         "(centered STFT, all frames, overlap-add) instead of one streaming hop per stream")
    ap.add_argument("--offline-engine", default="auto", choices=["auto", "frame_walk", "time_batched"],
                    help="fe_set_offline_engine: the time-batched (layer-by-layer) engine or the per-hop kernel walking the frames")
    ap.add_argument("--blocks", type=int, default=1,
                    help="consecutive timed blocks of --steps steps each; value / ms_per_step are the MEDIAN block (min / max / blocks reported), "
                         "fewer when a block takes long (--block-budget-s).  The default of one block makes --steps the number of timed steps")
    ap.add_argument("--block-budget-s", type=float, default=20.0)
    ap.add_argument("--cpu-dry-run", action="store_true",
                    help="no kernels, no GPU: the launch path alone - bench -> torch.distributed.run -> N ranks (gloo) -> weight-blob broadcast and its "
                         "checksum agreement -> the block loop's barriers / reductions around empty steps -> ONE JSON line with world_size and dry_run: true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the post-run parity check against the oracle (parity_rms_rel: null)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="HOST-CONTENTION PROBE, not a scaling number: all N ranks launch on cuda:0 (gloo for the control traffic; RCCL cannot put two ranks on "
                         "one device) - what N launch threads cost each other under the container's CPU quota (host_enqueue_us_per_step); "
                         "the JSON line carries contention_probe: true and no roofline claim")
    ap.add_argument("--cpu-budget-s", type=float, default=12.0)
    ap.add_argument("--graph", action="store_true",
                    help="capture the K timed steps (K launches, each on its own input hop) into ONE HIP graph and time its replay.  The DEFAULT when "
                         "the world has more than one rank (r6): a 32-us step leaves an eager N-rank number to the launch threads' jitter on a shared CPU "
                         "quota (enqueue 3.7 us per eager launch against 0.3-0.8 us per graph node, profiles/r5_host_contention.txt); the eager figure "
                         "of the same run is reported beside it as eager_ms_per_step")
    ap.add_argument("--no-graph", action="store_true", help="eager launches also at world > 1")
    ap.add_argument("--clock-ramp-ms", type=float, default=250.0,
                    help="untimed launches of the same step BEFORE the counted warm-up, until this much GPU time has passed "
                         "(brings the shader clock and the caches to steady state; reported as clock_ramp_steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed blocks, write what the last timed step returned (rank 0's streams) as DIR/<name>.npy in float32: "
                         "streaming: wav_out [B, T*H] and the caches in the reference's order (cache_00, ...); offline: wav_out and spec_hat.  At most "
                         f"{DUMP_LIMIT_BYTES >> 20} MB in all (larger outputs: the same seeded sample of elements of every array)")
    args = ap.parse_args()

    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ      # started by torch.distributed.run
    if not launched and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1")) if launched else 1
    rank = int(os.environ.get("RANK", "0")) if launched else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if launched else 0
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    share = args.share_gpu or os.environ.get("FE_BENCH_SHARE_GPU") == "1"
    use_graph = (args.graph or (world > 1 and not share)) and not args.no_graph and args.offline_seconds <= 0
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        pin_rank(local_rank, world)
    if args.cpu_dry_run:
        return dry_run(args, launched, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the FastEnhancer HIP path has no CPU fallback")
    if torch.cuda.device_count() <= local_rank and not share:
        raise SystemExit(f"bench.py: rank {rank} has no GPU (local_rank {local_rank}, {torch.cuda.device_count()} visible)")
    dev = torch.device("cuda:0" if share else f"cuda:{local_rank}")
    torch.cuda.set_device(dev)
    use_dist = launched
    cdev = dev                                        # where the control tensors of the collectives live
    if use_dist and share:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        cdev = torch.device("cpu")
    elif use_dist:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    if use_dist:
        assert dist.get_world_size() == world

    w = WORKLOADS[args.workload]
    kw = model_kwargs(w)
    if w.get("lisennet"):
        from fastenhancer_amd.config import LiSenNetConfig
        cfg = LiSenNetConfig.from_model_kwargs(**kw)
    elif w.get("fspen"):
        from fastenhancer_amd.config import FSPENConfig
        cfg = FSPENConfig.from_model_kwargs(**kw)
    elif w.get("bsrnn"):
        from fastenhancer_amd.config import BSRNNConfig
        cfg = BSRNNConfig.from_model_kwargs(**kw)
    elif w.get("kt"):
        from fastenhancer_amd.config import time_kernel_config
        cfg = time_kernel_config(**kw)
    elif w.get("frnn"):
        from fastenhancer_amd.config import dprnn_config
        cfg = dprnn_config(**kw)
    elif w.get("dpt"):
        from fastenhancer_amd.config import dpt_config
        cfg = dpt_config(**kw)
    elif w.get("ln"):
        from fastenhancer_amd.config import ln_config
        cfg = ln_config(**kw)
    elif w.get("nc"):
        from fastenhancer_amd.config import noncausal_config
        cfg = noncausal_config(**kw)
        if args.offline_seconds <= 0:
            args.offline_seconds = 4.0             # the noncausal model has the offline forward only
    else:
        cfg = FEConfig.from_model_kwargs(**kw)
    eng = Engine(cfg, dev)
    if args.offline_engine != "auto":
        eng.set_offline_engine(args.offline_engine)

    # ---- weights: rank 0 builds the seeded checkpoint, folds it, and broadcasts the blob (RCCL)
    blob = torch.empty(eng.weight_floats, dtype=torch.float32, device=dev)
    if rank == 0:
        # no trained checkpoints offline: PyTorch-style random init of the fused weights; the final conv is
        # scaled so that the complex mask is O(1) (the enhanced waveform has the level of the input)
        from fastenhancer_amd.weights import bsrnn_default_state_dict, default_state_dict, fspen_default_state_dict, lisennet_default_state_dict
        if w.get("lisennet"):
            sd = lisennet_default_state_dict(cfg, torch.Generator().manual_seed(2))
        elif w.get("fspen"):
            sd = fspen_default_state_dict(cfg, torch.Generator().manual_seed(2))
        elif w.get("bsrnn"):
            sd = bsrnn_default_state_dict(cfg, torch.Generator().manual_seed(2))
        else:
            sd = default_state_dict(cfg, torch.Generator().manual_seed(2))
            sd["dec_post.2.weight"] = sd["dec_post.2.weight"] * 12.0
        blob.copy_(eng.make_blob(sd))
    torch.cuda.synchronize(dev)
    tb0 = time.perf_counter()
    if share and use_dist:                            # (probe: gloo on a host copy)
        hb = blob.cpu()
        broadcast_blob(hb, src=0)
        blob.copy_(hb)
    else:
        broadcast_blob(blob, src=0)                   # the path's only collective: one ncclBroadcast over xGMI
    torch.cuda.synchronize(dev)
    bcast_ms = (time.perf_counter() - tb0) * 1e3      # (first collective of the communicator: includes RCCL's lazy init)
    rccl_world = dist.get_world_size() if use_dist else 1
    if use_dist:                                      # every rank must now hold rank 0's bytes
        chk = torch.stack([blob.double().sum(), blob.double().abs().sum()]).to(cdev)
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        assert torch.equal(lo, hi), "weight broadcast: ranks disagree"
    eng.load_blob(blob)

    # ---- synthetic streams of this rank, step-major [steps, B, T*H], resident in HBM
    B, T, H = args.streams, args.frames_per_step, cfg.hop_size
    offline = args.offline_seconds > 0
    total_steps = args.warmup + args.steps
    b0, b1 = shard_range(B * world, world, rank)
    lib = eng.lib
    stream = torch.cuda.current_stream(dev)
    sptr = ctypes.c_void_p(stream.cuda_stream)
    if offline:
        # one step = Model.forward over B utterances of offline_seconds each: T frames per utterance
        Tw = int(args.offline_seconds * w["sr"])
        T = 1 + Tw // H
        x = synthetic_streams(b0, b1, Tw, w["sr"], seed=1234 + 2).to(dev).contiguous()   # [B, Tw]
        out = torch.empty(B, H * (T - 1), dtype=torch.float32, device=dev)
        spec_hat = torch.empty(B, cfg.F0 + (1 if (w.get("bsrnn") or w.get("fspen") or w.get("lisennet")) else 0), T, 2, dtype=torch.float32, device=dev)
        work = torch.empty(int(lib.fe_offline_work_floats(eng._h, B, Tw)), dtype=torch.float32, device=dev)
        state = torch.zeros(1, device=dev)
        xp, op_, sp_, wp_ = (ctypes.c_void_p(t_.data_ptr()) for t_ in (x, out, spec_hat, work))

        def run(n, first):
            for _ in range(n):
                rc = lib.fe_offline(eng._h, xp, B, Tw, op_, sp_, wp_, sptr)
                if rc != 0:
                    _lib.check(rc, "fe_offline")
    else:
        pool = min(total_steps, 64)                       # distinct steps of input; reused cyclically
        x = synthetic_streams(b0, b1, pool * T * H, w["sr"], seed=1234 + 2).to(dev)         # [B, pool*T*H]
        x = x.view(B, pool, T * H).permute(1, 0, 2).contiguous()                             # [pool, B, T*H]
        out = torch.empty(B, T * H, dtype=torch.float32, device=dev)
        state = eng.new_state(B)
        xptr, optr, stptr = x.data_ptr(), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(state.data_ptr())
        step_bytes = B * T * H * 4

        def run(n, first):
            for i in range(n):
                s = (first + i) % pool
                rc = lib.fe_step(eng._h, ctypes.c_void_p(xptr + s * step_bytes), T * H, stptr, optr, T * H, B, T, sptr)
                if rc != 0:
                    _lib.check(rc, "fe_step")

    # untimed clock ramp: a 20-step run is otherwise measured on a GPU that is still raising its shader clock and
    # filling its instruction / TLB caches (r1: 39.3 us per step in the driver's 20-step run, 34.5 us in steady state)
    ramp_steps = 0
    cold_ms = None
    if args.clock_ramp_ms > 0 and not use_dist and not use_graph:
        # the figure WITHOUT the ramp, for comparison with r1's numbers and with baselines measured cold: W warm-up steps, then K steps
        # timed on the host clock, before anything else has run on the device (reported as cold_ms_per_step, never as `value`)
        run(args.warmup, 0)
        torch.cuda.synchronize(dev)
        c0 = time.perf_counter()
        run(args.steps, args.warmup)
        torch.cuda.synchronize(dev)
        cold_ms = (time.perf_counter() - c0) / args.steps * 1e3
        if not offline:
            state.zero_()
    if args.clock_ramp_ms > 0:
        r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r0.record(stream)
        chunk = 2 if offline else 50
        while True:
            run(chunk, 0)
            ramp_steps += chunk
            r1.record(stream)
            r1.synchronize()
            if r0.elapsed_time(r1) >= args.clock_ramp_ms or ramp_steps >= 100000:
                break
        state.zero_()
    run(args.warmup, 0)
    torch.cuda.synchronize(dev)
    kernel_name = eng.last_step_kernel()              # fe_last_step_kernel: what the library dispatched for this configuration (the timed launches are the same call)
    graph = None
    graph_note = None
    if use_graph and not offline:
        keep = state.clone()
        try:
            cap = torch.cuda.Stream(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=cap):
                csptr = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                for i in range(args.steps):
                    s_ = (args.warmup + i) % pool
                    rc = lib.fe_step(eng._h, ctypes.c_void_p(xptr + s_ * step_bytes), T * H, stptr, optr, T * H, B, T, csptr)
                    if rc != 0:
                        _lib.check(rc, "fe_step")
        except Exception as exc:                          # (a capture the runtime refuses: measure eagerly and say so)
            if args.graph:
                raise
            graph, graph_note = None, f"graph capture failed, eager launches timed: {type(exc).__name__}: {exc}"[:300]
        state.copy_(keep)
        torch.cuda.synchronize(dev)
    if use_dist:                                      # every rank must time the same way
        gflag = torch.tensor([1 if graph is not None else 0], dtype=torch.int64, device=cdev)
        dist.all_reduce(gflag, op=dist.ReduceOp.MIN)
        if int(gflag[0]) == 0 and graph is not None:
            graph, graph_note = None, "another rank could not capture its graph: eager launches timed on every rank"

    # ---- timed region: R consecutive blocks of EXACTLY K steps, each bracketed by barrier + synchronize on both sides and
    # reduced with MAX over the ranks; the MEDIAN block is reported (a single 20-step block is a 0.7 ms sample)
    def timed_block(first, eager=False):
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record(stream)
        if graph is not None and not eager:
            graph.replay()
        else:
            run(args.steps, first)
        enq = time.perf_counter() - t0                # the launch thread's own time: K launches enqueued (not complete)
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        dt_ = time.perf_counter() - t0                # this rank's K steps, device-complete
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)
        km = ev0.elapsed_time(ev1) / args.steps       # HIP events on the launch stream: avg per launch
        own = dt_
        lo_ = dt_
        if use_dist:
            tt = torch.tensor([dt_, km, enq, -dt_], dtype=torch.float64, device=cdev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt_, km, enq, lo_ = float(tt[0]), float(tt[1]), float(tt[2]), -float(tt[3])
        return dt_, km, own, enq, lo_                 # (lo_: the fastest rank's time for the block - the spread over the ranks)

    # the eager figure of the same run beside a graph-timed value: one block of K plain launches (state restored afterwards)
    eager_ms = None
    if graph is not None:
        keep = state.clone()
        timed_block(args.warmup, eager=True)
        eb = timed_block(args.warmup, eager=True)
        eager_ms = eb[0] / args.steps * 1e3
        state.copy_(keep)
        torch.cuda.synchronize(dev)

    blocks = [timed_block(args.warmup)]
    n_blocks = max(1, args.blocks)
    if blocks[0][0] > 0:
        n_blocks = max(1, min(n_blocks, int(args.block_budget_s / blocks[0][0])))
    if use_dist:                                      # every rank must run the same number of blocks
        nb = torch.tensor([n_blocks], dtype=torch.int64, device=cdev)
        dist.all_reduce(nb, op=dist.ReduceOp.MIN)
        n_blocks = int(nb[0])
    for r_ in range(1, n_blocks):
        blocks.append(timed_block(args.warmup + r_ * args.steps))
    order = sorted(range(len(blocks)), key=lambda i_: blocks[i_][0])
    med = order[(len(order) - 1) // 2]                # lower median: an actually measured block
    dt, kernel_ms = blocks[med][0], blocks[med][1]
    if use_dist:
        mine = torch.tensor([blocks[med][2] / args.steps * 1e3], dtype=torch.float64, device=cdev)
        per_rank = [torch.zeros(1, dtype=torch.float64, device=cdev) for _ in range(world)]
        dist.all_gather(per_rank, mine)
        per_rank_ms = [float(v) for v in per_rank]
    else:
        per_rank_ms = [dt / args.steps * 1e3]
    assert torch.isfinite(out).all()

    # ---- what the last timed step returned, written before the parity launch below overwrites it
    dumped = None
    if args.dump_outputs and rank == 0:
        if offline:
            arrs = {"wav_out": out, "spec_hat": spec_hat}
        else:
            arrs = {"wav_out": out}
            arrs.update({f"cache_{i:02d}": c for i, c in enumerate(eng.split_state(state, B))})
        dumped = dump_outputs({k: v.cpu().numpy() for k, v in arrs.items()}, args.dump_outputs)

    # ---- parity of exactly what was timed, outside the timed blocks: one more launch from the state the run left, against the oracle
    parity = None
    if rank == 0 and not offline and T == 1 and not args.no_parity:
        nxt = (args.warmup + len(blocks) * args.steps) % pool
        snap = state.clone()
        run(1, nxt)
        torch.cuda.synchronize(dev)
        parity = parity_after_timed_region(args.workload, w, kw, sd, eng, B, x[nxt].cpu().numpy(), [c.cpu().numpy() for c in eng.split_state(snap, B)],
                                           out.cpu().numpy(), [c.cpu().numpy() for c in eng.split_state(state, B)])

    if rank == 0:
        frames = B * world * T * args.steps
        flops_per_launch = eng.flops_per_frame * B * T
        achieved = flops_per_launch / (kernel_ms * 1e-3) / 1e12
        # algorithmic HBM bytes of a launch: the hop in and out, the state read and written back (dptransformer: its K / V caches
        # are rings - all read, one slot of 31 written per frame)
        state_bytes = 4 * eng.state_floats(B)
        alg_bytes = B * T * (2 * H * 4) + 2 * state_bytes
        if offline:          # the utterances in and out, spec_hat out (the state is born and dies inside the call)
            alg_bytes = B * (Tw * 4 + H * (T - 1) * 4) + spec_hat.numel() * 4
        if w.get("dpt"):
            cache_bytes = 4 * B * 2 * w["K"] * w["F2"] * w["C2"] * w["dpt"]
            alg_bytes = B * T * (2 * H * 4) + state_bytes + (state_bytes - cache_bytes) + T * cache_bytes // w["dpt"]
        res = {
            "metric": "audio frames/sec (hop=256, 16kHz) FastEnhancer_B" if args.workload == "fe_b" else f"audio frames/sec {w['desc']}",
            "value": frames / dt, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "clock_ramp_steps": ramp_steps, "cold_ms_per_step": cold_ms, "rccl_world_size": rccl_world, "weight_broadcast_ms": bcast_ms,
            "collective_backend": (dist.get_backend() if use_dist else "none (no launcher: no process group)"),
            "per_rank_ms_per_step": per_rank_ms,
            # host side of a step on the slowest rank: wall time per step minus the HIP-event time of its launches - tells a launch-jitter-bound
            # N-GPU number from a kernel-bound one
            "host_launch_overhead_ms_per_step": dt / args.steps * 1e3 - kernel_ms, "kernel_ms_hip_events": kernel_ms,
            # the launch thread alone: wall time for K fe_step calls to RETURN (enqueued, not complete), slowest rank of the median block
            "host_enqueue_us_per_step": blocks[med][3] / args.steps * 1e6,
            # parity of what was timed (outside the timed blocks): one more launch of the same configuration from the state the run left vs the
            # oracle stepping all B streams from that state - relative rms error of the enhanced hop / the worst returned cache
            "parity_rms_rel": None if parity is None else parity[0], "parity_cache_rms_rel": None if parity is None else parity[1],
            "parity_checker": None if parity is None else f"{parity[2]}, all {B} streams of rank 0, after the timed region",
            "blocks": len(blocks), "statistic": "median of `blocks` consecutive blocks of `steps` steps (max over ranks per block)",
            # how the K timed steps were issued: one HIP graph of K fe_step launches (the default at world > 1) or K eager launches; with a graph the
            # eager time of one block of the same run is reported beside it
            "launch_mode": "hip_graph" if graph is not None else "eager", "graph_note": graph_note, "eager_ms_per_step": eager_ms,
            # spread over the ranks (fastest / slowest rank's wall time per step): of the median block, and the widest of any block
            "rank_spread_ms_per_step": {"min": blocks[med][4] / args.steps * 1e3, "max": blocks[med][0] / args.steps * 1e3,
                                        "widest_block_max_over_min": max(b_[0] / max(b_[4], 1e-12) for b_ in blocks)},
            "min_ms_per_step": min(b_[0] for b_ in blocks) / args.steps * 1e3, "max_ms_per_step": max(b_[0] for b_ in blocks) / args.steps * 1e3,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "timed_steps": len(blocks) * args.steps, "dump_outputs": dumped,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": (f"{w['desc']} (N={w['N']}, H={w['H']}), offline Model.forward (centered STFT, all frames, overlap-add) over {B} utterances of "
                                    f"{args.offline_seconds:g} s per GPU and step = {T} frames each, engine {args.offline_engine}") if offline else
                                   (f"{w['desc']} (N={w['N']}, H={w['H']}), {B} concurrent streams per GPU, "
                                    f"{T} hop(s) per stream per step, wav->wav streaming step with STFT/iSTFT and GRU caches"),
                       "streams_per_gpu": B, "frames_per_step": T, "parallelism": f"streams sharded dp{world}, RCCL weight broadcast",
                       "weights": "seeded random checkpoint (no trained weights offline), BN/weight-norm folded"},
            "rtf_per_stream": dt * w["sr"] / (args.steps * (Tw if offline else T * H) * B * world),   # amortised: wall time / audio time / streams
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_FP32_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_FP32_TFLOPS, "traffic": None if offline else measured_traffic(args.workload, B, T)[0],
                         "algorithmic_flops_per_launch": flops_per_launch,
                         "algorithmic_hbm_bytes_per_launch": alg_bytes,
                         # fe_last_step_kernel: the kernels the library dispatched for this call, in launch order (kernel_ms: all of them)
                         "kernel": kernel_name, "kernel_ms": kernel_ms,
                         "flops_per_frame": eng.flops_per_frame,
                         "hbm_frac": alg_bytes / (kernel_ms * 1e-3) / 8e12},
        }
        # the dominant bound: a workload whose algorithmic HBM traffic uses a larger fraction of the HBM peak than its FLOPs do of
        # the fp32 matrix peak (the dptransformer variant: K / V caches of 31 frames read every hop) is priced against HBM
        rf = res["roofline"]
        # where `traffic` comes from: a PMC pass (FETCH_SIZE / WRITE_SIZE, rocprofv3 --pmc) of exactly this configuration committed under
        # profiles/pmc_*.json - a constant read back, not a measurement of this run; null when no such pass exists
        rf["traffic_source"] = None if offline else measured_traffic(args.workload, B, T)[1]
        if rf["hbm_frac"] > rf["frac"]:
            rf.update({"bound": "hbm", "achieved": alg_bytes / (kernel_ms * 1e-3) / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": rf["hbm_frac"],
                       "mfma_frac": achieved / PEAK_FP32_TFLOPS})
        if world == 1 and not args.no_cpu_baseline and (w.get("fspen") or w.get("lisennet")):
            res["cpu_baseline"] = cpu_baseline_fspen(kw, w["sr"], B, args.cpu_budget_s, lisennet=bool(w.get("lisennet")))
        elif world == 1 and not args.no_cpu_baseline and w.get("bsrnn"):
            res["cpu_baseline"] = cpu_baseline_bsrnn(args.workload, kw, w["sr"], B, args.cpu_budget_s)
        elif world == 1 and not args.no_cpu_baseline and (w.get("kt") or w.get("frnn") or w.get("dpt") or w.get("ln")):
            res["cpu_baseline"] = cpu_baseline_variant(kw, w["sr"], B, min(args.cpu_budget_s, 10.0), "ln" if w.get("ln") else None)
        elif world == 1 and not args.no_cpu_baseline and w.get("nc"):
            res["cpu_baseline"] = cpu_baseline_offline_numpy(kw, w["sr"], min(args.cpu_budget_s, 15.0))
        elif world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(args.workload, kw, w["sr"], B, args.cpu_budget_s)
        if share:
            res.update({"contention_probe": True, "metric": f"HOST-CONTENTION PROBE (NOT a scaling number): {world} ranks launching on ONE GPU",
                        "n_gpus_really_used": 1, "backend": "gloo"})
            res["roofline"] = None
        print(json.dumps(res), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
