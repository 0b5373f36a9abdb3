#!/usr/bin/env python3
"""Digests of the packed weight buffers of every shipped configuration, computed on the CPU (Engine.pack_blob: no GPU).

One line per configuration: name, packed floats, sha256 of the packed bytes, packing time.  Two builds pack the same
bytes exactly when their columns agree - run it on both (FASTENHANCER_HIP_LIB selects a side build):

    python tools/packed_digests.py                       # the 25 FastEnhancer models, the four BSRNN sizes, FSPEN, LiSenNet
    python tools/packed_digests.py --only fe_b --over activation=LeakyReLU mask=sigmoid      # an --add-shape option set
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from common import BSRNN_KWARGS, FSPEN_KWARGS, LISENNET_KWARGS, MODEL_KWARGS, MODEL_MODULE  # noqa: E402
from fastenhancer_amd import config as C  # noqa: E402
from fastenhancer_amd import weights as W  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402

_VARIANT = {"fastenhancer.dprnn": C.dprnn_config, "fastenhancer.dptransformer": C.dpt_config, "fastenhancer.ln": C.ln_config,
            "fastenhancer.noncausal": C.noncausal_config, "fastenhancer.time_kernel": C.time_kernel_config}


def configurations(only=None, over=None):
    """name -> (config, its family's default_state_dict): the 31 shipped configurations, or those named in `only`; `over` updates the
    FastEnhancer model_kwargs"""
    out = {}
    for name, (kw, _, _) in MODEL_KWARGS.items():
        if only and name not in only:
            continue
        kw = dict(kw, **(over or {}))
        out[name] = (_VARIANT.get(MODEL_MODULE[name], C.FEConfig.from_model_kwargs)(**kw), W.default_state_dict)
    for name, (kw, _, _) in BSRNN_KWARGS.items():
        out[name] = (C.BSRNNConfig.from_model_kwargs(**kw), W.bsrnn_default_state_dict)
    out["fspen"] = (C.FSPENConfig.from_model_kwargs(**FSPEN_KWARGS[0]), W.fspen_default_state_dict)
    out["lisennet"] = (C.LiSenNetConfig.from_model_kwargs(**LISENNET_KWARGS[0]), W.lisennet_default_state_dict)
    return {name: v for name, v in out.items() if not only or name in only}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--only", nargs="*", help="configuration names (default: all)")
    ap.add_argument("--over", nargs="*", default=[], metavar="KEY=VALUE", help="model_kwargs overrides of the FastEnhancer configurations (values: JSON or a bare string)")
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    over = {}
    for kv in a.over:
        k, _, v = kv.partition("=")
        try:
            over[k] = json.loads(v)
        except ValueError:
            over[k] = v
    total = 0.0
    for name, (cfg, default_sd) in configurations(a.only, over).items():
        eng = Engine(cfg, None)
        blob = eng.make_blob(default_sd(cfg, torch.Generator().manual_seed(a.seed)))
        t0 = time.perf_counter()
        packed = eng.pack_blob(blob)
        dt = time.perf_counter() - t0
        total += dt
        print(f"{name:<12} {packed.numel():>9} {hashlib.sha256(packed.numpy().tobytes()).hexdigest()} {dt * 1e3:8.1f} ms", flush=True)
    print(f"{'total':<12} {'':>9} {'':<64} {total * 1e3:8.1f} ms")


if __name__ == "__main__":
    main()
