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
from fastenhancer_amd.config import MODEL_CONFIGS  # noqa: E402
from fastenhancer_amd.engine import Engine  # noqa: E402
from fastenhancer_amd.family import family_of  # noqa: E402


def configurations(only=None, over=None):
    """name -> (config, its family's default_state_dict): the 31 shipped configurations, or those named in `only`; `over` updates the
    FastEnhancer model_kwargs.  (tests/test_cpu_pack.py imports this module, and earlier revisions of the tests are run against later
    trees: of tests/common.py only the kwargs tables, which every revision has, are used here.)"""
    out = {}
    for name, (kw, _, _) in {**MODEL_KWARGS, **BSRNN_KWARGS, "fspen": FSPEN_KWARGS, "lisennet": LISENNET_KWARGS}.items():
        if not only or name in only:
            module = MODEL_MODULE.get(name, "bsrnn" if name in BSRNN_KWARGS else name)
            cfg = MODEL_CONFIGS[module](**dict(kw, **(over or {}) if name in MODEL_KWARGS else {}))
            out[name] = (cfg, family_of(cfg).default_state_dict)
    return out


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
