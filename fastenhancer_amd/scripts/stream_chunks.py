#!/usr/bin/env python3
"""scripts/test_streaming.py with one more flag: --chunk-hops N runs the file in chunks of N hops on the time pipeline
(Engine.step_chunk - BSRNN and FSPEN checkpoints: Engine.step_backlog - through streaming.enhance_stream(chunk_hops=N)) instead of hop by hop.
A LiSenNet checkpoint walks its chunks unless --time-pipeline P (P >= 2: Engine.set_time_pipeline) opts it in to the pipeline.  Off by default: without the flag this IS
test_streaming.py (same flags, same loop, same output).
And a second one: --resample takes a file that is not at the model's rate (with or without --chunk-hops; test_streaming.py itself refuses
such a file): it is read at its own rate, resampled on the GPU and written at the model's rate.  Off by default.

    python -m fastenhancer_amd.scripts.stream_chunks -c configs/fastenhancer/b.yaml --checkpoint logs/b/00500.pth \\
        --audio-path noisy.wav --save-output --chunk-hops 256
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from ..streaming import enhance_stream
from . import test_streaming
from .common import build_model, latest_checkpoint, load_hparams, read_wav, resampling, split_resample_flag, write_wav


def main(argv=None):
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--chunk-hops", type=int, default=None, help="hops per call on the time pipeline (default: off - hop by hop)")
    p.add_argument("--time-pipeline", type=int, default=None, help="with --chunk-hops: frames in flight per stream (Engine.set_time_pipeline; "
                   "default: the model family's own; a LiSenNet model takes the pipeline only with a value of 2 or more)")
    own, rest = p.parse_known_args(argv)
    resample_on, rest = split_resample_flag(rest)
    if own.chunk_hops is None:
        with resampling(resample_on):
            return test_streaming.main(rest)
    q = argparse.ArgumentParser()
    q.add_argument("-n", "--name", type=str)
    q.add_argument("-c", "--config", type=str)
    q.add_argument("--checkpoint", type=str)
    q.add_argument("--audio-path", type=str, required=True)
    q.add_argument("--save-output", action="store_true")
    q.add_argument("--output-path", type=str, default="enhanced_streaming.wav")
    q.add_argument("--n-fft", type=int, default=None)
    q.add_argument("--hop-size", type=int, default=None)
    q.add_argument("--sr", type=int, default=None)
    q.add_argument("--device", type=str, default="cuda:0")
    args = q.parse_args(rest)

    hps = load_hparams(args.config, args.name)
    kw = hps["model_kwargs"]
    sr = hps["data"]["sampling_rate"]
    for flag, want in (("n_fft", kw["n_fft"]), ("hop_size", kw["hop_size"]), ("sr", sr)):
        got = getattr(args, flag)
        assert got is None or got == want, f"--{flag.replace('_', '-')}={got} does not match the config ({want})"
    ckpt = args.checkpoint or (latest_checkpoint(os.path.join("logs", args.name)) if args.name else None)
    model = build_model(hps, args.device, offline=False, checkpoint=ckpt)
    if own.time_pipeline is not None:
        model.engine.set_time_pipeline(own.time_pipeline)
    wav = torch.from_numpy(np.clip(read_wav(args.audio_path, sr, resample_on is not None, resample_on).reshape(1, -1), -1, 1)).to(args.device)
    print("Inferencing...")
    torch.cuda.synchronize()
    tic = time.perf_counter()
    y = enhance_stream(model, wav, chunk_hops=own.chunk_hops)       # (pads, drops the latency and clips as the hop loop does)
    torch.cuda.synchronize()
    toc = time.perf_counter()
    print(f">>> RTF: {(toc - tic) * sr / wav.shape[-1]}")
    if args.save_output:
        write_wav(args.output_path, sr, y[0].cpu().numpy())
        print(f"saved {args.output_path}")


if __name__ == "__main__":
    main()
