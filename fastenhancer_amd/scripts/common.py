"""Shared host logic of the command-line callers: config / checkpoint lookup as the reference does it
(`logs/<name>/config.yaml`, latest `[0-9]{5,}.pth`: utils/hparams.py:88-150, wrappers/ns.py:288-314) and WAV I/O
(scipy; librosa / soundfile are not required — the sampling rate must already match, unless the caller asks for the GPU resampler
with --resample)."""
from __future__ import annotations

import argparse
import contextlib
import importlib
import os
import re
import sys
from typing import Optional, Tuple

import numpy as np
import torch
import yaml
from scipy.io import wavfile


def load_hparams(config: Optional[str] = None, name: Optional[str] = None, log_root: str = "logs") -> dict:
    """-c <yaml> or -n <name> (-> logs/<name>/config.yaml), plain dict (only model / model_kwargs /
    data.sampling_rate are used)."""
    if config is None:
        if name is None:
            raise ValueError("Either --name or --config should be given.")
        config = os.path.join(log_root, name, "config.yaml")
    with open(config) as f:
        return yaml.safe_load(f)


def latest_checkpoint(base_dir: str) -> Optional[str]:
    """wrappers/ns.py:288-300: newest file matching [0-9]{5,}.pth in logs/<name>."""
    if not os.path.isdir(base_dir):
        return None
    files = [int(f[:-4]) for f in os.listdir(base_dir) if re.fullmatch(r"[0-9]{5,}\.pth", f)]
    if not files:
        return None
    return os.path.join(base_dir, f"{max(files):0>5d}.pth")


def build_model(hps: dict, device: str, offline: bool, checkpoint: Optional[str] = None):
    """importlib.import_module(f"models.{hps.model}.model") of wrappers/ns.py:29-32, on the HIP path."""
    module = importlib.import_module(f"fastenhancer_amd.models.{hps['model']}.model")
    cls = module.Model if offline else module.ONNXModel
    model = cls(**hps["model_kwargs"]).to(device).eval()
    if checkpoint is not None:
        ckpt = torch.load(checkpoint, map_location="cpu", weights_only=False)
        model.load_state_dict(ckpt["model"] if "model" in ckpt else ckpt, strict=True)
        model.remove_weight_reparameterizations()
    return model


# The callers that carry --resample run the hop-by-hop and the offline caller themselves (stream_chunks -> test_streaming, enhance_dir ->
# test_offline), whose read_wav(path, sr) calls name no resampling: the flag reaches them through this switch, set for the length of the call.
_RESAMPLING_ON: Optional[str] = None       # the device to resample on, or None: off


@contextlib.contextmanager
def resampling(device: Optional[str]):
    """inside the block read_wav(path, sr) resamples a file at another rate on `device` (None: the block changes nothing)"""
    global _RESAMPLING_ON
    before = _RESAMPLING_ON
    _RESAMPLING_ON = before if device is None else device
    try:
        yield
    finally:
        _RESAMPLING_ON = before


def split_resample_flag(argv):
    """(device to resample on or None, the other arguments) of a caller's argument list.  Only --resample is taken out; --device (which
    every caller has, default cuda:0) is looked at and left where it is.  With -h the flag's own help is printed before the caller's."""
    argv = sys.argv[1:] if argv is None else list(argv)
    p = argparse.ArgumentParser(add_help=False, usage=argparse.SUPPRESS)
    p.add_argument("--resample", action="store_true", help=RESAMPLE_HELP)
    own, rest = p.parse_known_args(argv)
    q = argparse.ArgumentParser(add_help=False)
    q.add_argument("--device", type=str, default="cuda:0")
    device = q.parse_known_args(rest)[0].device
    if "-h" in rest or "--help" in rest:
        p.print_help()
    return (device if own.resample else None), rest


def read_wav(path: str, sr: int, resample: Optional[bool] = None, device: Optional[str] = None) -> np.ndarray:
    """mono float32 in [-1, 1] at the rate sr.  A file at another rate raises (no resampler here) unless resample=True or the call is made
    inside resampling(device) (the callers' --resample): the file is then read at its own rate and resampled to sr on the GPU
    (fastenhancer_amd.resample.Resampler: the polyphase filter of scipy.signal.resample_poly, the `polyphase` type of the reference's
    scripts/resample.py - not librosa's default soxr_hq)."""
    if resample is None:
        resample, device = _RESAMPLING_ON is not None, _RESAMPLING_ON
    device = "cuda:0" if device is None else device
    rate, data = wavfile.read(path)
    if rate != sr and not resample:
        raise ValueError(f"{path}: sampling rate {rate} != model sampling rate {sr} (resample the file first)")
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)      # librosa.load(mono=True)
    if rate != sr:
        from ..resample import Resampler
        x = Resampler(int(rate), int(sr), device)(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).cpu().numpy()
    return x


RESAMPLE_HELP = ("read a file at another sampling rate at its own rate and resample it to the model's on the GPU (polyphase, as "
                 "scipy.signal.resample_poly); the output is written at the model's rate.  Off by default: such a file is refused")


def write_wav(path: str, sr: int, x: np.ndarray):
    wavfile.write(path, sr, np.asarray(x, dtype=np.float32))
