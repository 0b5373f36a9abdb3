"""G.711 mu-law and A-law on torch tensors: what a caller uses to make or inspect the one-byte-per-sample packets the resampler takes and
returns (FE_AUDIO_ULAW / FE_AUDIO_ALAW; `in_format=` / `out_format=` of resample.Resampler, `client_format=` of the resampled packet pools).
Not on the hot path: the resampler's kernels decode and encode by themselves.

The formulas are the contract's (include/fastenhancer_hip.h, "Audio at another sample rate") - the ITU-T G.711 tables as CPython's audioop
computes them - in 32-bit integer tensor operations, on any device."""
from __future__ import annotations

import torch
from torch import Tensor

LAWS = ("ulaw", "alaw")


def check_law(law) -> str:
    if law not in LAWS:
        raise ValueError(f"law must be 'ulaw' or 'alaw', got {law!r}")
    return law


def _hibit(v: Tensor) -> Tensor:
    """index of the highest set bit of positive int32 values below 2^15"""
    h = torch.zeros_like(v)
    for k in range(1, 15):
        h = h + (v >= (1 << k)).to(v.dtype)
    return h


def decode(bytes_u8: Tensor, law: str) -> Tensor:
    """uint8 G.711 bytes -> the int16 linear samples they stand for (same shape, same device)"""
    check_law(law)
    if not isinstance(bytes_u8, Tensor) or bytes_u8.dtype != torch.uint8:
        raise ValueError(f"G.711 {law} bytes are a uint8 tensor, got {getattr(bytes_u8, 'dtype', type(bytes_u8))}")
    b = bytes_u8.to(torch.int32)
    if law == "ulaw":
        u = ~b & 0xFF
        e, m = (u >> 4) & 7, u & 15
        mag = (((m << 3) + 0x84) << e) - 0x84
        s = torch.where((u & 0x80) != 0, -mag, mag)
    else:
        a = b ^ 0x55
        e, m = (a >> 4) & 7, a & 15
        mag = torch.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << (e - 1).clamp(min=0))
        s = torch.where((a & 0x80) != 0, mag, -mag)
    return s.to(torch.int16)


def encode(pcm_i16: Tensor, law: str) -> Tensor:
    """int16 linear samples -> uint8 G.711 bytes (same shape, same device)"""
    check_law(law)
    if not isinstance(pcm_i16, Tensor) or pcm_i16.dtype != torch.int16:
        raise ValueError(f"G.711 {law} is encoded from an int16 tensor, got {getattr(pcm_i16, 'dtype', type(pcm_i16))}")
    q = pcm_i16.to(torch.int32)
    if law == "ulaw":
        v = q >> 2
        neg = v < 0
        v = torch.where(neg, -v, v).clamp(max=8159) + 33
        seg = _hibit(v) - 5
        t = torch.where(seg >= 8, torch.full_like(v, 0x7F), (seg << 4) | ((v >> (seg + 1)) & 15))
        b = t ^ torch.where(neg, 0x7F, 0xFF)
    else:
        pos = q >= 0
        n = torch.where(pos, q, ~q)
        e = torch.where(n < 256, torch.zeros_like(n), _hibit(n) - 7)
        m = torch.where(n < 256, n >> 4, (n >> (e + 3)) & 15)
        b = (torch.where(pos, 0x80, 0) | (e << 4) | m) ^ 0x55
    return b.to(torch.uint8)
