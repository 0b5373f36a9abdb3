"""The polyphase resampler's contract in numpy float64 (include/fastenhancer_hip.h, "Audio at another sample rate"): the taps, the direct
form of one output, the output counts and the error bound.  No scipy, no library: the GPU tests compare the kernels against this, and the
CPU tests compare this against scipy.signal.resample_poly."""
from math import gcd

import numpy as np

# the seven pairs the contract was checked on (Hz)
PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (16000, 48000), (16000, 8000), (16000, 44100), (24000, 16000)]


def ratio(sr_in, sr_out):
    g = gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g          # up, down


def half_len(up, down):
    return 10 * max(up, down)


def taps_per_output(up, down):
    return -(-(2 * half_len(up, down) + 1) // up)


def taps(up, down):
    """h = up * firwin(L, 1 / R, window=("kaiser", 5.0)), spelled out"""
    R, hl = max(up, down), half_len(up, down)
    m = np.arange(2 * hl + 1, dtype=np.float64) - hl
    h0 = np.sinc(m / R) / R * np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (m / hl) ** 2))) / np.i0(5.0)
    return up * h0 / h0.sum()


def out_count(n, up, down):
    return -(-n * up // down)


def emitted(n, up, down):
    """M(N): outputs of a stream that has consumed n samples"""
    return max(0, -(-(n * up - half_len(up, down)) // down))


def emitted_brute(n, up, down, limit=100000):
    """... by counting the outputs whose newest input x[kmax] has arrived"""
    hl, m = half_len(up, down), 0
    while m < limit and (m * down + hl) // up <= n - 1:
        m += 1
    return m


def resample(x, up, down, h=None, n_out=None):
    """y[m] = sum_j h[r + j up] x[kmax - j] in float64; x [..., N] -> [..., n_out] (default: the whole-signal count)"""
    x = np.asarray(x, dtype=np.float64)
    h = taps(up, down) if h is None else np.asarray(h, dtype=np.float64)
    hl, K, N = half_len(up, down), taps_per_output(up, down), x.shape[-1]
    n_out = out_count(N, up, down) if n_out is None else n_out
    xp = np.concatenate([np.zeros(x.shape[:-1] + (K,)), x, np.zeros(x.shape[:-1] + (K + hl // up + 2,))], axis=-1)      # x = 0 outside [0, N)
    y = np.zeros(x.shape[:-1] + (n_out,))
    c = np.arange(n_out, dtype=np.int64) * down + hl
    kmax, r = c // up, c % up
    for j in range(K):
        t = r + j * up
        ok = t <= 2 * hl
        idx = np.clip(kmax - j + K, 0, xp.shape[-1] - 1)
        y += np.where(ok, h[np.minimum(t, 2 * hl)], 0.0) * xp[..., idx] * ((kmax - j + K >= 0) & (kmax - j + K < xp.shape[-1]))
    return y


def error_bound(up, down, peak, h=None):
    """|fp32 kernel - float64 oracle| <= (K + 2) 2^-24 S peak, S = max_r sum_j |h[r + j up]|: a K-term fp32 dot product plus one rounding of
    each tap"""
    h = taps(up, down) if h is None else h
    K = taps_per_output(up, down)
    S = max(np.abs(h[r::up]).sum() for r in range(up))
    return (K + 2) * 2.0 ** -24 * S * peak


def pcm16(y):
    """clamp(rint(y * 32768), -32768, 32767), ties to even, NaN -> 0, on float32 values"""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = np.clip(np.rint(y * np.float32(32768.0)), -32768.0, 32767.0)
    return np.where(np.isnan(y), 0, v).astype(np.int16)
