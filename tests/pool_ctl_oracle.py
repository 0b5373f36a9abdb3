"""The suppression limit of fe_step_pool_streams_ctl on the oracle side (include/fastenhancer_hip.h): the streaming step of the BSRNN, FSPEN and
LiSenNet oracles with the floor, in float64, between what the model produced in the compressed domain and the un-compress.  Composed from the
oracles' public methods (stft_step, model_forward, LiSenNet's features, istft_step), so with every gain 0 it is oracle.step itself.  No library:
the GPU tests compare the kernels against this, and the CPU tests check this against oracle.step and against the contract."""
import functools

import numpy as np

from common import build_named_oracle, rms

FLT_MIN = float(np.finfo(np.float32).tiny)
GAINS = [0.0, 0.2, 0.25]           # the three streams of the parity case: one without a limit, two with (issue: what each family's seeded masks answer to)
HOPS = 6
MODELS = ["bsrnn_xxt", "bsrnn_s", "fspen", "lisennet"]


def clamp_gain(g):
    """the kernel's reading of a table entry: clamped to [0, 1]; NaN is 0 (off)"""
    g = np.asarray(g, np.float64)
    return np.where(np.isnan(g), 0.0, np.clip(g, 0.0, 1.0))


def compressed(orc, spec_in):
    """X_c: the compressed input spectrum the model sees (the first lines of every oracle's spec_forward)"""
    dt = orc.dtype
    x = spec_in.astype(dt)
    mag = np.maximum(np.sqrt(x[..., 0:1] ** 2 + x[..., 1:2] ** 2), dt(1e-5))
    return x * mag ** dt(orc.cfg.input_compression - 1.0)


def produced(orc, x, cache_model):
    """Y_c: the bins the model produced in the compressed domain, as they stand before the un-compress, and the model's new caches.
    BSRNN, FSPEN: model_forward.  LiSenNet: features -> model_forward -> complex multiply."""
    if not hasattr(orc, "features"):
        return orc.model_forward(x, list(cache_model))
    feat, pha_last = orc.features(x, cache_model[0], True)
    mask, cache_out = orc.model_forward(feat, list(cache_model[1:]))
    y = np.stack([x[..., 0] * mask[..., 0] - x[..., 1] * mask[..., 1], x[..., 0] * mask[..., 1] + x[..., 1] * mask[..., 0]], axis=3)
    return y.astype(orc.dtype), [pha_last] + cache_out


def floor(x, y, gains, compression):
    """Y_c' = Y_c max(1, m |X_c| / |Y_c|), m = g^c, and m X_c where |Y_c|^2 < FLT_MIN; in float64.  x, y [B, F, T, 2]; gains [B] (clamped
    here).  A stream whose gain is off keeps y as it is.  Returns y' (float64) and the lifted bins [B, F, T] (bool)."""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    m = (clamp_gain(gains) ** float(compression)).reshape(-1, 1, 1)
    on = m > 0.0
    xa = np.sqrt(x64[..., 0] ** 2 + x64[..., 1] ** 2)
    y2 = y64[..., 0] ** 2 + y64[..., 1] ** 2
    tiny = y2 < FLT_MIN
    scale = np.maximum(1.0, m * xa / np.sqrt(np.where(tiny, 1.0, y2)))
    lifted = on & np.where(tiny, m * xa > 0.0, scale > 1.0)
    out = np.where((on & tiny)[..., None], m[..., None] * x64, y64 * np.where(on & ~tiny, scale, 1.0)[..., None])
    return out, lifted


def step(orc, wav_in, cache_stft, cache_istft, *cache_model, gains):
    """oracle.step with the floor; gains [B].  Returns (the step's outputs, the share of bins lifted per stream [B], X_c, Y_c, Y_c')."""
    dt, c = orc.dtype, orc.cfg
    spec_in, cache_stft = orc.stft_step(wav_in, cache_stft)
    x = compressed(orc, spec_in)
    y, cache_out = produced(orc, x, list(cache_model))
    if np.any(clamp_gain(gains) > 0.0):
        y_lim, lifted = floor(x, y, gains, c.input_compression)
        y_lim = y_lim.astype(dt)
    else:
        y_lim, lifted = y, np.zeros(y.shape[:3], bool)
    mag2 = np.sqrt(y_lim[..., 0:1] ** 2 + y_lim[..., 1:2] ** 2)
    spec_out = (y_lim * mag2 ** dt(1.0 / c.input_compression - 1.0)).astype(dt)
    wav_out, cache_istft = orc.istft_step(spec_out, cache_istft)
    return (wav_out, cache_stft, cache_istft, *cache_out), lifted.mean(axis=(1, 2)), x, y, y_lim


@functools.lru_cache(maxsize=None)
def reference(name):
    """Six hops of three streams (GAINS) from zero state on 0.1 randn seeded 77: the input; the composed step's output and overlap tail; the
    plain oracle.step's output; per hop the lifted shares [HOPS, B] and (X_c, Y_c, Y_c').  Computed once per model and shared.  The oracle
    runs in its float32, as in every streaming parity test (the floor itself is float64): LiSenNet's phase features are discontinuous where
    a phase difference wraps at +-pi, and on this input its float64 oracle is 1e-1 (relative rms) away from its own float32 run - no yardstick
    for float32 kernels."""
    cfg, sd, fused, orc = build_named_oracle(name)
    import torch
    H, B = cfg.hop_size, len(GAINS)
    x = (0.1 * torch.randn(B, HOPS * H, generator=torch.Generator().manual_seed(77))).numpy()
    lim, plain = orc.initialize_cache(B), orc.initialize_cache(B)
    out_lim, out_plain, shares, bins = [], [], [], []
    for t in range(HOPS):
        xt = x[:, t * H:(t + 1) * H]
        (o, *lim), share, xc, yc, yl = step(orc, xt, *lim, gains=GAINS)
        out_lim.append(o)
        shares.append(share)
        bins.append((xc, yc, yl))
        o, *plain = orc.step(xt, *plain)
        out_plain.append(o)
    return dict(x=x, out=np.concatenate(out_lim, axis=1), tail=np.asarray(lim[1]), plain=np.concatenate(out_plain, axis=1), plain_caches=plain,
                caches=lim, shares=np.asarray(shares), bins=bins, compression=float(cfg.input_compression), hop=H)


def rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return rms(got - ref) / max(rms(ref), 1e-3)
