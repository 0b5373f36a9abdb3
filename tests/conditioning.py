"""Conditioning perturbations (test helper): seeded, deterministic edits of a training-form state dict or of an input that drive one
numerically delicate step of a model into its hard regime, so that the kernels are compared with the fp64 oracle where fp32 can lose
digits.  Both the HIP model (`load_state_dict`) and the oracle (`fold_state_dict`) are built from the edited state dict.

- `norm_offset(family, ratio, x)`: a common offset at the input of the norm sites, so that |mean| / std >= ratio there.  A GroupNorm /
  LayerNorm removes a constant exactly, so an offset added through a bias leaves everything downstream unchanged (in exact
  arithmetic): the sites are calibrated on one fp64 pass and offset in one step.
- `gru_saturate`, `attention_sharpen`: scaled GRU / attention weights (weight-norm gains), so that many GRU pre-activations exceed 15
  in magnitude and the largest attention logits reach about 60.
- input generators next to `oracle.weightgen.make_input`.

`measure_*` restate what each perturbation promises, on the fp64 oracle; tests/test_conditioning.py checks them on the CPU."""
from __future__ import annotations

import copy

import numpy as np

import oracle.fe_oracle as feo
import oracle.lisennet_oracle as lo
from common import FSPEN_KWARGS, LISENNET_KWARGS, MODEL_KWARGS, build_oracle
from oracle.weightgen import make_input

NORM_RATIOS = (10, 30, 100)
SUB_CLAMP_LEVEL = 1e-8


# ---------------------------------------------------------------- oracles of an edited state dict
def fe_oracle(name, sd, dtype=np.float64):
    cfg = build_oracle(name)[0]
    return feo.FEOracle(cfg, feo.fold_state_dict(sd, cfg), dtype)


def fspen_oracle(sd, dtype=np.float64):
    from oracle import fspen_oracle as fo
    cfg = fo.FSPENConfig.from_model_kwargs(FSPEN_KWARGS[0])
    return fo.FSPENOracle(cfg, fo.fold_state_dict(sd, cfg), dtype)


def lisennet_oracle(sd, dtype=np.float64):
    cfg = lo.LiSenNetConfig.from_model_kwargs(LISENNET_KWARGS[0])
    return lo.LiSenNetOracle(cfg, sd, dtype)


class LiSenNetSplitOracle(lo.LiSenNetOracle):
    """LiSenNet's fp64 oracle with the fp32 oracle's front end.  LiSenNet's input features are phase differences wrapped to (-pi, pi]:
    where one sits at +-pi, the last bit of the spectrum flips it by 2 pi, and fp32 and fp64 disagree by ~2e-2 on the unperturbed
    checkpoint already.  So the STFT, the compression and the features are the fp32 oracle's, bit for bit, and the network after them
    runs in fp64: its error against the fp32 oracle is what fp32 arithmetic costs in the network itself.  (The STFT cache holds fp32
    input samples, so the fp32 front end's cache is the fp64 one rounded - exactly.)"""

    def __init__(self, sd):
        cfg = lo.LiSenNetConfig.from_model_kwargs(LISENNET_KWARGS[0])
        super().__init__(cfg, sd, np.float64)
        self.o32 = lo.LiSenNetOracle(cfg, sd, np.float32)
        self._spec32 = None

    def step(self, wav_in, cache_stft, *caches, taps=None):
        self._spec32, _ = self.o32.stft_step(wav_in, cache_stft.astype(np.float32))       # (read by features() within this step)
        try:
            return super().step(wav_in, cache_stft, *caches, taps=taps)
        finally:
            self._spec32 = None

    def features(self, spec, pha_prev, onnx):
        c = self.cfg
        s = self._spec32       # (the compression of LiSenNetOracle.spec_forward, in fp32)
        mag = np.maximum(np.sqrt(s[..., 0:1] ** 2 + s[..., 1:2] ** 2), np.float32(1e-5))
        s = s * mag ** np.float32(c.input_compression - 1.0)
        feat, pha = self.o32.features(s, None if pha_prev is None else pha_prev.astype(np.float32), onnx)
        return feat.astype(np.float64), pha.astype(np.float64)


def base_state_dict(family):
    """(training-form state dict, sampling rate, hop) of `fe_<...>` / "fspen" / "lisennet" - the suite's seeded checkpoints"""
    from common import build_fspen_oracle, build_lisennet_oracle
    if family == "fspen":
        cfg, sd, _, _ = build_fspen_oracle()
        return sd, FSPEN_KWARGS[1], cfg.hop_size
    if family == "lisennet":
        cfg, sd, _, _ = build_lisennet_oracle()
        return sd, LISENNET_KWARGS[1], cfg.hop_size
    cfg, sd, _, _ = build_oracle(family)
    return sd, MODEL_KWARGS[family][1], cfg.hop_size


def make_oracle(family, sd, dtype=np.float64):
    if family == "fspen":
        return fspen_oracle(sd, dtype)
    if family == "lisennet":
        return lisennet_oracle(sd, dtype)
    return fe_oracle(family, sd, dtype)


def reference_oracle(family, sd):
    """the high-precision reference of the GPU tests: the fp64 oracle (LiSenNet: with the fp32 front end, LiSenNetSplitOracle)"""
    return LiSenNetSplitOracle(sd) if family == "lisennet" else make_oracle(family, sd)


def run_oracle(orc, x, hop, taps_per_hop=None):
    """the streaming oracle over the hops of x [B, n]: (output [B, n], final caches); taps_per_hop, if given, receives one dict per hop"""
    caches = orc.initialize_cache(x.shape[0])
    outs = []
    for t in range(x.shape[1] // hop):
        taps = {} if taps_per_hop is not None else None
        o, *caches = orc.step(x[:, t * hop:(t + 1) * hop], *caches, taps=taps)
        outs.append(o)
        if taps is not None:
            taps_per_hop.append(taps)
    return np.concatenate(outs, axis=1), caches


def prenorm_stats(family, sd, x, hop):
    """site -> (smallest |mean| / std, largest std, largest |mean|) over every sample of every hop, fp64 oracle"""
    hops = []
    run_oracle(make_oracle(family, sd), x, hop, hops)
    out = {}
    for k in hops[0]:
        if not k.startswith("prenorm."):
            continue
        site = k[len("prenorm."):]
        r = np.concatenate([np.ravel(h[k]) for h in hops])
        s = np.concatenate([np.ravel(h["prenorm_std." + site]) for h in hops])
        m = np.concatenate([np.ravel(h["prenorm_mean." + site]) for h in hops])
        out[site] = (float(r.min()), float(s.max()), float(np.abs(m).max()))
    return out


def _offset(stats, site, ratio):
    """the offset that puts every sample of `site` at |mean| / std >= ratio (mean + off >= off - |mean| >= ratio * std), 5 % margin"""
    _, s, m = stats[site]
    return np.float32(1.05 * (ratio * s + m))


# ---------------------------------------------------------------- norm_offset
FE_LN_FORCED = 0      # the channel the fastenhancer.ln perturbation pins: GRU output / GroupNorm output held constant (see below)


def fe_ln_norm_offset(name, sd, ratio, x):
    """fastenhancer.ln (`fe_ln_b`): every norm site but the blocks' attn_post_norm at |mean| / std >= ratio.

    - conv + bias -> GroupNorm (enc_pre.0, encoder.i.0, rf_pre.1, rf_post.1, decoder.i.0): the offset goes into the bias.
    - the bias-free convs (decoder.i.3, dec_post.0): input channel FE_LN_FORCED of each is made a constant, silu(1) - the gain of that
      channel of the GroupNorm before it (decoder.i.1 / decoder.{last}.4) set to 0, its shift to 1 - and the conv reads it through its
      centre tap only, so that tap times silu(1) is the same at every frequency (no zero padding reaches it).
    - rnn_post_norm (input: GRU output @ rnn_fc.weight.T, no bias): GRU channel FE_LN_FORCED is pinned at h = 1 (update gate bias -60:
      z = 0; candidate bias +60: n = tanh(>= 30) = 1 in fp32 and fp64), and column FE_LN_FORCED of rnn_fc.weight adds the offset.
    - attn_post_norm is not reached: the attention output has no constant direction to carry an offset."""
    cfg = build_oracle(name)[0]
    sd = copy.deepcopy(sd)
    C2, j, nl = cfg.rf_channels, FE_LN_FORCED, cfg.n_layers
    for i in range(nl):
        sd[f"decoder.{i}.1.weight"][j], sd[f"decoder.{i}.1.bias"][j] = 0.0, 1.0
        w = sd[f"decoder.{i}.3.weight"]
        w[:, j, :] = 0.0
    sd[f"decoder.{nl - 1}.4.weight"][j], sd[f"decoder.{nl - 1}.4.bias"][j] = 0.0, 1.0
    sd["dec_post.0.weight"][:, j, :] = 0.0
    for k in range(cfg.rf_blocks):
        b = sd[f"rf_block.{k}.rnn.bias_ih_l0"]
        b[C2 + j], b[2 * C2 + j] = -60.0, 60.0
        sd[f"rf_block.{k}.rnn_fc.weight"][:, j] = 0.0
    st = prenorm_stats(name, sd, x, cfg.hop_size)
    s1 = np.float32(feo.silu(np.float64(1.0)))
    for key in ["enc_pre.0"] + [f"encoder.{i}.0" for i in range(nl)] + ["rf_pre.1", "rf_post.1"] + [f"decoder.{i}.0" for i in range(nl)]:
        site = key[:-1] + str(int(key[-1]) + 1)             # the GroupNorm after the conv
        sd[key + ".bias"] = sd[key + ".bias"] + _offset(st, site, ratio)
    for i in range(nl):
        w = sd[f"decoder.{i}.3.weight"]
        w[:, j, w.shape[2] // 2] = _offset(st, f"decoder.{i}.4", ratio) / s1
    sd["dec_post.0.weight"][:, j, 0] = _offset(st, "dec_post.1", ratio) / s1
    for k in range(cfg.rf_blocks):
        sd[f"rf_block.{k}.rnn_fc.weight"][:, j] = _offset(st, f"rf_block.{k}.rnn_post_norm", ratio)
    return sd


def fe_ln_offset_sites(name):
    cfg = build_oracle(name)[0]
    nl = cfg.n_layers
    return (["enc_pre.1"] + [f"encoder.{i}.1" for i in range(nl)] + ["rf_pre.2", "rf_post.2"] + [f"decoder.{i}.{k}" for i in range(nl) for k in (1, 4)]
            + ["dec_post.1"] + [f"rf_block.{k}.rnn_post_norm" for k in range(cfg.rf_blocks)])


def fspen_norm_offset(sd, ratio, x, hop):
    """FSPEN: each DPE block's intra LayerNorm (input: intra GRU outputs @ intra_fc.weight.T + intra_fc.bias) - offset in the bias"""
    sd = copy.deepcopy(sd)
    st = prenorm_stats("fspen", sd, x, hop)
    for site in fspen_offset_sites(sd):
        p = site[:-len("intra_ln")]
        sd[p + "intra_fc.bias"] = sd[p + "intra_fc.bias"] + _offset(st, site, ratio)
    return sd


def fspen_offset_sites(sd):
    return sorted(k[:-len(".weight")] for k in sd if k.endswith("intra_ln.weight"))


def lisennet_norm_offset(sd, ratio, x, hop, residual=True):
    """LiSenNet: every norm site.

    - conv + bias -> CustomLayerNorm (encoder.conv_1, the three DSConvs - low and high conv biases alike -, decoder.mask_conv): the
      offset goes into the biases.
    - the dual-path blocks' intra / inter LayerNorms and the ConvGLU norms read the residual stream, which starts at encoder.conv_4's
      output: its norm shift (beta, per frequency) gets a common offset, large enough that the PReLU after it passes everything and
      the residual stream carries the offset through both blocks.  That offset does change what follows, so it is calibrated first
      (a few fp64 passes); the bias offsets then leave it as it is."""
    sd = copy.deepcopy(sd)
    blocks = lisennet_residual_sites(sd)
    beta = sd["encoder.conv_4.norm.beta"].copy()
    off = np.float32(0.0)
    for _ in range(8 if residual else 0):
        st = prenorm_stats("lisennet", sd, x, hop)
        worst = min(st[s][0] for s in blocks)
        if worst >= 1.02 * ratio:
            break
        # ratio ~ (off + m) / s at the residual sites: step the offset by what the worst site lacks
        s = max(st[s_][1] for s_ in blocks)
        off = np.float32(off + 1.5 * (1.05 * ratio - worst) * s)
        sd["encoder.conv_4.norm.beta"] = beta + off
    st = prenorm_stats("lisennet", sd, x, hop)
    for site, keys in lisennet_bias_sites().items():
        o = _offset(st, site, ratio)
        for k in keys:
            sd[k] = sd[k] + o
    return sd


def lisennet_bias_sites():
    return {"encoder.conv_1.1": ["encoder.conv_1.0.bias"],
            **{f"encoder.conv_{i}.norm": [f"encoder.conv_{i}.low_conv.bias", f"encoder.conv_{i}.high_conv.bias"] for i in (2, 3, 4)},
            "decoder.mask_conv.1": ["decoder.mask_conv.0.bias"]}


def lisennet_residual_sites(sd):
    return sorted({k.rsplit(".", 1)[0] for k in sd if k.endswith(("intra_norm.weight", "inter_norm.weight", "conv_glu.norm.gamma"))})


def norm_offset(family, ratio, x):
    """(edited state dict, the sites it targets) of `family` at |mean| / std >= ratio on input x"""
    sd, sr, hop = base_state_dict(family)
    if family == "fspen":
        return fspen_norm_offset(sd, ratio, x, hop), fspen_offset_sites(sd)
    if family == "lisennet":
        return lisennet_norm_offset(sd, ratio, x, hop), list(lisennet_bias_sites()) + lisennet_residual_sites(sd)
    return fe_ln_norm_offset(family, sd, ratio, x), fe_ln_offset_sites(family)


# ---------------------------------------------------------------- GRU saturation, sharp attention
# per model: the factor that takes its GRU gate pre-activations beyond +-15 in a sizeable fraction (> 10 %), and its attention logits to
# about 60 (tests/test_conditioning.py measures both on the fp64 oracle)
# (fe_dprnn_b: 5 puts 3 % beyond +-15; at 6 its fp32 oracle already drifts 1e-4 from the fp64 one, at 8 by 1e-2 - chaotic, not a test)
GRU_FACTOR = {"fe_b": 8.0, "fe_dprnn_b": 5.0, "fe_nc": 6.0, "fspen": 4.0}
GRU_FRACTION = {"fe_b": 0.1, "fe_dprnn_b": 0.03, "fe_nc": 0.1, "fspen": 0.1}
ATTN_FACTOR = {("fe_b", "attn"): 1.7, ("fe_t", "attn"): 2.4, ("fe_dpt_b", "time_attn"): 1.75}


def _gru_param(k):
    leaf = k.split(".")[-1]
    if "rnn" not in k.replace("rnn_fc", "").replace("rnn_post_norm", "").replace("inter_fc", ""):
        return False
    if ".parametrizations." in k:                       # weight norm: the gain g scales the weight
        return leaf == "original0"
    return leaf.startswith(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))


def gru_saturate(sd, factor):
    """every GRU (uni- and bidirectional, intra / inter): input and recurrent weights (their weight-norm gains) and biases times factor"""
    sd = copy.deepcopy(sd)
    for k in sd:
        if _gru_param(k):
            sd[k] = (sd[k] * np.float32(factor)).astype(np.float32)
    return sd


def attention_sharpen(sd, factor, which="attn"):
    """the qkv projections of every block's frequency attention ("attn") or time attention ("time_attn"): weight-norm gain (or weight)
    times factor - the logits q.k grow with factor^2, and faster through the blocks"""
    sd = copy.deepcopy(sd)
    for k in sd:
        if f".{which}.qkv." in k and k.endswith(("original0", "qkv.weight")):
            sd[k] = (sd[k] * np.float32(factor)).astype(np.float32)
    return sd


def hard_state_dict(family, hard):
    """(family's seeded state dict under `hard`: "gru" / "attn" / "time_attn", sampling rate, hop)"""
    sd0, sr, hop = base_state_dict(family)
    if hard == "gru":
        return gru_saturate(sd0, GRU_FACTOR[family]), sr, hop
    return attention_sharpen(sd0, ATTN_FACTOR[(family, hard)], hard), sr, hop


def measure_gru_and_attention(family, sd, x, offline=False):
    """(fraction of GRU pre-activations with |.| > 15, largest |attention logit| - frequency or time attention) of the fp64 oracle on x:
    the streaming oracle, or offline_forward"""
    from oracle import fspen_oracle as fo
    pre, logits = [], [0.0]
    saved = feo.gru_step, feo.mhsa, feo.causal_time_attention, fo.gru_cell

    def gru(xx, h, w_ih, w_hh, b_ih, b_hh):
        C = h.shape[1]
        gi, gh = xx @ w_ih.T + b_ih, h @ w_hh.T + b_hh
        r = feo.sigmoid(gi[:, :C] + gh[:, :C])
        pre.extend([np.ravel(gi[:, :2 * C] + gh[:, :2 * C]), np.ravel(gi[:, 2 * C:] + r * gh[:, 2 * C:])])
        return saved[0](xx, h, w_ih, w_hh, b_ih, b_hh)

    def gru_fspen(xx, h, w_ih, w_hh, b_ih, b_hh):
        gru(xx, h, w_ih, w_hh, b_ih, b_hh)
        return saved[3](xx, h, w_ih, w_hh, b_ih, b_hh)

    def mhsa(xx, w_qkv, nh):
        M, F, C = xx.shape
        hd = C // nh
        qkv = (xx @ w_qkv.T).reshape(M, F, nh, 3 * hd).transpose(0, 2, 1, 3)
        logits.append(float(np.abs(qkv[..., :hd] @ qkv[..., hd:2 * hd].transpose(0, 1, 3, 2) * hd ** -0.5).max()))
        return saved[1](xx, w_qkv, nh)

    def time_attn(xx, w_qkv, pe, nh, L, h_k, h_v):
        M, T, C = xx.shape
        hd = C // nh
        qkv = (xx @ w_qkv.T).reshape(M, T, nh, 3 * hd).transpose(0, 2, 1, 3)
        kk = np.concatenate([np.zeros((M, nh, L, hd)) if h_k is None else h_k, qkv[..., hd:2 * hd]], axis=2)
        for t in range(T):        # frame t's window, as causal_time_attention scores it (masked slots of a cache-less call included)
            a = pe[None] + hd ** -0.5 * np.einsum("mnd,mnjd->mnj", qkv[:, :, t, :hd], kk[:, :, t:t + L + 1])
            logits.append(float(np.abs(a).max()))
        return saved[2](xx, w_qkv, pe, nh, L, h_k, h_v)

    feo.gru_step, feo.mhsa, feo.causal_time_attention, fo.gru_cell = gru, mhsa, time_attn, gru_fspen
    try:
        orc = make_oracle(family, sd)
        if offline:
            orc.offline_forward(x)
        else:
            run_oracle(orc, x, base_state_dict(family)[2])
    finally:
        feo.gru_step, feo.mhsa, feo.causal_time_attention, fo.gru_cell = saved
    p = np.abs(np.concatenate(pre)) if pre else np.zeros(1)
    return float((p > 15.0).mean()), max(logits)


# ---------------------------------------------------------------- inputs
def dc_input(B, n, seed, sr, dc=0.4):
    """the suite's input plus a constant offset (clipped to [-1, 1])"""
    return np.clip(make_input(B, n, seed, sr) + np.float32(dc), -1.0, 1.0).astype(np.float32)


def clipped_noise_input(B, n, seed):
    """full-scale noise: N(0, 1) clipped to [-1, 1] - a third of the samples sit on the rails"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.clip(rng.standard_normal((B, n)), -1.0, 1.0).astype(np.float32)


def impulse_input(B, n, seed):
    """isolated unit impulses of either sign on silence, a few per stream at seeded positions"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros((B, n), np.float32)
    for b in range(B):
        pos = rng.choice(n, size=max(1, n // 700), replace=False)
        x[b, pos] = rng.choice([-1.0, 1.0], size=pos.size)
    return x


def sub_clamp_input(B, n, seed, sr, level=1e-8):
    """the suite's input scaled so that every STFT bin is far below the 1e-5 magnitude clamp of the compression"""
    return (make_input(B, n, seed, sr) * np.float32(level)).astype(np.float32)


def mixed_batch_input(B, n, seed, sr):
    """streams cycling through silence, a quiet stream (1e-3 of the suite's input) and full-scale clipped noise"""
    x = make_input(B, n, seed, sr)
    loud = clipped_noise_input(B, n, seed + 1)
    x[0::3] = 0.0
    x[1::3] *= np.float32(1e-3)
    x[2::3] = loud[2::3]
    return x
