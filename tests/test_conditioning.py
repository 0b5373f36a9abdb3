"""CPU checks of the conditioning perturbations (tests/conditioning.py): each reaches its regime in the fp64 oracle - without that a GPU
test could pass because it never met the hard case - and the fp32 oracle stays close to the fp64 one there, so that a kernel that
misses is a kernel defect, not an ill-posed problem."""
import numpy as np
import pytest

import conditioning as C
from oracle.weightgen import make_input


def _e32(family, sd, x, hop):            # (the default model: the fp64 oracle is the reference)
    o64, _ = C.run_oracle(C.make_oracle(family, sd), x, hop)
    o32, _ = C.run_oracle(C.make_oracle(family, sd, np.float32), x, hop)
    return float(np.sqrt(np.mean((o32 - o64) ** 2)) / max(np.sqrt(np.mean(o64 ** 2)), 1e-3))


# (family, B, hops, input seed): the inputs test_gpu_conditioning.py uses
NORM_CASES = [("fe_ln_b", 4, 8, 4242), ("fspen", 5, 5, 4243), ("lisennet", 5, 4, 4244)]


@pytest.mark.parametrize("ratio", C.NORM_RATIOS)
@pytest.mark.parametrize("family,B,hops,seed", NORM_CASES)
def test_norm_offset_reaches_the_ratio_at_every_targeted_site(family, B, hops, seed, ratio):
    sd0, sr, hop = C.base_state_dict(family)
    x = make_input(B, hops * hop, seed, sr)
    sd, sites = C.norm_offset(family, ratio, x)
    st = C.prenorm_stats(family, sd, x, hop)
    assert set(sites) <= set(st), set(sites) - set(st)
    low = {s: st[s][0] for s in sites if st[s][0] < ratio}
    assert not low, f"{family}: sites below |mean| / std = {ratio}: {low}"
    if family == "fe_ln_b":       # 13 of the 16 norm sites (not the blocks' attn_post_norm), the GRU channel pinned at 1
        assert len(sites) == 13 and len(st) == 16
    if family == "lisennet":      # every norm site of the model is targeted
        assert set(sites) == set(st)


def test_norm_offset_leaves_the_unperturbed_sites_benign():
    sd0, sr, hop = C.base_state_dict("fe_ln_b")
    st = C.prenorm_stats("fe_ln_b", sd0, make_input(4, 8 * hop, 4242, sr), hop)
    assert max(v[0] for v in st.values()) < 3.0, st          # (the synthetic checkpoint never gets near the hard regime)


@pytest.mark.parametrize("family,B,hops,seed", NORM_CASES)
def test_fp32_oracle_stays_close_to_the_reference_under_norm_offset(family, B, hops, seed):
    """at |mean| / std = 100 the fp32 oracle (centred variance) is within half the north_star bound of the high-precision reference.
    (Not within the regression bound: the fp32 inputs of a norm carry a rounding of eps * |offset| = 100 eps * std already.)"""
    sd0, sr, hop = C.base_state_dict(family)
    x = make_input(B, hops * hop, seed, sr)
    sd, _ = C.norm_offset(family, 100, x)
    o32, _ = C.run_oracle(C.make_oracle(family, sd, np.float32), x, hop)
    ref, _ = C.run_oracle(C.reference_oracle(family, sd), x, hop)
    assert np.sqrt(np.mean((o32 - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)) < 5e-5


def test_lisennet_reference_keeps_the_fp32_front_end():
    """why LiSenNet's reference is LiSenNetSplitOracle: with fp64 phase features the fp32 oracle is 1e-3+ off on the unperturbed checkpoint
    (phase differences at +-pi flip with the last bit), with the fp32 oracle's own features the network alone is 1e-6 off"""
    sd0, sr, hop = C.base_state_dict("lisennet")
    x = make_input(5, 4 * hop, 4244, sr)
    o32, _ = C.run_oracle(C.make_oracle("lisennet", sd0, np.float32), x, hop)
    for orc, lo, hi in ((C.make_oracle("lisennet", sd0), 1e-3, np.inf), (C.reference_oracle("lisennet", sd0), 0.0, 1e-6)):
        ref, _ = C.run_oracle(orc, x, hop)
        e = np.sqrt(np.mean((o32 - ref) ** 2)) / np.sqrt(np.mean(ref ** 2))
        assert lo < e < hi, (type(orc).__name__, e)


# (family, perturbation, B, hops, input seed, offline): the cases test_gpu_conditioning.py runs
HARD_CASES = [("fe_b", "gru", 4, 6, 911, False), ("fe_dprnn_b", "gru", 3, 6, 912, False), ("fe_nc", "gru", 2, 6, 914, True),
              ("fspen", "gru", 5, 5, 915, False), ("fe_b", "attn", 4, 6, 911, False), ("fe_t", "attn", 3, 6, 913, False),
              ("fe_dpt_b", "time_attn", 2, 35, 913, False)]


@pytest.mark.parametrize("family,hard,B,hops,seed,offline", HARD_CASES)
def test_gru_saturation_and_sharp_attention_reach_their_regimes(family, hard, B, hops, seed, offline):
    """each model's GRUs saturate (a sizeable fraction of |gate pre-activation| > 15) or its attention's largest logits reach ~60, in
    the fp64 oracle on the GPU test's input - and the fp32 oracle stays within the suite's regression bound of the fp64 one"""
    sd0, sr, hop = C.base_state_dict(family)
    x = make_input(B, hops * hop + (17 if offline else 0), seed, sr)
    frac0, logit0 = C.measure_gru_and_attention(family, sd0, x, offline)
    sd, _, _ = C.hard_state_dict(family, hard)
    frac, logit = C.measure_gru_and_attention(family, sd, x, offline)
    if hard == "gru":
        assert frac0 < 0.01 and frac > C.GRU_FRACTION[family], (frac0, frac)
    else:
        assert logit0 < 15.0 and 50.0 <= logit <= 120.0, (logit0, logit)
    if offline:
        o64, o32 = C.make_oracle(family, sd).offline_forward(x)[0], C.make_oracle(family, sd, np.float32).offline_forward(x)[0]
        e = float(np.sqrt(np.mean((o32 - o64) ** 2)) / np.sqrt(np.mean(o64 ** 2)))
    else:
        e = _e32(family, sd, x, hop)
    assert e < 2e-5, e


@pytest.mark.parametrize("kind", ["dc", "clipped_noise", "sub_clamp", "impulses", "mixed"])
def test_edge_inputs_are_what_they_claim(kind):
    sr, hop, n = 16000, 256, 6 * 256
    if kind == "dc":
        x = C.dc_input(3, n, 51, sr)
        assert abs(float(x.mean()) - 0.4) < 0.05
    elif kind == "clipped_noise":
        x = C.clipped_noise_input(3, n, 52)
        assert 0.25 < float((np.abs(x) == 1.0).mean()) < 0.4
    elif kind == "sub_clamp":
        x = C.sub_clamp_input(3, n, 53, sr, C.SUB_CLAMP_LEVEL)
        sd0, _, _ = C.base_state_dict("fe_b")
        orc = C.make_oracle("fe_b", sd0)
        cache = orc.initialize_cache(3)[0]
        for t in range(6):
            spec, cache = orc.stft_step(x[:, t * hop:(t + 1) * hop], cache)
            assert float(np.sqrt((np.asarray(spec, np.float64) ** 2).sum(-1)).max()) < 1e-5 / 10     # every bin well below the clamp
    elif kind == "impulses":
        x = C.impulse_input(3, n, 54)
        assert set(np.unique(x)) <= {-1.0, 0.0, 1.0} and all(0 < np.count_nonzero(r) <= 5 for r in x)
    else:
        x = C.mixed_batch_input(6, n, 55, sr)
        assert float(np.abs(x[0::3]).max()) == 0.0 and float(np.abs(x[1::3]).max()) < 2e-3 and float(np.abs(x[2::3]).max()) == 1.0
    assert x.dtype == np.float32 and np.isfinite(x).all() and float(np.abs(x).max()) <= 1.0
