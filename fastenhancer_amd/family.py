"""The four model families (FastEnhancer and its variants, BSRNN, FSPEN, LiSenNet), each described once for the Python layer - the
counterpart of the C++ host code's `Family` entries.  `family_of(cfg)` finds the description from the config's type; Engine and the
model mirrors ask it wherever the families differ, so adding a family is one config class (config.py), its checkpoint functions
(weights.py), one entry here and a model.py with its docstrings and constructor.

The model's caches appear in two orders: the reference's cache list (`cfg.cache_shapes(B)`: what initialize_cache returns and forward
threads) and the C ABI state (include/fastenhancer_hip.h).  `split` and `order` map between them; only FastEnhancer's time_kernel and
dptransformer variants differ from the identity."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Sequence

import torch
from torch import Tensor

from . import _lib, weights as W
from .config import BSRNNConfig, FEConfig, FSPENConfig, LiSenNetConfig


def views(flat: Tensor, shapes: Sequence[Sequence[int]]) -> List[Tensor]:
    """consecutive views of a flat tensor, one per shape"""
    out, o = [], 0
    for s in shapes:
        n = math.prod(s)
        out.append(flat[o:o + n].view(*s))
        o += n
    return out


def _shapes(expected) -> Callable:
    return lambda fused, cfg, strict=True: W.check_shapes(fused, expected(cfg), strict=strict)


@dataclass(frozen=True)
class Family:
    arch: int                       # FE_ARCH_*
    fill_config: Callable           # (fe_config, cfg): the family's fields of the fe_config for fe_create
    fold: Callable                  # (state_dict, cfg) -> fused state dict, the tensors the weight sections name
    check: Callable                 # (fused, cfg, strict): shapes and names against what the kernels expect
    default_state_dict: Callable    # (cfg, generator=None) -> random weights of the right shapes
    nyquist: bool = True            # the model's spectrum keeps the Nyquist bin (n_fft/2 + 1 bins)
    # h = the model's part of a C ABI state for B streams (what fe_spec_step takes); caches = the reference's cache list
    split: Callable = lambda cfg, h, B, head0=False: views(h, cfg.cache_shapes(B))      # h -> caches
    order: Callable = lambda cfg, caches: [t.reshape(-1) for t in caches]               # caches -> flat pieces of h, in its order
    start: Callable = lambda cfg, h, B: None                                            # zeroed h -> the state of a call without caches
    backlog: bool = False           # chunks of many hops go through Engine.step_backlog (fe_step_backlog pipelines the family), not step_chunk
    backlog_on_request: bool = False  # ... and fe_step_backlog pipelines the family when handed Engine.lisennet_backlog_work(B, T) (LiSenNet)
    pool: bool = False              # the slotted step of live streams is Engine.step_pool (fe_step_slots refuses the family), not step_slots

    def spec_bins(self, cfg) -> int:
        return cfg.F0 + (1 if self.nyquist else 0)


# ---------------------------------------------------------------- FastEnhancer (default, ln, dprnn, time_kernel, dptransformer, noncausal)
def _fe_config(c, cfg: FEConfig):
    c.channels = cfg.channels
    c.n_kernels = len(cfg.kernel_size)
    for i, k in enumerate(cfg.kernel_size):
        c.kernel_size[i] = k
    c.stride = cfg.stride
    c.rf_channels, c.rf_freq, c.rf_blocks, c.rf_heads = cfg.rf_channels, cfg.rf_freq, cfg.rf_blocks, cfg.rf_heads
    c.kernel_size_time = cfg.kernel_size_time
    c.channels_frnn = cfg.channels_frnn
    c.lookbehind = cfg.lookbehind
    c.ln = 1 if cfg.ln else 0
    c.rf_eps = cfg.rf_eps
    c.bidirectional = 1 if cfg.noncausal else 0
    c.activation, c.activation_param, c.mask = cfg.activation, cfg.activation_param, cfg.mask


def _fe_split(c: FEConfig, h: Tensor, B: int, head0: bool = False) -> List[Tensor]:
    K, nl = c.rf_blocks, c.n_layers
    if c.dpt:
        # In the state every K / V cache is a ring over its L slots with one head per stream, the heads [B] after the rings
        # (include/fastenhancer_hip.h, fe_config.lookbehind): the reference's tensors (oldest frame first) are the rings rotated left
        # by head - one gathered copy (made on the device without looking at the heads: no device-to-host sync on the per-hop path),
        # or views when the caller knows every head is 0 (head0: a fresh state)
        shape = (2 * K, B, c.rf_freq, c.rf_heads, c.lookbehind, c.rf_channels // c.rf_heads)
        n, L = math.prod(shape), c.lookbehind
        rings = h[:n].view(shape)
        if not head0:
            idx = (h[n:n + B].long()[:, None] + torch.arange(L, device=h.device)[None, :]) % L             # [B, L]
            rings = torch.gather(rings, 4, idx[None, :, None, None, :, None].expand(shape))
        return [t.reshape(B * c.rf_freq, *shape[3:]) for t in rings]
    # the state holds the GRU states, then (time_kernel variant) the causal convs' frame caches as [B, kt-1, F1, C1]; the reference
    # tensors (B, C1, kt-1, F1) are permuted views of them, and its list is encoder caches, GRU states, decoder caches
    # (models/fastenhancer/time_kernel/model.py:746-754)
    vs = views(h, [(1, B * c.rf_freq, c.rf_channels)] * K
               + [(B, c.kernel_size_time - 1, c.F1, c.channels)] * (2 * nl if c.time_kernel else 0))
    conv = [t.permute(0, 3, 1, 2) for t in vs[K:]]
    return conv[:nl] + vs[:K] + conv[nl:]


def _fe_order(c: FEConfig, caches: List[Tensor]) -> List[Tensor]:
    if c.dpt:      # reference-order caches = rings with head 0
        B = caches[0].shape[0] // c.rf_freq
        return [t.reshape(-1) for t in caches] + [torch.zeros(B, dtype=torch.float32, device=caches[0].device)]
    if not c.time_kernel:
        return [t.reshape(-1) for t in caches]
    nl, K = c.n_layers, c.rf_blocks
    assert len(caches) == 2 * nl + K, f"expected {2 * nl + K} caches, got {len(caches)}"
    conv = lambda t: t.permute(0, 2, 3, 1).reshape(-1)          # (B, C1, kt-1, F1) -> [B, kt-1, F1, C1]
    return [t.reshape(-1) for t in caches[nl:nl + K]] + [conv(t) for t in caches[:nl]] + [conv(t) for t in caches[nl + K:]]


def _fe_start(c: FEConfig, h: Tensor, B: int) -> None:
    """the dptransformer variant without caches masks the frames before the start (dptransformer/model.py:216-218) instead of
    attending to zero caches: marked by +inf in the first element of every K slot (fe_config.lookbehind).  (The caches returned keep
    all L slots, the not-yet-filled ones still marked; the reference returns min(T, L) slots.)"""
    if c.dpt:
        n = B * c.rf_freq * c.rf_channels * c.lookbehind
        h[:2 * c.rf_blocks * n].view(c.rf_blocks, 2, -1, c.rf_channels // c.rf_heads)[:, 0, :, 0] = float("inf")


# ---------------------------------------------------------------- the baselines
def _bsrnn_config(c, cfg: BSRNNConfig):
    c.channels, c.rf_blocks = cfg.num_channels, cfg.num_layers


def _fspen_config(c, cfg: FSPENConfig):
    c.channels = cfg.channels[-1]
    c.n_kernels = len(cfg.kernel_size)
    for i, k in enumerate(cfg.kernel_size):
        c.kernel_size[i] = k
    if len(set(cfg.stride)) != 1 or list(cfg.channels) != [4, 16, 32]:
        raise _lib.FEError(f"no FSPEN kernel compiled for channels={list(cfg.channels)} stride={list(cfg.stride)} "
                           "(configs/others/fspen.yaml is the compiled architecture)")
    c.stride = cfg.stride[0]
    c.rf_channels, c.rf_freq, c.rf_blocks, c.rf_heads = cfg.dpe_channels, cfg.freq, cfg.num_blocks, cfg.groups


def _lisennet_config(c, cfg: LiSenNetConfig):
    c.channels, c.rf_blocks = cfg.num_channels, cfg.n_blocks


_FAMILIES = {
    FEConfig: Family(_lib.FE_ARCH_FASTENHANCER, _fe_config, W.fold_state_dict, W.check_fused, W.default_state_dict, nyquist=False,
                     split=_fe_split, order=_fe_order, start=_fe_start),
    BSRNNConfig: Family(_lib.FE_ARCH_BSRNN, _bsrnn_config, W.bsrnn_fold_state_dict, _shapes(W.bsrnn_expected_fused_shapes),
                        W.bsrnn_default_state_dict, backlog=True, pool=True),
    FSPENConfig: Family(_lib.FE_ARCH_FSPEN, _fspen_config, W.fspen_fold_state_dict, _shapes(W.fspen_expected_fused_shapes),
                        W.fspen_default_state_dict, backlog=True, pool=True),
    LiSenNetConfig: Family(_lib.FE_ARCH_LISENNET, _lisennet_config, W.lisennet_state_dict, _shapes(W.lisennet_expected_shapes),
                           W.lisennet_default_state_dict, pool=True, backlog_on_request=True),
}


def family_of(cfg) -> Family:
    return _FAMILIES[type(cfg)]


def chunk_step(engine) -> Callable:
    """The engine's call for a chunk of many hops of few streams (streaming.enhance_stream(chunk_hops=...), StreamPool.catch_up):
    step_backlog for the families fe_step_backlog pipelines (BSRNN, FSPEN), step_chunk for every other - FastEnhancer's own path as it
    has always been called.  LiSenNet: step_chunk too - the walk of step() - unless the engine's time pipeline was set to an explicit
    width of two or more: then step_backlog with the engine's scratch tensor sized for that family's pipelined launch."""
    fam = _FAMILIES.get(type(getattr(engine, "cfg", None)))
    if fam is not None and fam.backlog_on_request and getattr(engine, "_time_pipeline", -1) >= 2:
        def step(wav_in, state, wav_out=None, T=None):
            hops = wav_in.shape[1] // engine.cfg.hop_size if T is None else T
            return engine.step_backlog(wav_in, state, wav_out, T=T, work=engine.lisennet_backlog_work(wav_in.shape[0], hops))
        return step
    return engine.step_backlog if fam is not None and fam.backlog else engine.step_chunk


def slot_step(engine) -> Callable:
    """The engine's call for one step of the named slots of a state buffer (StreamPool.step): step_pool for the families whose slotted
    step is fe_step_pool's (BSRNN, FSPEN, LiSenNet), step_slots for FastEnhancer - its own path as it has always been called - and for an
    engine object without a family description."""
    fam = _FAMILIES.get(type(getattr(engine, "cfg", None)))
    return engine.step_pool if fam is not None and fam.pool else engine.step_slots


def packet_step(engine, pinned: bool) -> Callable:
    """The engine's call for one packet step of a state buffer's streams (PacketPool.tick): step_pool_streams[_pinned] for the families whose
    slotted steps are fe_step_pool's (BSRNN, FSPEN, LiSenNet), step_streams[_pinned] for FastEnhancer - its own path as it has always been
    called - and for an engine object without a family description."""
    fam = _FAMILIES.get(type(getattr(engine, "cfg", None)))
    if fam is not None and fam.pool:
        return engine.step_pool_streams_pinned if pinned else engine.step_pool_streams
    return engine.step_streams_pinned if pinned else engine.step_streams


def packet_ctl_step(engine, pinned: bool) -> Callable:
    """The engine's call for one packet step with a suppression limit or level meters (FamilyPacketPool.tick, when either control is in use):
    step_pool_streams_ctl[_pinned] for BSRNN, FSPEN and LiSenNet, step_streams[_pinned] - which takes min_gain= and levels= itself - for
    FastEnhancer and for an engine object without a family description."""
    fam = _FAMILIES.get(type(getattr(engine, "cfg", None)))
    if fam is not None and fam.pool:
        return engine.step_pool_streams_ctl_pinned if pinned else engine.step_pool_streams_ctl
    return engine.step_streams_pinned if pinned else engine.step_streams


def packet_chunk_step(engine, pinned: bool) -> Callable:
    """The engine's call for a packet step whose streams come with a backlog, each stream's hops on the time pipeline
    (BacklogPacketPool.tick's second launch): step_pool_streams_chunk[_pinned] for BSRNN, FSPEN and LiSenNet - min_gain=, levels= and work=, no
    bank table - and step_streams_chunk[_pinned] for FastEnhancer and for an engine object without a family description."""
    fam = _FAMILIES.get(type(getattr(engine, "cfg", None)))
    if fam is not None and fam.pool:
        return engine.step_pool_streams_chunk_pinned if pinned else engine.step_pool_streams_chunk
    return engine.step_streams_chunk_pinned if pinned else engine.step_streams_chunk


def packet_chunk_on_request(engine) -> bool:
    """Whether that call runs pipelined only because the engine was asked to: a family whose pipeline carries the streaming state on request
    (LiSenNet) after Engine.set_time_pipeline(P >= 2) - the scratch is then Engine.lisennet_pool_streams_chunk_work_floats(n, T_max)."""
    fam = _FAMILIES.get(type(getattr(engine, "cfg", None)))
    return fam is not None and fam.backlog_on_request and getattr(engine, "_time_pipeline", -1) >= 2


def pool_family_name(engine) -> Optional[str]:
    """"BSRNN", "FSPEN" or "LiSenNet" for an engine of a family that steps through fe_step_pool / fe_step_pool_streams, else None: what a
    pool names when it refuses a control that is FastEnhancer's (suppression limit, level meters, weight banks, the pipelined packet step)."""
    cfg = getattr(engine, "cfg", None)
    fam = _FAMILIES.get(type(cfg))
    return type(cfg).__name__[:-len("Config")] if fam is not None and fam.pool else None
