"""What the host-side mirrors of the reference's model modules share: the nn.Module-like plumbing around one config, one checkpoint
and one lazily created Engine.  ``StreamingMirror`` is the base of every ``ONNXModel`` (streaming, spec -> spec, caches threaded by
the caller), ``OfflineMirror`` of every ``Model`` (offline wav -> wav).  Whatever differs between the families comes from the
config's family description (fastenhancer_amd/family.py); a model.py adds its constructor, its docstrings and the attributes its
reference module exposes.

All arithmetic runs in libfastenhancer_hip.so on the GPU the model was moved to; these classes only hold the checkpoint and marshal
torch tensors across the C ABI.  They are inference-only (``.eval()``; no autograd, no training forward)."""
from __future__ import annotations

import typing as tp

import torch
from torch import Tensor

from ..engine import Engine
from ..family import family_of
from ..stft import CompressedSTFT, ONNXSTFT


class StreamingMirror:
    def __init__(self, cfg):
        self.cfg = cfg
        self.family = family_of(cfg)
        self.input_compression = cfg.input_compression
        self.stft = self.get_stft()
        self.device = torch.device("cpu")
        self._sd: tp.Dict[str, Tensor] = self.family.default_state_dict(cfg)
        self._engine: tp.Optional[Engine] = None
        self.training = False

    def get_stft(self):
        """the streaming model carries an ONNXSTFT"""
        return ONNXSTFT(self, self.cfg)

    # ---- nn.Module-like plumbing -----------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("fastenhancer_amd models are inference-only")
        return self

    def to(self, device):
        self.device = torch.device(device)
        self._engine = None
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def state_dict(self) -> tp.Dict[str, Tensor]:
        return dict(self._sd)

    def load_state_dict(self, state_dict: tp.Mapping[str, Tensor], strict: bool = True):
        self.family.check(self.family.fold(state_dict, self.cfg), self.cfg, strict=strict)
        self._sd = {k: torch.as_tensor(v).detach().clone() for k, v in state_dict.items()}
        self._engine = None
        return self

    def remove_weight_reparameterizations(self):
        """Folding happens when the blob is built; make it visible in state_dict()."""
        self._sd = self.family.fold(self._sd, self.cfg)

    def flatten_parameters(self):
        pass

    def parameters(self):
        return iter(self._sd.values())

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            eng = Engine(self.cfg, self.device)
            eng.load_state_dict(self._sd)     # raises without a GPU: no CPU fallback
            self._engine = eng
        return self._engine

    # ---- reference API ---------------------------------------------------------------------
    def initialize_cache(self, x: Tensor) -> tp.List[Tensor]:
        """the model's cache list, zeros, sized for the B = x.size(0) streams of the batch (b-major)"""
        return [torch.zeros(*s, dtype=torch.float32, device=x.device) for s in self.cfg.cache_shapes(x.size(0))]

    def forward(self, spec_noisy: Tensor, *args: Tensor):
        """input/output: [B, n_fft//2+1, T_spec, 2], any T >= 1; returns (spec_hat, *cache_out), the caches as views of one buffer
        allocated for this call.  Functional like the reference: the caches passed in are not modified.  Without caches the model
        starts from its zero state."""
        B = spec_noisy.size(0)
        cfg, fam, eng = self.cfg, self.family, self.engine
        if len(args) == 0:
            h = torch.zeros(eng.model_state_floats(B), dtype=torch.float32, device=eng.device)
            fam.start(cfg, h, B)
        else:
            n_caches = len(cfg.cache_shapes(B))
            assert len(args) == n_caches, f"expected {n_caches} caches, got {len(args)}"
            h = torch.cat([t.to(eng.device, torch.float32) for t in fam.order(cfg, list(args))]).contiguous()
        spec_hat = eng.spec_step(spec_noisy.to(eng.device).contiguous().float(), h)
        return (spec_hat, *fam.split(cfg, h, B))

    __call__ = forward


class OfflineMirror(StreamingMirror):
    """forward(noisy [B, T_wav]) -> (wav_hat [B, H*(Tw//H)], spec_hat [B, F, T, 2]), F = the family's spec_bins."""

    def get_stft(self):
        """CompressedSTFT(compression=input_compression, discard_last_freq_bin = the family's spectrum has no Nyquist bin)"""
        return CompressedSTFT(self, self.cfg, discard_last_freq_bin=not self.family.nyquist)

    def forward(self, noisy: Tensor):
        """One fused launch sequence (fe_offline): centered STFT, all T frames, envelope-normalised overlap-add.  ``self.stft`` /
        ``self.stft.inverse`` give the front / back end alone."""
        if isinstance(noisy, (list, tuple)):      # utterances of different lengths, one batched call: (list of wavs, list of specs)
            return self.engine.offline_ragged(list(noisy))
        return self.engine.offline(noisy.to(self.engine.device))

    __call__ = forward
