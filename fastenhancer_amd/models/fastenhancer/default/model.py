"""Host-side mirror of ``models.fastenhancer.default.model`` of the reference
(models/fastenhancer/default/model.py): the classes ``ONNXModel`` (streaming,
spec -> spec, caches threaded by the caller) and ``Model`` (offline wav -> wav),
constructed from the yaml ``model_kwargs`` verbatim, e.g.

    module = importlib.import_module(f"fastenhancer_amd.models.{hps.model}.model")
    model = module.ONNXModel(**hps.model_kwargs)            # scripts/export_onnx.py:32-35
    model.load_state_dict(ckpt["model"], strict=True)       # wrappers/ns.py:313
    model.remove_weight_reparameterizations()               # scripts/export_onnx.py:78

All arithmetic runs in libfastenhancer_hip.so on the GPU the model was moved to;
these classes only hold the checkpoint and marshal torch tensors across the C ABI.
They are inference-only (``.eval()``; no autograd, no training forward)."""
from __future__ import annotations

import typing as tp

from ....config import FEConfig
from ..._mirror import OfflineMirror, StreamingMirror


class ONNXModel(StreamingMirror):
    """get_stft: model.py:523-530; remove_weight_reparameterizations: :532-608; initialize_cache: :614-618 (time_kernel variant: + the
    causal convs' frame caches, in its order encoder / GRU / decoder - time_kernel/model.py:746-754; dptransformer variant: h_k, h_v per
    block - dptransformer/model.py:194-198, 740-744); forward: :677-710."""

    def __init__(self, _cfg: tp.Optional[FEConfig] = None, **model_kwargs):
        # (_cfg: a ready FEConfig - how the variants' mirrors, whose yaml keys differ, construct this class)
        super().__init__(_cfg if _cfg is not None else FEConfig.from_model_kwargs(**model_kwargs))
        self.rf_ch, self.rf_freq = self.cfg.rf_channels, self.cfg.rf_freq


class Model(OfflineMirror, ONNXModel):
    """Offline wav -> wav model (model.py:713-735): forward(noisy [B, T_wav]) -> (wav_hat, spec_hat [B, F0, T, 2]); its CompressedSTFT
    discards the last frequency bin (:717-726)."""
