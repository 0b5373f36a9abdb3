"""Host-side mirror of ``models.lisennet.model`` of the reference (models/lisennet/model.py): ``ONNXModel`` (streaming, spec -> spec
with 1 + 3 + 2 n_blocks + 1 caches) and ``Model`` (offline wav -> wav), built from the yaml ``model_kwargs``
(configs/others/lisennet.yaml).  All arithmetic runs in libfastenhancer_hip.so (lisennet_frame_kernel); inference only."""
from __future__ import annotations

from ...config import LiSenNetConfig
from .._mirror import OfflineMirror, StreamingMirror


class ONNXModel(StreamingMirror):
    """get_stft: models/lisennet/model.py:342-349; initialize_cache: :380-396; forward: :434-474."""

    def __init__(self, **model_kwargs):
        super().__init__(LiSenNetConfig.from_model_kwargs(**model_kwargs))
        self.n_freqs = self.cfg.n_fft // 2 + 1

    def remove_weight_reparameterizations(self):
        """models/lisennet/model.py:476-477: nothing to remove"""


class Model(OfflineMirror, ONNXModel):
    """Offline wav -> wav (models/lisennet/model.py:480-531): forward(noisy) -> (wav_hat, spec_hat [B, 257, T, 2]); its CompressedSTFT
    keeps all 257 bins (:481-489).
    NB its phase features take `current - previous` (torch.diff) where ONNXModel takes `previous - current`; the kernel follows
    each, as the reference does."""
