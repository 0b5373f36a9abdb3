"""Host-side mirror of ``models.fspen.model`` of the reference (models/fspen/model.py): ``ONNXModel`` (streaming, spec -> spec
with num_blocks * groups inter-GRU caches) and ``Model`` (offline wav -> wav), built from the yaml ``model_kwargs``
(configs/others/fspen.yaml).  All arithmetic runs in libfastenhancer_hip.so (fspen_frame_kernel); inference only."""
from __future__ import annotations

from ...config import FSPENConfig
from .._mirror import OfflineMirror, StreamingMirror


class ONNXModel(StreamingMirror):
    """get_stft: models/fspen/model.py:279-286; initialize_cache: :293-297 (-> :111-116); forward: :409-429."""

    def __init__(self, **model_kwargs):
        super().__init__(FSPENConfig.from_model_kwargs(**model_kwargs))


class Model(OfflineMirror, ONNXModel):
    """Offline wav -> wav (models/fspen/model.py:432-449): forward(noisy) -> (wav_hat, spec_hat [B, 257, T, 2]); its CompressedSTFT
    keeps all 257 bins (:433-441)."""
