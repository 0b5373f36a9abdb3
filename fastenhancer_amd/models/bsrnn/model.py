"""Host-side mirror of ``models.bsrnn.model`` of the reference (models/bsrnn/model.py): ``ONNXModel`` (streaming,
spec -> spec with 2*num_layers LSTM caches) and ``Model`` (offline wav -> wav), built from the yaml ``model_kwargs``.
All arithmetic runs in libfastenhancer_hip.so (bsrnn_frame_kernel); inference only."""
from __future__ import annotations

from ...config import BSRNNConfig
from .._mirror import OfflineMirror, StreamingMirror


class ONNXModel(StreamingMirror):
    """get_stft: models/bsrnn/model.py:323-329; initialize_cache: :409-416 (onnx form); forward: :418-448 - unlike the reference's
    LSTMCell path (T=1 only), any T >= 1 is accepted."""

    def __init__(self, **model_kwargs):
        super().__init__(BSRNNConfig.from_model_kwargs(**model_kwargs))
        self.num_layers = self.cfg.num_layers


class Model(OfflineMirror, ONNXModel):
    """Offline wav -> wav (models/bsrnn/model.py:463-483): forward(noisy) -> (wav_hat, spec_hat [B, 257, T, 2]); its CompressedSTFT
    keeps all 257 bins (:467-475)."""
