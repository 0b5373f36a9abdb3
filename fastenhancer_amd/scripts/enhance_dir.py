#!/usr/bin/env python3
"""scripts/test_offline.py with one more flag: --resample takes files that are not at the model's rate - each is read at its own rate,
resampled to the model's on the GPU (fastenhancer_amd.resample.Resampler: the polyphase filter of scipy.signal.resample_poly), enhanced and
written at the model's rate, as the reference's caller writes what librosa.load(path, sr=model_rate) gave it.  Off by default: without the
flag this IS test_offline.py (same flags, same loops, same output), which refuses such a file.

    python -m fastenhancer_amd.scripts.enhance_dir -n fastenhancer_b -i noisy_dir_48k -o enhanced/dns --resample
"""
from __future__ import annotations

from . import test_offline
from .common import resampling, split_resample_flag


def main(argv=None):
    resample_on, rest = split_resample_flag(argv)
    with resampling(resample_on):
        return test_offline.main(rest)


if __name__ == "__main__":
    main()
