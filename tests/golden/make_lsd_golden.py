"""Generate the LSD fixtures in tests/golden/ by running the REFERENCE's own LSD class.

Run in the build container only (it reads /root/reference, as make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lsd_golden.py

The reference package imports torchaudio (``base.py:2``), which ``oracle/ta_shim`` stands in for;
``fast_se_metrics/LSD.py`` is the reference's own code, executed unmodified.  Only inputs (int16
codes) and outputs are stored: data, not source.

    lsd_16k.npz  4 x 48000 rows at 16 kHz, SNR -5 ... 40 dB, scored by the reference's LSD(16000)
    lsd_8k.npz   4 x 24000 rows at 8 kHz, scored by the reference's LSD(8000) (its resampler first)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REFERENCE = "/root/reference"

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle", "ta_shim"))
sys.path.insert(1, REFERENCE)
sys.dont_write_bytecode = True

from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs, to_int16  # noqa: E402

from fast_se_metrics.LSD import LSD as RefLSD  # noqa: E402  (the reference, via sys.path)

assert "reference" in sys.modules["fast_se_metrics.LSD"].__file__, "must import the reference"


def lsd_case(name: str, batch: int, length: int, sr: int, seed: int, snr=(-5.0, 40.0)):
    clean, noisy, snr_v = speech_like_pairs(batch, length, sr, seed=seed, snr_low=snr[0], snr_high=snr[1])
    codes_c, codes_n = to_int16(clean).numpy(), to_int16(noisy).numpy()
    # the rows the tests rebuild from the stored codes
    c = torch.from_numpy(codes_c.astype(np.float32) / 32768.0)
    n = torch.from_numpy(codes_n.astype(np.float32) / 32768.0)
    m = RefLSD(sample_rate=sr, use_gpu=False)
    scores = np.array([d["LSD"] for d in m(c, n)], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), clean=codes_c, noisy=codes_n, snr=snr_v.numpy(),
                        sample_rate=sr, lsd=scores)
    print(name, snr_v.numpy(), scores)


if __name__ == "__main__":
    torch.set_num_threads(8)
    lsd_case("lsd_16k", batch=4, length=48000, sr=16000, seed=31)
    lsd_case("lsd_8k", batch=4, length=24000, sr=8000, seed=32)
