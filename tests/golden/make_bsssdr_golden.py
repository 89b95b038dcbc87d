"""Generate the BSSSDR fixtures in tests/golden/ by running the REFERENCE's own SDR class.

Run in the build container only (it reads /root/reference, as make_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bsssdr_golden.py

The reference package imports torchaudio (``base.py:2``), which ``oracle/ta_shim`` stands in for;
``fast_se_metrics/SDR.py`` is the reference's own code, executed unmodified.  Only inputs (int16
codes), flags and outputs are stored: data, not source.

Every row is scored ALONE (a batch of one).  The reference solves its 512 x 512 Toeplitz system by a
float32 Cholesky factorisation and falls back to ``torch.linalg.solve`` for the whole batch when
that fails -- which it does on some speech-like rows, and the fallback does not return on every
torch build.  So each row first goes through the reference's own ``preprocess_speech`` and
``_compute_autocorr_crosscorr`` and ``torch.linalg.cholesky_ex``; only a row with ``info == 0`` is
given to the reference's ``SDR(sr)(clean_row, noisy_row)``, under a time limit.  The others are
stored with ``has_ref`` False and no score.

    bsssdr_16k.npz    8 x 32000 speech-like rows at 16 kHz, SNR -5 ... 40 dB
    bsssdr_8k.npz     4 x 16000 speech-like rows at 8 kHz (the reference's resampler first)
    bsssdr_white.npz  16000-sample rows at 16 kHz: 4 white rows plus white noise at 0, -10, -30 and
                      -50 dB, an identical pair, a silent denoised row

Stored per file: clean, noisy (int16 codes), sample_rate, info (the factorisation's), has_ref,
sdr (the reference's score, NaN without one), ref_minus_definition (sdr minus the float64 definition
of tests/bsssdr_cases.py on the 16 kHz rows this package scores -- for 8 kHz input the rows this
package's resampler makes), definition (that float64 score), ref_ok (has_ref and
|ref_minus_definition| <= 1e-2 dB; where |definition| > 60 dB: the same sign and a magnitude >= 60 dB).
Condition (asserted): at least half of the speech-like rows and all white rows carry a score.
"""
from __future__ import annotations

import os
import signal
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

from fast_speech_enhancement_metrics_amd.BSSSDR import BSSSDR  # noqa: E402
from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs, to_int16  # noqa: E402

# tests/bsssdr_cases.py by its path (the reference has a `tests` package of its own on sys.path)
import importlib.util  # noqa: E402
_spec = importlib.util.spec_from_file_location("bsssdr_cases", os.path.join(REPO, "tests", "bsssdr_cases.py"))
bc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bc)

import fast_se_metrics.SDR  # noqa: E402,F401  (the reference, via sys.path)

# the reference's __init__ rebinds fast_se_metrics.SDR to the class: the module is in sys.modules
ref_mod = sys.modules["fast_se_metrics.SDR"]
assert "reference" in ref_mod.__file__, "must import the reference"
RefSDR = ref_mod.SDR
TIME_LIMIT_S = 120


class _Timeout(Exception):
    pass


def _alarm(signum, frame):
    raise _Timeout()


def reference_row(c: torch.Tensor, n: torch.Tensor, sr: int):
    """(info of the float32 factorisation, the reference's score or NaN) of one row pair, alone."""
    m = RefSDR(sample_rate=sr, use_gpu=False)
    cp, npp = m.prepare_inputs(c[None], n[None])
    r0, b = ref_mod._compute_autocorr_crosscorr(m.preprocess_speech(cp), m.preprocess_speech(npp), m.filter_length)
    idx = (torch.arange(512)[None] - torch.arange(512)[:, None]).abs()
    info = int(torch.linalg.cholesky_ex(r0.to(torch.float32)[..., idx]).info.reshape(-1)[0])
    if info != 0:
        return info, float("nan")
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(TIME_LIMIT_S)
    try:
        return info, float(m(c[None], n[None])[0]["SDR"])
    except _Timeout:
        return -1, float("nan")
    finally:
        signal.alarm(0)


def store(name: str, codes_c: np.ndarray, codes_n: np.ndarray, sr: int) -> np.ndarray:
    # the rows the tests rebuild from the stored codes
    c = torch.from_numpy(codes_c.astype(np.float32) / 32768.0)
    n = torch.from_numpy(codes_n.astype(np.float32) / 32768.0)
    res = [reference_row(c[b], n[b], sr) for b in range(c.shape[0])]
    info = np.array([r[0] for r in res], dtype=np.int64)
    sdr = np.array([r[1] for r in res], dtype=np.float64)
    has_ref = np.isfinite(sdr)
    c16, n16 = BSSSDR(sr, use_gpu=False).prepare_inputs(c, n)
    want, _ = bc.expected(c16, n16)
    diff = np.where(has_ref, sdr - want, np.nan)
    high = np.abs(want) > bc.HIGH_DB  # (beyond it the bar is the sign and a magnitude >= HIGH_DB)
    near = np.where(high, (np.sign(sdr) == np.sign(want)) & (np.abs(sdr) >= bc.HIGH_DB),
                    np.abs(np.nan_to_num(diff, nan=np.inf)) <= bc.REF_CAP_DB)
    ref_ok = has_ref & near
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), clean=codes_c, noisy=codes_n, sample_rate=sr, info=info,
                        has_ref=has_ref, sdr=sdr, definition=want, ref_minus_definition=diff, ref_ok=ref_ok)
    print(name, "info", info, "\n  reference", sdr, "\n  definition", want, "\n  reference - definition", diff,
          "\n  ref_ok", ref_ok)
    return has_ref


def speech_case(name: str, batch: int, length: int, sr: int, seed: int):
    clean, noisy, _ = speech_like_pairs(batch, length, sr, seed=seed, snr_low=-5.0, snr_high=40.0)
    has_ref = store(name, to_int16(clean).numpy(), to_int16(noisy).numpy(), sr)
    assert 2 * int(has_ref.sum()) >= batch, f"{name}: fewer than half of the rows carry a reference score"


def white_case(name: str, length: int = 16000, seed: int = 43):
    c, n = bc.white_rows(4, length, seed=seed)
    quant = lambda x: torch.round(x.clamp(-1, 32767 / 32768) * 32768.0).to(torch.int16).numpy()  # noqa: E731
    cc, nn = quant(c), quant(n)
    cc = np.concatenate([cc, cc[:1], cc[1:2]])
    nn = np.concatenate([nn, cc[:1], np.zeros_like(cc[:1])])  # an identical pair, a silent denoised row
    has_ref = store(name, cc, nn, 16000)
    assert has_ref[:4].all(), f"{name}: a white row without a reference score"


if __name__ == "__main__":
    torch.set_num_threads(8)
    speech_case("bsssdr_16k", batch=8, length=32000, sr=16000, seed=41)
    speech_case("bsssdr_8k", batch=4, length=16000, sr=8000, seed=42)
    white_case("bsssdr_white")
