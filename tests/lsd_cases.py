"""The float64 statement of the LSD metric's definition (include/fsem_lsd.h, the reference's
LSD.py:32-52) and the seeded cases of tests/test_lsd_cpu.py and tests/test_lsd_gpu.py.

``expected`` is written from the definition, one row and one frame at a time in numpy float64 with
``np.fft.rfft``; it shares no code with the package's CPU mode (``_cpu.lsd``) or with the engine.
"""
import math
import os

import numpy as np
import torch

from fast_speech_enhancement_metrics_amd.synthetic import speech_like_pairs

# The reference's own test tolerance (pytest.approx(..., 1e-5) in its test_lsd.py).
RTOL = 1e-5
# For values near zero: a float32 ratio within a few ulp of 1 has a logarithm of the order of
# 16 * 2^-24 = 1e-6.
ATOL = 2e-6
# Both bounds hold for the reference's float32 formulation itself on full-band 16 kHz rows (measured
# on the CPU: within 3.1e-6 relative of `expected` on 4-row speech-like batches of 48000, 30001, 700
# and 255 samples, also at x32768; within 3.3e-7 absolute on identical and gain rows).

# The 8 kHz drop-in call against the reference's LSD(8000) scores (tests/golden/lsd_8k.npz).
# Measured on the CPU mode: worst |LSD(8000, use_gpu=False) - golden| / golden over the four rows
# = 1.15e-4 (MEASURED_8K; the rows: 5.9e-5, 6.4e-5, 1.15e-4, 1.4e-5); the tests allow four times
# that, 4.6e-4 (RTOL_8K).  The deviation is not the resamplers': the reference's float32 operations
# applied to the rows THIS package resamples reproduce the golden scores digit for digit.  It is
# the reference's float32 STFT: rows resampled from 8 kHz have an upper half-spectrum ~100 dB below
# the frame's peak, the log ratio weighs those bins like any other, and a float32 transform's
# rounding (1e-7 of the peak) is a tenth of such a bin.  The package (CPU mode and engine) computes
# the transform in float64 and stays within RTOL of `expected` on these rows.
MEASURED_8K = 1.15e-4
RTOL_8K = 4 * MEASURED_8K

LN1E8 = math.log(1e8)  # 18.420680743952367: a silent clean row, or a row of no samples
LENGTHS = (48000, 30001, 700, 255)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

_W = np.array([0.5 * (1.0 - math.cos(2.0 * math.pi * t / 512.0)) for t in range(512)])


def expected_row(s, h) -> float:
    """LSD of one unpadded row pair, float64."""
    s = np.asarray(s, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n = s.shape[0]
    if not (np.isfinite(s).all() and np.isfinite(h).all()):
        return float("nan")
    a = float(np.sum(s * h)) / (float(np.sum(h * h)) + 1e-8)
    sp = np.concatenate([np.zeros(256), s, np.zeros(512)])
    hp = np.concatenate([np.zeros(256), a * h, np.zeros(512)])
    F = 1 + n // 256
    acc = 0.0
    for f in range(F):
        S = np.abs(np.fft.rfft(_W * sp[256 * f:256 * f + 512]))
        H = np.abs(np.fft.rfft(_W * hp[256 * f:256 * f + 512]))
        with np.errstate(over="ignore"):
            t = np.log(S ** 2 / (H + 1e-8) ** 2 + 1e-8)
        acc += math.sqrt(float(np.sum(t * t)) / 257.0)
    return acc / F


def _np(x):
    return np.asarray(x.detach().cpu()) if isinstance(x, torch.Tensor) else np.asarray(x)


def expected(clean, noisy, lengths=None) -> np.ndarray:
    """[B] float64 LSD of the rows' first lengths[b] samples."""
    c, n = np.atleast_2d(_np(clean)), np.atleast_2d(_np(noisy))
    lens = [c.shape[1]] * c.shape[0] if lengths is None else [int(v) for v in _np(lengths)]
    return np.array([expected_row(c[b, :lens[b]], n[b, :lens[b]]) for b in range(c.shape[0])])


def assert_close(got, want, what: str = "", rtol: float = RTOL, atol: float = ATOL):
    """got: [B] tensor / array / list of dicts; want: ``expected``'s [B].  NaN positions match
    exactly; elsewhere |got - want| <= atol + rtol |want|.  Prints the worst error."""
    if isinstance(got, list):
        got = [r["LSD"] for r in got]
    g = np.asarray(_np(got), dtype=np.float64).reshape(-1)
    w = np.asarray(want, dtype=np.float64).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: NaN positions")
    ok = ~np.isnan(w)
    assert np.isfinite(g[ok]).all(), (what, g, w)
    err = np.abs(g[ok] - w[ok])
    rel = err / np.maximum(np.abs(w[ok]), 1e-300)
    over = err - (atol + rtol * np.abs(w[ok]))
    print(f"{what}: worst |got - expected| = {err.max() if ok.any() else 0.0:.3e} absolute, "
          f"{rel.max() if ok.any() else 0.0:.3e} relative over {int(ok.sum())} rows")
    assert (over <= 0).all(), (what, g, w, err)


def speech_rows(batch: int, length: int, seed: int = 11, sr: int = 16000, snr_high: float = 40.0):
    c, n, _ = speech_like_pairs(batch, length, sr, seed=seed, snr_low=-5, snr_high=snr_high)
    return c, n


GAIN_CASES = [(0.3, -60.0), (0.3, -80.0), (1.0, -90.0)]


def gain_batch():
    """[3, 48000] clean / estimate float32 rows, as sdr_cases.gain_batch: y = g x + g rms(x)
    10^(dB / 20) r on row 0 of speech_like_pairs(4, 48000, 16000, seed=11, snr_low=-5, snr_high=30),
    r = the cases' successive float32 randn draws of one generator seeded with 3."""
    c, _, _ = speech_like_pairs(4, 48000, 16000, seed=11, snr_low=-5, snr_high=30.0)
    x = c[0].double()
    gen = torch.Generator().manual_seed(3)
    ys = []
    for g, db in GAIN_CASES:
        r = torch.randn(x.shape[0], generator=gen).double()
        ys.append((g * x + g * x.square().mean().sqrt() * 10 ** (db / 20) * r).float())
    return torch.stack([x.float()] * len(ys)), torch.stack(ys)


EDGE_NAMES = ("identical", "silent clean", "silent estimate", "both silent", "gain -0.5", "gain 3")


def edge_rows(n: int = 2000, seed: int = 5):
    """[6, n] pairs in EDGE_NAMES' order."""
    gen = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(n, generator=gen)
    y = 0.1 * torch.randn(n, generator=gen)
    z = torch.zeros(n)
    return torch.stack([x, z, x, z, x, x]), torch.stack([x, y, z, z, -0.5 * x, 3 * x])


def golden(name: str):
    """(clean, noisy float32 rows rebuilt from the stored int16 codes, sample rate, the reference's scores)."""
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        c = torch.from_numpy(z["clean"].astype(np.float32) / 32768.0)
        n = torch.from_numpy(z["noisy"].astype(np.float32) / 32768.0)
        return c, n, int(z["sample_rate"]), z["lsd"].astype(np.float64)
