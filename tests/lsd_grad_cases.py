"""The float64 statement of the LSD gradient (include/fsem.h, "LSD with gradients") and the seeded cases of
tests/test_lsd_grad_cpu.py and tests/test_lsd_grad_gpu.py.

``expected_row`` extends ``lsd_cases.expected_row``: the same definition, one row and one frame at a time in
numpy float64 with ``np.fft``, and the closed-form gradient with respect to the estimate beside the score.  It
shares no code with the package's CPU mode (``_cpu.lsd64`` under torch's autograd) or with the engine.  For
rows at another rate the expected gradient is the statement's 16 kHz gradient pulled back through
``_cpu.resample64`` by ``torch.autograd.grad`` in float64.

A row's error is max|g - g_ref| / max|g_ref|.

The bar of the engine tests is BAR = 4 x MEASURED (the convention of ``lsd_cases.RTOL_8K``), MEASURED being the
engine's worst row error over the parity cases (both incoming gradients) on an MI355X; the resampler's
transpose alone has its own pair.  Both bars must stay at or below BAR_LIMIT = 1e-5 -- about 170 float32
roundings of the row's largest element, where the double chain itself sits at 1e-12 and the output is float32;
a bar above it means a stage runs in float32 that should not.
"""
import functools
import math

import numpy as np
import torch

from fast_speech_enhancement_metrics_amd import _cpu, _native

from . import lsd_cases as lc

BAR_LIMIT = 1e-5
# Measured on an MI355X (tests/test_lsd_grad_gpu.py prints each case's row errors): the engine's worst row
# error over the five parity cases, both incoming gradients -- edges 5.50e-8, speech 4.93e-8, gain 5.30e-8,
# 8k 4.99e-8 (rows 2.89e-8, 4.99e-8, 3.05e-8, 3.45e-8; random incoming 4.06e-8), 48k 5.34e-8 (rows 5.34e-8,
# 3.18e-8, 3.01e-8; random incoming 4.62e-8): one float32 rounding of the row's largest element.
# The 8k and 48k rows go through fsem_lsd_grad_rate_f32, which resamples in double and differentiates at those
# rows.  At the float32 16 kHz rows the forward resampler stores, the same statement is 1.75e-2, 5.80e-3,
# 6.44e-3, 8.74e-3 (8k) and 7.5e-6, 5.7e-6, 4.5e-4 (48k) away from the expected gradient: the upper half-spectrum
# of such rows lies 100 dB below the frame's peak, where 1e-7 of the peak is a tenth of the bin.
MEASURED = 5.5e-8
BAR = 4 * MEASURED
# The transposed resampler alone (3 rows, lengths 1, 999, 3000): 8000 -> 16000 rows 3.34e-9, 3.26e-8, 5.00e-8;
# 48000 -> 16000 rows 5.90e-11, 2.92e-8, 4.22e-8.
MEASURED_RESAMPLE = 5.0e-8
BAR_RESAMPLE = 4 * MEASURED_RESAMPLE
RTOL_CPU = 1e-9   # CPU mode against the statement: both are float64

PARITY = ("edges", "speech", "gain", "8k", "48k")

_W = np.array([0.5 * (1.0 - math.cos(2.0 * math.pi * t / 512.0)) for t in range(512)])


def expected_row(s, h):
    """(LSD, d LSD / d h [n]) of one unpadded 16 kHz row pair, float64; (NaN, zeros) for a non-finite sample."""
    s = np.asarray(s, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n = s.shape[0]
    if not (np.isfinite(s).all() and np.isfinite(h).all()):
        return float("nan"), np.zeros(n)
    sh, hh = float(np.sum(s * h)), float(np.sum(h * h))
    a = sh / (hh + 1e-8)
    sp = np.concatenate([np.zeros(256), s, np.zeros(512)])
    yp = np.concatenate([np.zeros(256), a * h, np.zeros(512)])
    ybar = np.zeros_like(yp)
    F = 1 + n // 256
    acc = 0.0
    for f in range(F):
        S = np.abs(np.fft.rfft(_W * sp[256 * f:256 * f + 512]))
        Hc = np.fft.rfft(_W * yp[256 * f:256 * f + 512])
        H = np.abs(Hc)
        q = S ** 2 / (H + 1e-8) ** 2
        t = np.log(q + 1e-8)
        v = math.sqrt(float(np.sum(t * t)) / 257.0)
        acc += v
        if v == 0.0:
            continue   # a frame with v = 0 contributes 0
        dH = t / (257.0 * v * F) * (-2.0 * q / ((H + 1e-8) * (q + 1e-8)))
        G = np.where(H > 0, dH * Hc / np.where(H > 0, H, 1.0), 0.0)   # |H| = 0: the subgradient 0
        # Re sum_{k <= 256} G_k e^{+2 pi i k t / 512}: the unnormalised inverse of G zero-extended to 512 bins
        xbar = np.real(np.fft.ifft(np.concatenate([G, np.zeros(255)]))) * 512.0
        ybar[256 * f:256 * f + 512] += _W * xbar
    yb = ybar[256:256 + n]
    D = float(np.sum(yb * h))
    return acc / F, a * yb + D * (s - 2.0 * a * h) / (hh + 1e-8)


def row_errors(got, want) -> np.ndarray:
    """[B] max|g - g_ref| / max|g_ref| per row (0 where both rows are all zero)."""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(w).max(axis=1)
    diff = np.abs(g - w).max(axis=1)
    return np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), diff)


def incoming(batch: int) -> torch.Tensor:
    """The seeded random incoming gradient [B] (float32, 0.5 .. 1.5 in magnitude, both signs)."""
    gen = torch.Generator().manual_seed(29)
    u = torch.rand(batch, generator=gen) + 0.5
    return torch.where(torch.rand(batch, generator=gen) < 0.5, -u, u)


def chunk() -> int:
    return int(_native.load_lsd().fsem_lsd_chunk())


@functools.lru_cache(maxsize=None)
def rows(name: str):
    """(clean, noisy [B, L] float32 host rows, their rate, lengths or None) of a named case; for ``edges`` the
    memory past each length holds NaN (clean) and 1e30 (estimate)."""
    if name == "edges":
        C = chunk()
        lens = [255, 256, 257, 511, 512, 513, 4095, 4096, 4097, C - 1, C, C + 1, C + 255, C + 256, 2 * C + 257]
        c, n = lc.speech_rows(len(lens), 2 * C + 257, seed=17)
        c, n = c.clone(), n.clone()
        for b, k in enumerate(lens):
            c[b, k:] = float("nan")
            n[b, k:] = 1e30
        return c, n, 16000, tuple(lens)
    if name == "speech":
        c, n = lc.speech_rows(4, 16000, seed=22)
        return c, n, 16000, None
    if name == "gain":
        c, n = lc.gain_batch()
        return c[:, :4000].contiguous(), n[:, :4000].contiguous(), 16000, None
    if name == "8k":
        c, n, sr, _ = lc.golden("lsd_8k")
        assert sr == 8000
        return c, n, sr, None
    if name == "48k":
        c, n = lc.speech_rows(3, 9000, seed=23, sr=48000)
        return c, n, 48000, None
    raise KeyError(name)


def expected_for(c, n, sr: int, lens=None):
    """(lsd [B], gradient [B, L]) float64 of host rows at rate sr for incoming gradients all one: per row the
    statement on the row's first lens[b] samples (resampled to 16 kHz in float64 for other rates, the gradient
    pulled back through that resampler); zeros past each length."""
    B, L = c.shape
    lens = [L] * B if lens is None else list(lens)
    score, grad = np.zeros(B), np.zeros((B, L))
    for b in range(B):
        k = lens[b]
        if sr == 16000:
            score[b], grad[b, :k] = expected_row(c[b, :k].numpy(), n[b, :k].numpy())
            continue
        x = n[b:b + 1, :k].double().requires_grad_(True)
        y16 = _cpu.resample64(x, sr, 16000)
        c16 = _cpu.resample64(c[b:b + 1, :k], sr, 16000)
        score[b], g16 = expected_row(c16[0].numpy(), y16[0].detach().numpy())
        grad[b, :k] = torch.autograd.grad(y16, x, grad_outputs=torch.from_numpy(g16)[None])[0][0].numpy()
    return score, grad


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """``expected_for`` a named case."""
    c, n, sr, lens = rows(name)
    return expected_for(c, n, sr, lens)


@functools.lru_cache(maxsize=None)
def rate_rows(sr: int):
    """(clean, noisy [4, L] float32 host rows at rate sr, lengths) for the other-rate backward: 0.3 s rows with
    lengths L, L // 2 + 1, 257 and 1; the memory past each length holds NaN (clean) and 1e30 (estimate)."""
    L = 3 * sr // 10
    lens = (L, L // 2 + 1, 257, 1)
    c, n = lc.speech_rows(4, L, seed=37, sr=sr)
    c, n = c.clone(), n.clone()
    for b, k in enumerate(lens):
        c[b, k:] = float("nan")
        n[b, k:] = 1e30
    return c, n, lens


def float32_autograd(name: str) -> np.ndarray:
    """[B] row errors of the yardstick: the same definition under torch autograd in float32 (printed, never
    asserted: 4e-8 .. 5e-4 on speech rows, a few per cent on the gain rows and on rows resampled from 8 kHz)."""
    c, n, sr, lens = rows(name)
    B, L = c.shape
    lens = [L] * B if lens is None else list(lens)
    got = np.zeros((B, L))
    w = torch.hann_window(512)
    for b in range(B):
        k = lens[b]
        x = n[b:b + 1, :k].clone().requires_grad_(True)
        s, h = c[b:b + 1, :k], x
        if sr != 16000:
            from fast_speech_enhancement_metrics_amd.resample import Resample
            rs = Resample(sr, 16000)
            s, h = rs(s), rs(h)
        a = (s * h).sum(1, keepdim=True) / (h.square().sum(1, keepdim=True) + 1e-8)
        S = torch.stft(s, 512, 256, window=w, center=True, pad_mode="constant", return_complex=True).abs()
        H = torch.stft(a * h, 512, 256, window=w, center=True, pad_mode="constant", return_complex=True).abs()
        v = torch.log(S.square() / (H + 1e-8).square() + 1e-8).square().mean(1).sqrt().mean(1)
        got[b, :k] = torch.autograd.grad(v.sum(), x)[0][0].double().numpy()
    return row_errors(got, expected(name)[1])
