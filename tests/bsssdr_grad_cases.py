"""The float64 statement of the BSSSDR gradient (include/fsem.h, "BSS-eval SDR with gradients") and the seeded
cases of tests/test_bsssdr_grad_cpu.py and tests/test_bsssdr_grad_gpu.py.

``expected_row`` is written from the definition, one row at a time in numpy: the float32 norms and the float32
quotients as include/fsem_bsssdr.h states them, direct ``np.correlate`` for r and b, ``np.linalg.solve`` on the
dense Toeplitz matrix, ``np.convolve`` for y, and the clamps' rules.  It shares no code with the package's CPU
mode (``_cpu.bsssdr64`` under torch's autograd, FFT correlations and a Levinson recursion) or with the engine.
For rows at another rate the expected gradient is the statement's at the float32 rows the package's resampler
gives on the host, pulled back through ``_cpu.resample64``'s transpose by ``torch.autograd.grad`` in float64.

A row's error is max|g - g_ref| / max|g_ref| (``lsd_grad_cases.row_errors``).

The bar of the engine tests is BAR = 4 x MEASURED, MEASURED being the engine's worst row error over the parity
cases (both incoming gradients) on an MI355X.  It must stay at or below BAR_LIMIT = 1e-5: the double chain should
leave about one float32 rounding, and a bar above the limit means a stage runs in float32 that should not.
RTOL_CPU, CPU mode against the statement, is set the same way from what is measured on the host, with the limit
RTOL_CPU_LIMIT = 1e-6: both are float64, but the systems' condition numbers reach 1e8 on these rows.
"""
import functools

import numpy as np
import torch

from fast_speech_enhancement_metrics_amd import _cpu, _native
from fast_speech_enhancement_metrics_amd.resample import Resample

from . import lsd_cases as lc
from .lsd_grad_cases import incoming, row_errors  # noqa: F401  (the tests take them from here)

K = 512
K10 = 10.0 / np.log(10.0)
BAR_LIMIT = 1e-5
RTOL_CPU_LIMIT = 1e-6
# Measured on an MI355X (tests/test_bsssdr_grad_gpu.py prints each case's row errors): the engine's worst row error
# over the six parity cases, incoming gradients all one / the seeded random ones -- edges 5.24e-8 / 4.71e-8, speech
# 4.87e-8 / 4.64e-8, gain 5.12e-8 / 4.02e-8, load_diag 4.24e-8 / 4.19e-8, 8k 4.71e-8 / 6.06e-8, 48k 6.70e-8 /
# 6.11e-8: one float32 rounding of the row's largest element.  The float32-autograd yardstick on the same rows:
# 2.5e-7 .. 1.2e-2 (edges), 4.5e-5 .. 9.7e-3 (speech), 7.5e-3 .. 1.3e-2 (gain), 0.81 on the one-sample 8 kHz row.
# The 8k and 48k rows are held against the statement at the float32 16 kHz rows the engine's resampler makes (the
# rows the score is taken at).  The host resampler's float32 rows differ from those in their last bits, and the
# statement there is 1.1e-6, 4.8e-6, 1.5e-4 (8k) and 5.8e-6, 1.6e-6, 2.5e-5 (48k) of the row's largest element
# away: the residual a float32 rounding of the rows leaves in the gradient, largest on the 45 dB row.
MEASURED = 6.7e-8
BAR = 4 * MEASURED
# CPU mode against the statement, measured on the host (tests/test_bsssdr_grad_cpu.py prints each case's).
# edges 4.2e-11, speech 1.9e-11, gain 3.2e-11, load_diag 1.4e-12, 8k 4.5e-10 (its one-sample row: two 16 kHz
# samples at 70 dB, 1 - coh = 1e-7; the others 2.4e-12), 48k 4.5e-12.
MEASURED_CPU = 4.5e-10
RTOL_CPU = 4 * MEASURED_CPU

PARITY = ("edges", "speech", "gain", "load_diag", "8k", "48k")
GAINS = (1e-4, 1.0, 1e4)
LOAD_DIAG = 1e-3


def quotients(s, h):
    """(s', h' float64 of the float32 quotients, nh float32, whether the estimate's norm sat below its clamp)."""
    s = np.asarray(s, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    tiny = np.float32(1e-6)
    ns = np.float32(np.sqrt(np.sum(s.astype(np.float64) ** 2)))
    nh = np.float32(np.sqrt(np.sum(h.astype(np.float64) ** 2)))
    clamped = bool(nh < tiny)
    ns, nh = max(ns, tiny), max(nh, tiny)
    return (s / ns).astype(np.float32).astype(np.float64), (h / nh).astype(np.float32).astype(np.float64), nh, clamped


def expected_row(s, h, load_diag: float = 0.0):
    """(SDR in dB, d SDR / d h [n]) of one unpadded 16 kHz row pair, float64; (NaN, zeros) for a row of no
    samples, a silent clean row and a row with a non-finite sample."""
    s = np.asarray(s, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    n = s.shape[0]
    if n == 0 or not (np.isfinite(s).all() and np.isfinite(h).all()):
        return float("nan"), np.zeros(n)
    sp, hp, nh, clamped = quotients(s, h)
    pad = np.zeros(K - 1)
    r = np.correlate(np.concatenate([sp, pad]), sp, "valid")   # r[k] = sum_t s'[t] s'[t + k], k < 512
    b = np.correlate(np.concatenate([hp, pad]), sp, "valid")   # b[k] = sum_t s'[t] h'[t + k]
    r[0] += load_diag
    if not r[0] > 0:
        return float("nan"), np.zeros(n)
    lag = np.arange(K)
    x = np.linalg.solve(r[np.abs(lag[:, None] - lag[None, :])], b)
    coh = float(b @ x)
    den = 1.0 - coh
    ratio = coh / max(den, 1e-8)
    score = 10.0 * np.log10(max(ratio, 1e-8))
    if ratio < 1e-8:
        return score, np.zeros(n)                              # the score is the constant -80
    D = K10 / coh if den < 1e-8 else K10 / (coh * den)
    y = np.convolve(sp, x)[:n]                                 # y[u] = sum_k x[k] s'[u - k]
    return score, D * (2.0 / float(nh)) * (y if clamped else y - coh * hp)


def chunk() -> int:
    return int(_native.load_bsssdr().fsem_bsssdr_chunk())


def _garbage_past(c, n, lens):
    c, n = c.clone(), n.clone()
    for b, k in enumerate(lens):
        c[b, k:] = float("nan")
        n[b, k:] = 1e30
    return c, n


@functools.lru_cache(maxsize=None)
def rows(name: str):
    """(clean, noisy [B, L] float32 host rows, their rate, lengths or None, load_diag or None) of a named case;
    where lengths are given the memory past each holds NaN (clean) and 1e30 (estimate)."""
    if name == "edges":
        C = chunk()
        lens = (1, 2, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, C - 1, C, C + 1, 2 * C + 257)
        c, n = _garbage_past(*lc.speech_rows(len(lens), 2 * C + 257, seed=17), lens)
        return c, n, 16000, lens, None
    if name in ("speech", "load_diag"):
        c, n = lc.speech_rows(4, 16000, seed=22)
        return c, n, 16000, None, LOAD_DIAG if name == "load_diag" else None
    if name == "gain":
        c, n = lc.speech_rows(1, 4000, seed=23)
        return c.repeat(3, 1), torch.cat([n * g for g in GAINS]), 16000, None, None
    if name in ("8k", "48k"):
        sr = 8000 if name == "8k" else 48000
        c, n, lens = rate_rows(sr)
        return c, n, sr, lens, None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def rate_rows(sr: int):
    """(clean, noisy [4, L] float32 host rows at rate sr, lengths): 0.3 s rows with lengths L, L // 2 + 1, 257
    and 1; the memory past each length holds NaN (clean) and 1e30 (estimate)."""
    L = 3 * sr // 10
    lens = (L, L // 2 + 1, 257, 1)
    c, n = lc.speech_rows(4, L, seed=37, sr=sr)
    return (*_garbage_past(c, n, lens), lens)


def expected_for(c, n, sr: int, lens=None, load_diag=None, resampled=None):
    """(sdr [B], gradient [B, L]) float64 of host rows at rate sr for incoming gradients all one: per row the
    statement on the row's first lens[b] samples (for other rates: on the float32 16 kHz rows made of them, the
    gradient pulled back through the float64 resampler's transpose); zeros past each length.  ``resampled``:
    (clean, noisy [B, L16] float32 host rows, their lengths), the 16 kHz rows an engine test took from the
    engine's resampler; by default the package's host resampler makes them, row by row."""
    B, L = c.shape
    lens = [L] * B if lens is None else list(lens)
    diag = 0.0 if load_diag is None else float(load_diag)
    score, grad = np.zeros(B), np.zeros((B, L))
    for b in range(B):
        k = lens[b]
        if sr == 16000:
            score[b], grad[b, :k] = expected_row(c[b, :k].numpy(), n[b, :k].numpy(), diag)
            continue
        if resampled is None:
            rs = Resample(sr, 16000)
            c16, n16 = rs(c[b, :k][None])[0], rs(n[b, :k][None])[0]
        else:
            c16, n16 = (rows16[b, :int(resampled[2][b])] for rows16 in resampled[:2])
        score[b], g16 = expected_row(c16.numpy(), n16.numpy(), diag)
        x = torch.zeros(1, k, dtype=torch.float64, requires_grad=True)   # (the resampler is linear)
        y16 = _cpu.resample64(x, sr, 16000)
        grad[b, :k] = torch.autograd.grad(y16, x, grad_outputs=torch.from_numpy(g16)[None])[0][0].numpy()
    return score, grad


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """``expected_for`` a named case."""
    c, n, sr, lens, diag = rows(name)
    return expected_for(c, n, sr, lens, diag)


def float32_autograd(name: str) -> np.ndarray:
    """[B] row errors of the yardstick: the same definition in torch operations (FFT correlations, a dense
    solve) under autograd in float32.  Printed, never asserted."""
    c, n, sr, lens, diag = rows(name)
    B, L = c.shape
    lens = [L] * B if lens is None else list(lens)
    got = np.zeros((B, L))
    lag = torch.arange(K)
    toep = (lag[:, None] - lag[None, :]).abs()
    for b in range(B):
        k = lens[b]
        x = n[b:b + 1, :k].clone().requires_grad_(True)
        s, h = c[b:b + 1, :k], x
        if sr != 16000:
            rs = Resample(sr, 16000)
            s, h = rs(s), rs(h)
        s = s / s.norm().clamp(min=1e-6)
        h = h / h.norm().clamp(min=1e-6)
        nfft = 1 << (s.shape[1] + K - 1).bit_length()
        Sf = torch.fft.rfft(s, n=nfft)
        r = torch.fft.irfft(Sf.abs().square(), n=nfft)[0, :K].clone()
        bb = torch.fft.irfft(Sf.conj() * torch.fft.rfft(h, n=nfft), n=nfft)[0, :K]
        if diag is not None:
            r[0] += diag
        try:
            coh = bb @ torch.linalg.solve(r[toep], bb)
        except RuntimeError:   # (singular in float32: the yardstick has no gradient for this row)
            got[b, :k] = float("nan")
            continue
        v = 10.0 * torch.log10((coh / (1.0 - coh).clamp(min=1e-8)).clamp(min=1e-8))
        got[b, :k] = torch.autograd.grad(v, x)[0][0].double().numpy()
    return row_errors(got, expected(name)[1])


# Chosen in CPU mode, which follows the statement to 1e-10: 30 steps raise the row from 5.67 to 11.90 dB, each step
# upwards (5e-4 overshoots at step 28, near 25 dB, where the gradient has grown with 1 / (1 - coh)).
ASCENT_STEP = 3e-4


def ascent(metric, device):
    """(the starting SDR, the SDR after each of 30 steps) of gradient ascent on the samples of one 4000-sample
    estimate that starts 5 dB above white noise: h <- h + ASCENT_STEP |h|^2 dSDR/dh (SDR does not depend on the
    estimate's scale and its gradient goes with the inverse, so the step is a fraction of the row per dB)."""
    c, _ = lc.speech_rows(1, 4000, seed=41)
    gen = torch.Generator().manual_seed(43)
    noise = torch.randn(1, 4000, generator=gen)
    est = (c + noise * (c.norm() / noise.norm()) * 10.0 ** (-5.0 / 20.0)).to(device)
    c = c.to(device)
    first = float(metric.scores(c, est))
    trace = []
    for _ in range(30):
        x = est.clone().requires_grad_(True)
        metric.differentiable_scores(c, x).sum().backward()
        est = est + ASCENT_STEP * float(est.double().square().sum()) * x.grad.to(est)
        trace.append(float(metric.scores(c, est)))
    return first, trace
