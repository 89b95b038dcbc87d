"""Cases and references of the STOI / ESTOI gradients (include/fsem.h, "STOI with gradients").

The reference is the definition: ``_cpu.stoi`` (float64, the subgradient 0 at a zero band envelope) on rows
resampled in float64 with ``resample.sinc_kernel``'s float32 taps (``resample64`` here, written apart from the
package's), under torch's autograd.  L = sum_b (g_s[b] STOI_b + g_e[b] ESTOI_b) is linear in the incoming
gradients, so a case keeps two gradients per row, dSTOI_b/dy and dESTOI_b/dy, and every incoming (g_s, g_e)
is their combination.

``restated`` is the same function written out again in plain torch ops in a chosen dtype.  In float64 it
checks the reference; in float32 it is the yardstick of the engine's bar: the engine computes in float32, and
is held to BAR_FACTOR = 32 times the largest error the float32 restatement has against the float64
reference over SETS + LONG (``bar()``), the ratio the forward's bar has to that formulation (3e-6 against a
measured 1.0-1.5e-7).  The error of a row is max|g - g_ref| / max|g_ref|.
"""
import functools

import numpy as np
import torch

from fast_speech_enhancement_metrics_amd import _cpu, synthetic
from fast_speech_enhancement_metrics_amd.resample import sinc_kernel

SEED = 7
# (name, sample rate, length): 1 s at 16 kHz is 10000 samples at 10 kHz -- three 4096-sample resampler chunks,
# ~75 STFT frames (three 32-frame workgroups), one 64-segment wave; row 2 of the 10 kHz and 48 kHz sets has no
# 30-frame segment (NaN scores, a zero gradient row).
SETS = (("16k", 16000, 16000), ("10k", 10000, 9000), ("8k", 8000, 8000), ("48k", 48000, 40000))
LONG = ("long10k", 10000, 50000)   # one row with more than 256 segments (two forward segment blocks, five waves)
RAGGED_LENGTHS = [16000, 12001, 9000, 4000]
ODD_LENGTH = 16001
# 10 kHz rows of 40 VAD frames whose estimate drops to 2^-20 of its level at sample GAP_STEP: the STFT frame pair
# across the step lies 20 peak exponents apart, so both stoi_tob and stoi_tob_grad equalise it (pair_level_shift;
# no other case has a kept frame pair 7 or more exponents apart)
GAP_LENGTH, GAP_STEP = 5248, 128 * 22
BAR_FACTOR = 32.0
UPSTREAMS = ((1.0, 0.0), (0.0, 1.0))
RTOL_CPU = 1e-9      # CPU mode against the reference, of the row's largest gradient
ATOL_SCORE_CPU = 1e-12
# central differences of the reference in float64 along random unit directions: at EPS the quotient moves by
# less than FD_BAR (relative to the directional derivative) when EPS is halved (measured: see
# test_reference_against_central_differences, which prints both)
FD_EPS = 5e-4
FD_BAR = 1e-5


def rows(name: str):
    """(clean, noisy [B, L] float32, sample rate) of a named set."""
    for nm, sr, L in SETS + (LONG,):
        if nm == name:
            B = 1 if nm == LONG[0] else 4
            c, n, _ = synthetic.speech_like_pairs(B, L, sr, seed=SEED)
            return c, n, sr
    if name == "odd":
        c, n, _ = synthetic.speech_like_pairs(4, ODD_LENGTH, 16000, seed=SEED)
        return c, n, 16000
    if name == "gap":
        c, n, _ = synthetic.speech_like_pairs(4, GAP_LENGTH, 10000, seed=SEED)
        n = n.clone()
        n[:, GAP_STEP:] *= 2.0 ** -20
        return c, n, 10000
    if name == "zero":  # the 16 kHz set with an all-zero estimate in row 1
        c, n, sr = rows("16k")
        n = n.clone()
        n[1] = 0
        return c, n, sr
    raise KeyError(name)


def resample64(x: torch.Tensor, sr: int) -> torch.Tensor:
    """[B, n] -> [B, ceil(10000 n / sr)] float64: out[m new + j] = sum_t K[j, t] x[m orig + t - width]."""
    x = x.to(torch.float64)
    if sr == 10000:
        return x
    kern, width, orig, new = sinc_kernel(sr, 10000)
    n = x.shape[1]
    xp = torch.nn.functional.pad(x, (width, width + orig))
    groups = xp.unfold(1, kern.shape[1], orig)                       # [B, M, taps]
    out = torch.einsum("bmt,jt->bmj", groups, kern.to(torch.float64))
    return out.reshape(x.shape[0], -1)[:, :-(-new * n // orig)]


def _obm(dtype):
    freqs = np.arange(257) * (5000.0 / 256)
    m = torch.zeros(15, 257, dtype=dtype)
    for i in range(15):
        lo, hi = 150 * 2.0 ** ((2 * i - 1) / 6), 150 * 2.0 ** ((2 * i + 1) / 6)
        m[i, int(np.argmin(np.abs(freqs - lo))):int(np.argmin(np.abs(freqs - hi)))] = 1
    return m


def restated(x10: torch.Tensor, y10: torch.Tensor, dtype):
    """(stoi, estoi) 0-d tensors of one 10 kHz row pair in ``dtype``, or None without a segment.  The frames are
    selected in float64 from the clean row (a constant of the function), everything else runs in ``dtype``."""
    w64 = torch.hann_window(257)[1:].double()   # the float32 window's values, as the definition
    e = 20 * torch.log10((x10.detach().double().unfold(0, 256, 128) * w64).norm(dim=1) + 1e-9)
    keep = (e.max() - 40 - e) < 0
    n = int(keep.sum())
    S = n - 31
    if S <= 0:
        return None
    w = w64.to(dtype)

    def envelopes(v):
        k = (v.to(dtype).unfold(0, 256, 128) * w)[keep]                # [n, 256]
        z = torch.zeros(1, 128, dtype=dtype)
        sig = (torch.cat([k[:, :128], z]) + torch.cat([z, k[:, 128:]])).reshape(-1)   # overlap-add, (n + 1) 128
        fr = sig.unfold(0, 512, 128)[:, 128:384] * w                    # the window centred in 512 samples
        p = torch.fft.rfft(torch.nn.functional.pad(fr, (128, 128)), dim=1).abs().square() @ _obm(dtype).T   # [T, 15]
        pos = p > 0
        return (torch.where(pos, p, torch.ones_like(p)).sqrt() * pos).T   # sqrt with the subgradient 0 at 0

    X, Y = envelopes(x10), envelopes(y10)
    xs, ys = X.unfold(1, 30, 1)[:, :S].transpose(0, 1), Y.unfold(1, 30, 1)[:, :S].transpose(0, 1)   # [S, 15, 30]

    def vnorm(v, dim):
        return torch.linalg.vector_norm(v, dim=dim, keepdim=True)

    def unit(v, dim):
        v = v - v.mean(dim=dim, keepdim=True)
        return v / torch.sqrt(v.square().sum(dim=dim, keepdim=True) + v.shape[dim] * 1e-24)

    def unit2(v):
        c = v - v.mean(dim=2, keepdim=True)
        n2 = c.square().sum(dim=2, keepdim=True) + 30e-24
        a = c / n2.sqrt()
        a = a - a.mean(dim=1, keepdim=True)
        return a / torch.sqrt(a.square().sum(dim=1, keepdim=True) + (14 / 15) * (1e-24 / n2).sum(dim=1, keepdim=True)
                              + 15e-24)

    clip = 1 + 10 ** (15 / 20)
    yc = torch.minimum(ys * (vnorm(xs, 2) / (vnorm(ys, 2) + 1e-9)), xs * clip)
    return (unit(xs, 2) * unit(yc, 2)).sum() / 15 / S, (unit2(xs) * unit2(ys)).sum() / 30 / S


def _row_grads(fn, est_row):
    """((stoi, estoi) floats, (dSTOI/dy, dESTOI/dy) float64 arrays) of fn(est) -> (s, e) | None for one row."""
    y = est_row.clone().requires_grad_(True)
    out = fn(y)
    if out is None or not (out[0].requires_grad or out[1].requires_grad):
        z = np.zeros(est_row.numel())
        sc = (float("nan"),) * 2 if out is None else (float(out[0]), float(out[1]))
        return sc, (z, z.copy())
    gs, = torch.autograd.grad(out[0], y, retain_graph=True)
    ge, = torch.autograd.grad(out[1], y)
    return (float(out[0].detach()), float(out[1].detach())), (gs.double().numpy(), ge.double().numpy())


def reference_row(clean_row, est_row, sr):
    """The definition for one unpadded row: _cpu.stoi on the float64-resampled rows, under autograd."""
    c10 = resample64(clean_row[None], sr)

    def fn(y):
        if c10.shape[1] < 256:
            return None
        s, e = _cpu.stoi(c10, resample64(y[None], sr))
        return None if bool(torch.isnan(s[0])) else (s[0], e[0])

    return _row_grads(fn, est_row.double())


def restated_row(clean_row, est_row, sr, dtype):
    """The restatement for one unpadded row; the resampler's taps are applied in ``dtype`` too."""
    c10 = resample64(clean_row[None], sr)[0]

    def fn(y):
        if c10.shape[0] < 256:
            return None
        if sr == 10000:
            y10 = y
        else:
            kern, width, orig, new = sinc_kernel(sr, 10000)
            groups = torch.nn.functional.pad(y, (width, width + orig)).unfold(0, kern.shape[1], orig)
            y10 = (groups @ kern.to(dtype).T).reshape(-1)[:-(-new * y.numel() // orig)]
        return restated(c10, y10, dtype)

    return _row_grads(fn, est_row.to(dtype))


@functools.lru_cache(maxsize=None)
def expected(name: str, lengths=None):
    """The reference of a named set: {"scores": [B, 2] float64 (NaN without a segment), "gs", "ge": [B, L] float64,
    zero past each row's length and in rows without a segment}.  ``lengths``: a tuple, the ragged form."""
    c, n, sr = rows(name)
    B, L = c.shape
    out = {"scores": np.full((B, 2), np.nan), "gs": np.zeros((B, L)), "ge": np.zeros((B, L))}
    for b in range(B):
        nb = L if lengths is None else int(lengths[b])
        sc, (gs, ge) = reference_row(c[b, :nb], n[b, :nb], sr)
        out["scores"][b] = sc
        out["gs"][b, :nb], out["ge"][b, :nb] = gs, ge
    for v in out.values():
        v.setflags(write=False)
    return out


def row_errors(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """[B]: max|got - want| / max|want| per row; rows whose reference is zero: max|got| (must be 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(1)
    err = np.abs(got - want).max(1)
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.abs(got).max(1))


@functools.lru_cache(maxsize=None)
def yardstick():
    """{set: [B, 2] errors of the float32 restatement's (dSTOI, dESTOI) against the reference}."""
    res = {}
    for name, sr, L in SETS + (LONG,):
        c, n, _ = rows(name)
        want = expected(name)
        g32 = [restated_row(c[b], n[b], sr, torch.float32)[1] for b in range(c.shape[0])]
        res[name] = np.stack([row_errors(np.stack([g[0] for g in g32]), want["gs"]),
                              row_errors(np.stack([g[1] for g in g32]), want["ge"])], 1)
    return res


def bar() -> float:
    """The engine's bar: BAR_FACTOR x the float32 restatement's largest row error over the whole case set."""
    return BAR_FACTOR * max(float(v.max()) for v in yardstick().values())


def combine(want: dict, g_s, g_e) -> np.ndarray:
    """[B, L]: the reference gradient for incoming (g_s [B], g_e [B])."""
    return np.asarray(g_s, np.float64)[:, None] * want["gs"] + np.asarray(g_e, np.float64)[:, None] * want["ge"]


def incoming(B: int):
    """(g_s, g_e [B] float32) exact in float32, of both signs, away from 0."""
    g = torch.Generator().manual_seed(101)
    v = torch.randint(-16, 17, (2, B), generator=g).float() / 8
    return torch.where(v == 0, torch.ones_like(v), v)


def segments(name: str) -> list:
    """30-frame segments per row of a set (kept frames - 31, 0 without one), from the clean rows."""
    c, _, sr = rows(name)
    return [int(v) for v in _cpu.stoi_segments(resample64(c, sr))]

