"""The float64 statement of the SRMR gradient (include/fsem.h, "SRMR with gradients"; INTEGRATION.md section
21) and the seeded cases of tests/test_srmr_grad_cpu.py and tests/test_srmr_grad_gpu.py.

``expected_row`` is the closed form in numpy with scipy's lfilter on reversed arrays, built from
``srmr_cases``' filter helpers: the forward of ``srmr_cases.analytic_envelopes`` keeping y, the energies and
K* by ``srmr_cases``' own functions, then the six steps of the statement with K* taken as a constant.  It
shares no code with the package's CPU mode (``_cpu.srmr64``) or with the engine, and takes the float32 row as
the engine does.  ``ctype=np.complex64`` runs the gammatone stage and its adjoint in complex64: the yardstick
of the engine's float32 gammatone, as ``srmr_cases.bars`` for the forward.

A row's error is max|g - g_ref| / max|g_ref|.

Bars.  The engine's bar is computed in the test from the statement alone: 4 x max(the largest row error of
the complex64 statement against the complex128 one over the same rows, 2^-24).  The two CPU bars are 4 x the
values measured here and recorded below.
"""
import functools

import numpy as np
import torch
from scipy.signal import lfilter

from . import srmr_cases as sc

RATES = (8000, 16000)
FD_STEP = 1e-4
# The statement against central differences of analytic_envelopes -> energies_of -> score_of in float64 along a
# seeded unit direction at step 1e-4, relative, on the parity rows (harmonic, noisy, reverberated, white):
# 8 kHz 1.4e-8, 7.6e-8, 3.4e-7, 4.2e-9; 16 kHz 8.5e-6, 7.0e-7, 2.5e-7, 8.1e-8.  (The 16 kHz harmonic row's
# derivative along the direction is small, -4.0e-4, and its difference quotient is at its rounding floor: 7.1e-5,
# 6.8e-6, 8.5e-6, 4.2e-5, 9.6e-5 at steps 1e-3, 3e-4, 1e-4, 3e-5, 1e-5.)  A missing term of the adjoint changes
# the derivative by order one, so the bar must stay below FD_LIMIT.
FD_MEASURED = 8.5e-6
FD_BAR = 4 * FD_MEASURED
FD_LIMIT = 1e-3
# _cpu.srmr64 against the statement, both float64 on float64 rows, edge and parity rows, both incoming
# gradients: worst row error 8 kHz edges 6.1e-13, parity 9.6e-13; 16 kHz edges 1.7e-12, parity 1.8e-12 (the
# same recurrences, the sums over k and t in another order).
CPU_MEASURED = 1.8e-12
CPU_BAR = 4 * CPU_MEASURED
# The engine on an MI355X against the statement (tests/test_srmr_grad_gpu.py prints every row's error beside the
# bar it computes from the statement alone; the log is profiles/srmr_loss_a/srmr_grad_tests.log).  Worst row,
# ones / random incoming: 8 kHz edges 2.58e-6 / 2.51e-6 (bar 1.07e-5), parity 2.62e-6 / 2.57e-6 (bar 1.06e-5);
# 16 kHz edges 2.82e-6 / 2.81e-6 (bar 1.07e-5), parity 3.66e-6 / 3.68e-6 (bar 1.44e-5).  The complex64 statement's
# own worst rows: 2.68e-6, 2.64e-6, 2.68e-6, 3.60e-6.  Recorded, never asserted against.
ENGINE_MEASURED = 3.68e-6

ASCENT_ROW = ("reverberated", 1, 1)   # (kind, seed, seconds)
# x <- x + ASCENT_STEP |x|^2 dSRMR/dx (SRMR does not depend on the row's scale and its gradient goes with the
# inverse, so the step is a fraction of the row per unit of SRMR).  Chosen in CPU mode, where the statement is
# followed: 20 steps of 1e-4, 2e-4, 3e-4 and 5e-4 raise SRMR at every step at both rates (2e-4: 1.964 -> 2.879 at
# 8 kHz, 1.795 -> 2.884 at 16 kHz), 1e-3 overshoots within the 20 steps; 2e-4 leaves a factor 2.5 to the
# largest step that still climbs.
ASCENT_STEP = 2e-4
ASCENT_STEPS = 20


def gammatone(sr: int):
    """(p [23], g [23]): the poles and gains of include/fsem.h "SRMR", from srmr_cases' centre frequencies."""
    cf = sc.centre_freqs(sr)
    p = np.exp((-2 * np.pi * 1.019 * sc.erb(cf) + 2j * np.pi * cf) / sr)
    z0 = np.exp(2j * np.pi * cf / sr)

    def G(q):
        return q / z0 * (1 + 4 * q / z0 + (q / z0) ** 2) / (1 - q / z0) ** 4

    return p, np.abs(G(p) + G(np.conj(p))) / 2


def kstar(A: np.ndarray, sr: int) -> int:
    cum = sc.shares(A)
    bw = sc.erb(sc.centre_freqs(sr)[sc.NCH - 1 - int(np.nonzero(cum > 90)[0][0])])
    L = sc.mod_filters(sr)[2]
    return 8 if bw > L[7] else 7 if bw > L[6] else 6 if bw > L[5] else 5


def frame_weights(n: int, sr: int) -> np.ndarray:
    """V[t] = sum_f w^2[t - f wi], t < nend."""
    wi, wl = sc.geometry(sr)
    F = sc.frames_of(n, sr)
    w2 = np.square(0.54 - 0.46 * np.cos(2 * np.pi * np.arange(wl) / wl))
    V = np.zeros((F - 1) * wi + wl)
    for f in range(F):
        V[f * wi:f * wi + wl] += w2
    return V


def expected_row(x, sr: int, ctype=np.complex128):
    """(SRMR, d SRMR / d x [n]) of one unpadded row, float64; (NaN, zeros) for a row without a frame, with a
    non-finite sample or with a non-finite score."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    F = sc.frames_of(n, sr)
    if F == 0 or not np.isfinite(x).all():
        return float("nan"), np.zeros(n)
    p, g = gammatone(sr)
    b, a, _ = sc.mod_filters(sr)
    ys = []
    for i in range(sc.NCH):
        y = lfilter((np.array([0, p[i], 4 * p[i] ** 2, p[i] ** 3]) / g[i]).astype(ctype), np.ones(1, ctype), x.astype(ctype))
        for _ in range(4):
            y = lfilter(np.ones(1, ctype), np.array([1, -p[i]]).astype(ctype), y)
        assert y.dtype == ctype
        ys.append(y)
    env = np.abs(np.stack(ys)).astype(np.float64)
    A = sc.energies_of(env, sr)
    score = sc.score_of(A, sr)
    if not np.isfinite(score):
        return float("nan"), np.zeros(n)
    K = kstar(A, sr)
    N, D = A[:, :4].sum(), A[:, 4:K].sum()
    c = np.zeros(sc.NMOD)
    c[:4] = 1.0 / D
    c[4:K] = -N / (D * D)
    V = frame_weights(n, sr)
    nend = len(V)
    dx = np.zeros(n)
    for i in range(sc.NCH):
        de = np.zeros(nend)
        for k in range(K):
            m = lfilter(b[k], a[k], env[i])[:nend]
            q = (2.0 * c[k] / F) * m * V
            r = lfilter([1.0], a[k], q[::-1])[::-1]          # r[t] = q[t] - a1 r[t + 1] - a2 r[t + 2]
            r2 = np.concatenate([r[2:], np.zeros(2)])         # r[t + 2], 0 from nend on
            de += b[k][0] * (r - r2)
        a0 = np.zeros(n, dtype=np.complex128)
        e = env[i, :nend]
        live = e > 0
        a0[:nend][live] = de[live] * ys[i][:nend][live].astype(np.complex128) / e[live]   # |y| = 0: 0
        aj = a0.astype(ctype)[::-1]
        for _ in range(4):
            aj = lfilter(np.ones(1, ctype), np.array([1, -np.conj(p[i])]).astype(ctype), aj)
        assert aj.dtype == ctype
        a4 = np.concatenate([aj[::-1].astype(np.complex128), np.zeros(3)])
        taps = (np.array([p[i], 4 * p[i] ** 2, p[i] ** 3]) / g[i]).astype(ctype).astype(np.complex128)
        dx += np.real(np.conj(taps[0]) * a4[1:n + 1] + np.conj(taps[1]) * a4[2:n + 2] + np.conj(taps[2]) * a4[3:n + 3])
    return score, dx


@functools.lru_cache(maxsize=None)
def expected(kind: str, seed: int, sr: int, n: int, single: bool = False):
    """``expected_row`` of a seeded row of srmr_cases (complex64 gammatone when ``single``), computed once,
    shared, read-only."""
    x = sc.reference(kind, seed, sr, n)[0]
    score, g = expected_row(x, sr, np.complex64 if single else np.complex128)
    g.setflags(write=False)
    return score, g


def edge_specs(sr: int) -> list:
    return [(kind, seed, sr, n) for (kind, seed), n in zip(sc.EDGE_ROWS[sr], sc.edge_lengths(sr))]


def parity_specs(sr: int) -> list:
    return [(kind, seed, sr, sec * sr) for kind, seed, sec in sc.PARITY_ROWS]


SETS = {"edges": edge_specs, "parity": parity_specs}


def batch_of(specs, fill=True):
    """(rows [B, L] float32, lengths) of the specs' rows as one ragged batch; past each length the memory holds
    NaN (even rows) or 1e30 (odd rows)."""
    rows = [sc.reference(*s)[0] for s in specs]
    lens = [len(r) for r in rows]
    out = torch.zeros(len(rows), max(lens))
    for b, r in enumerate(rows):
        out[b, :lens[b]] = torch.from_numpy(np.array(r))
        if fill:
            out[b, lens[b]:] = float("nan") if b % 2 == 0 else 1e30
    return out, lens


def expected_batch(specs, single: bool = False) -> np.ndarray:
    """[B, L] float64: the expected gradients for incoming gradients all one, zeros past each length."""
    grads = [expected(*s, single)[1] for s in specs]
    out = np.zeros((len(grads), max(len(g) for g in grads)))
    for b, g in enumerate(grads):
        out[b, :len(g)] = g
    return out


def engine_bar(specs) -> float:
    """4 x max(the largest row error of the complex64 statement against the complex128 one, 2^-24)."""
    err = row_errors(expected_batch(specs, True), expected_batch(specs, False))
    return 4 * max(float(err.max()), 2.0 ** -24)


def row_errors(got, want) -> np.ndarray:
    """[B] max|g - g_ref| / max|g_ref| per row (the absolute difference where the reference row is all zero)."""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(w).max(axis=1)
    diff = np.abs(g - w).max(axis=1)
    return np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), diff)


def incoming(batch: int) -> torch.Tensor:
    """The seeded random incoming gradient [B] (float32, 0.5 .. 1.5 in magnitude, both signs)."""
    gen = torch.Generator().manual_seed(29)
    u = torch.rand(batch, generator=gen) + 0.5
    return torch.where(torch.rand(batch, generator=gen) < 0.5, -u, u)


def nend_of(n: int, sr: int) -> int:
    wi, wl = sc.geometry(sr)
    F = sc.frames_of(n, sr)
    return (F - 1) * wi + wl if F else 0


def ascent(metric, device):
    """(the starting SRMR, the SRMR after each of ASCENT_STEPS steps) of gradient ascent on the samples of the
    one-second reverberated row: x <- x + ASCENT_STEP |x|^2 dSRMR/dx."""
    kind, seed, sec = ASCENT_ROW
    x = torch.from_numpy(np.array(sc.reference(kind, seed, metric.sample_rate, sec * metric.sample_rate)[0]))[None].to(device)
    first = float(metric.scores(x))
    trace = []
    for _ in range(ASCENT_STEPS):
        v = x.clone().requires_grad_(True)
        metric.differentiable_scores(v).sum().backward()
        x = x + ASCENT_STEP * float(x.double().square().sum()) * v.grad.to(x)
        trace.append(float(metric.scores(x)))
    return first, trace
