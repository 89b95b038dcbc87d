"""The float64 statement of the SRMR definition (include/fsem.h "SRMR")
with numpy and scipy's lfilter, independent of the package: the analytic-gammatone form in
complex128 and in complex64, the SRMRpy form (|hilbert| of Slaney's real cascade), seeded input
generators and the rows the tolerance tests use.

Every row of a tolerance test keeps K* stable: on the float64 statement the cumulative share at
the 90 % channel i* is >= 90.5 and at the channel before it <= 89.5 (`reference` asserts it), so no
rounding moves the bandwidth rule to another channel."""
import functools

import numpy as np
from scipy.signal import hilbert, lfilter

NCH, NMOD = 23, 8
EARQ, MINBW = 9.26449, 24.7
TILE = 4096  # samples the engine stages at a time (csrc/srmr.hip)


def geometry(sr: int):
    """(wi, wl): hop and window in samples."""
    return int(np.ceil(0.064 * sr)), int(np.ceil(0.256 * sr))


def frames_of(n: int, sr: int) -> int:
    wi, wl = geometry(sr)
    return 1 + (n - wl) // wi if n >= wl else 0


def erb(f):
    return f / EARQ + MINBW


def centre_freqs(sr: int) -> np.ndarray:
    c = EARQ * MINBW
    i = np.arange(1, NCH + 1)
    return -c + np.exp(i * (np.log(125 + c) - np.log(sr / 2 + c)) / NCH) * (sr / 2 + c)


def mod_filters(sr: int):
    """(b [8, 3], a [8, 3], lower edges L [8]) of the modulation filters."""
    mcf = 4.0 * 32.0 ** (np.arange(NMOD) / 7.0)
    W0 = np.tan(np.pi * mcf / sr)
    B0 = W0 / 2.0
    a0 = 1 + B0 + W0 ** 2
    b = np.stack([B0 / a0, 0 * B0, -B0 / a0], 1)
    a = np.stack([a0 / a0, (2 * W0 ** 2 - 2) / a0, (1 - B0 + W0 ** 2) / a0], 1)
    return b, a, mcf - np.tan(np.pi * mcf / sr) / 2.0 * sr / (2 * np.pi)


def analytic_envelopes(x: np.ndarray, sr: int, ctype=np.complex128) -> np.ndarray:
    """e_i[t] = |h_i * x|, [23, n]; the filter runs in `ctype`, the result is float64."""
    cf = centre_freqs(sr)
    out = np.empty((NCH, len(x)))
    for i in range(NCH):
        p = np.exp((-2 * np.pi * 1.019 * erb(cf[i]) + 2j * np.pi * cf[i]) / sr)
        z0 = np.exp(2j * np.pi * cf[i] / sr)
        G = [q / z0 * (1 + 4 * q / z0 + (q / z0) ** 2) / (1 - q / z0) ** 4 for q in (p, np.conj(p))]
        g = abs(G[0] + G[1]) / 2
        y = lfilter((np.array([0, p, 4 * p * p, p ** 3]) / g).astype(ctype), np.ones(1, ctype), x.astype(ctype))
        for _ in range(4):
            y = lfilter(np.ones(1, ctype), np.array([1, -p]).astype(ctype), y)
        assert y.dtype == ctype
        out[i] = np.abs(y)
    return out


def hilbert_envelopes(x: np.ndarray, sr: int) -> np.ndarray:
    """SRMRpy's envelopes: |hilbert| of Slaney's four-biquad real gammatone, [23, n]."""
    cf = centre_freqs(sr)
    T = 1.0 / sr
    out = np.empty((NCH, len(x)))
    for i in range(NCH):
        B = 2 * np.pi * 1.019 * erb(cf[i])
        th = 2 * np.pi * cf[i] * T
        a = np.array([1.0, -2 * np.cos(th) * np.exp(-B * T), np.exp(-2 * B * T)])
        bs = [np.array([T, -T * np.exp(-B * T) * (np.cos(th) + s * np.sin(th)), 0.0])
              for s in (1 + np.sqrt(2), -(1 + np.sqrt(2)), np.sqrt(2) - 1, -(np.sqrt(2) - 1))]
        zi = np.exp(-1j * th * np.arange(3))
        gain = abs(np.prod([np.dot(b, zi) / np.dot(a, zi) for b in bs]))
        y = x.astype(np.float64)
        for j, b in enumerate(bs):
            y = lfilter(b / gain if j == 0 else b, a, y)
        out[i] = np.abs(hilbert(y))
    return out


def energies_of(env: np.ndarray, sr: int) -> np.ndarray:
    """A[i, k] = mean_f sum_m (w[m] m_ik[f wi + m])^2 from the envelopes, [23, 8]; NaN without a frame."""
    wi, wl = geometry(sr)
    n = env.shape[1]
    F = frames_of(n, sr)
    if F == 0:
        return np.full((NCH, NMOD), np.nan)
    b, a, _ = mod_filters(sr)
    w = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(wl) / wl)
    A = np.empty((NCH, NMOD))
    for k in range(NMOD):
        m = lfilter(b[k], a[k], env, axis=-1)
        fr = np.lib.stride_tricks.sliding_window_view(m, wl, axis=-1)[:, ::wi][:, :F]  # [23, F, wl]
        A[:, k] = np.square(fr * w).sum(-1).mean(-1)
    return A


def shares(A: np.ndarray) -> np.ndarray:
    """The cumulative percentages of the channel energies, walking i = 23, 22, ... 1."""
    ac = A.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):  # (a silent row: 0 / 0)
        return np.cumsum(100 * ac[::-1] / ac.sum())


def score_of(A: np.ndarray, sr: int) -> float:
    if not np.isfinite(A).all():
        return float("nan")
    cum = shares(A)
    over = np.nonzero(cum > 90)[0]
    if not len(over):
        return float("nan")
    bw = erb(centre_freqs(sr)[NCH - 1 - over[0]])
    L = mod_filters(sr)[2]
    K = 8 if bw > L[7] else 7 if bw > L[6] else 6 if bw > L[5] else 5
    den = A[:, 4:K].sum()
    return float(A[:, :4].sum() / den) if den > 0 else float("nan")


def srmr(x, sr: int, form: str = "f64"):
    """(SRMR, A [23, 8]) of one row; form: "f64" (the definition), "c64" (its gammatone stage in
    complex64) or "hilbert" (SRMRpy's envelopes)."""
    x = np.asarray(x, dtype=np.float64)
    if frames_of(len(x), sr) == 0 or not np.isfinite(x).all():
        return float("nan"), np.full((NCH, NMOD), np.nan)
    if form == "hilbert":
        env = hilbert_envelopes(x, sr)
    else:
        env = analytic_envelopes(x.astype(np.float32), sr, np.complex64 if form == "c64" else np.complex128)
    A = energies_of(env, sr)
    return score_of(A, sr), A


def margin(A: np.ndarray):
    """(share at i*, share at the channel before it)."""
    cum = shares(A)
    j = int(np.nonzero(cum > 90)[0][0])
    return float(cum[j]), float(cum[j - 1]) if j else 0.0


# ---- seeded inputs (float32, peak below 1)
def harmonic(sr: int, n: int, seed: int, rate: float = 4.0) -> np.ndarray:
    """A harmonic complex of equal amplitudes up to 0.45 sr with random phases (f0 = 100 + 7 seed Hz), its level
    modulated at `rate` Hz.  (Equal amplitudes: the wide upper channels each hold several per cent of the energy,
    so the 90 % rule has room.)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 100.0 + 7.0 * seed
    h = np.arange(1, int(0.45 * sr / f0) + 1)
    x = np.sin(2 * np.pi * f0 * h[:, None] * t + rng.uniform(0, 2 * np.pi, len(h))[:, None]).sum(0)
    x *= 0.5 * (1 + 0.9 * np.cos(2 * np.pi * rate * t + rng.uniform(0, 2 * np.pi)))
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def white(sr: int, n: int, seed: int, level: float = 0.1) -> np.ndarray:
    return (level * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def noisy(sr: int, n: int, seed: int, snr_db: float = 10.0) -> np.ndarray:
    x = harmonic(sr, n, seed).astype(np.float64)
    v = np.random.default_rng(seed + 1000).standard_normal(n)
    v *= np.sqrt(np.mean(x * x) / np.mean(v * v)) * 10 ** (-snr_db / 20)
    return (x + v).astype(np.float32)


def reverberated(sr: int, n: int, seed: int, t60: float = 0.4) -> np.ndarray:
    x = harmonic(sr, n, seed).astype(np.float64)
    m = int(t60 * sr)
    tail = np.random.default_rng(seed + 2000).standard_normal(m) * 10 ** (-3 * np.arange(m) / m)
    tail[0] = 1.0
    y = np.convolve(x, tail)[:n]
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


KINDS = {"harmonic": harmonic, "noisy": noisy, "reverberated": reverberated, "white": white}


def edge_lengths(sr: int) -> list:
    """Frame and tile edges: wl - 1 (no frame), wl, wl + wi - 1 (one frame), wl + wi (two), kT - 1, kT,
    kT + 1 for the engine's tile T, kT + wi (a last, partial tile) and 1.5 s."""
    wi, wl = geometry(sr)
    k = 2
    return [wl - 1, wl, wl + wi - 1, wl + wi, k * TILE - 1, k * TILE, k * TILE + 1, k * TILE + wi, 3 * sr // 2]


# (kind, seed) of the row at each edge length, chosen so that every row is stable (see `reference`)
EDGE_ROWS = {
    8000: [("harmonic", 1), ("harmonic", 1), ("noisy", 1), ("reverberated", 1), ("white", 1), ("harmonic", 1),
           ("noisy", 1), ("reverberated", 1), ("noisy", 1)],
    16000: [("harmonic", 1), ("harmonic", 3), ("noisy", 1), ("reverberated", 1), ("white", 1), ("harmonic", 3),
            ("noisy", 1), ("reverberated", 1), ("noisy", 3)],
}
# (kind, seed, seconds) of the CPU mode's parity rows
PARITY_ROWS = [("harmonic", 3, 1), ("noisy", 3, 2), ("reverberated", 1, 1), ("white", 1, 2)]


@functools.lru_cache(maxsize=None)
def reference(kind: str, seed: int, sr: int, n: int):
    """(row, (SRMR, A) in float64, (SRMR, A) with the complex64 gammatone) -- computed once, shared, read-only."""
    x = KINDS[kind](sr, n, seed)
    f64, c64 = srmr(x, sr, "f64"), srmr(x, sr, "c64")
    if frames_of(n, sr):
        at, before = margin(f64[1])
        assert at >= 90.5 and before <= 89.5, (kind, seed, sr, n, at, before)
    for a in (x, f64[1], c64[1]):
        a.setflags(write=False)
    return x, f64, c64


def edge_rows(sr: int) -> list:
    """[(row, f64, c64)] at edge_lengths(sr)."""
    return [reference(kind, seed, sr, n) for (kind, seed), n in zip(EDGE_ROWS[sr], edge_lengths(sr))]


def parity_rows(sr: int) -> list:
    """[(row, f64, c64)]: each kind once, 1 s and 2 s."""
    return [reference(kind, seed, sr, sec * sr) for kind, seed, sec in PARITY_ROWS]


def rel(a, b) -> float:
    return float(abs(a - b) / abs(b))


def bars(refs) -> tuple:
    """(score bar, energy bar) of a set of reference rows: 4 x the largest relative |complex64 - float64|
    of the statement itself, the energies relative to the row's largest entry."""
    live = [(f, c) for _, f, c in refs if np.isfinite(f[0])]
    s = max(rel(c[0], f[0]) for f, c in live)
    e = max(float(np.abs(c[1] - f[1]).max() / f[1].max()) for f, c in live)
    return 4 * s, 4 * e
