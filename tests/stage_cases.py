"""Statements, yardsticks and cases of the two stage kernels' outputs, band by band: ``stoi_tob``'s third-octave
envelopes and ``pesq_front``'s Bark bands and band-pass power (tests/test_stage_bands_cpu.py holds the statements
to the pinned oracle, tests/test_stage_bands_gpu.py holds the kernels to the statements).  CPU only; the engine
library is not loaded here.

float64 statements, evaluated in float64 end to end from the float32 rows:
  tob64(clean10, deg10)  -> (kept, tob [2, 15, T]): oracle/stoi_oracle.py's steps (hann(257)[1:] window, 40 dB
                            selection on the clean row, overlap-add of the kept frames, 512-point STFT with the
                            256-sample window centred and hop 128, band sums over band_edges(), square root)
                            without the oracle's float32 roundings of the overlap-added signal and the powers.
  bark64(row)            -> (power, bark [F, 49]): ``_bark`` below without the level scale (the pre-emphasis and
                            the transform are linear: unscaled = scaled p / 1e7), power = sum u^2 of the band-pass.

float32 yardsticks: the same two statements in float32, (a) one real transform per frame, (b) two consecutive
frames per complex transform with the Hermitian split in float32, at both pair parities.  The yardstick of a case
is the larger of (a) and (b); a family's is its largest case's.  The float32 Bark statement's pre-emphasis is the
float32 ``oracle.ta.lfilter`` order that tests/test_stage_api_gpu.py pins bitwise to the engine's stage entry;
``bark32`` also has the order pesq_front itself takes (the second difference first, the recursion restarted every
52 samples from a scanned state), for the per-band yardstick (front_band_yardstick).

Error norms, per element, so that a quiet band counts:
  neighbour norm  |got - ref| / max(ref[j, t-1], ref[j, t], ref[j, t+1], phi max_j' of those three frames):
                  the rounding of a pair transform is relative to the neighbour's spectrum in that bin, by
                  design.  phi = 2^-16 for envelopes (amplitudes), 2^-24 for Bark powers.
  own-frame norm  |got - ref| / max(ref[j, t], 2^-8 max_j ref[:, t]), for the level-gap family only.

Cases (``tob_cases``, ``front_cases``), all seeded: tob frame-count edges, selection gaps, level gaps with zero
runs, spectra; front-end lengths on every segment and frame edge, spectra, ragged batches.  The speech-like rows
come out of torch's float32 sin and exp, whose last bit differs between CPUs, and a rounding to the int16 grid
turns that into a whole step at a sample or two: statements and engine must see the rows of one process.  An
engine output dumped on one machine set against statements of rows generated on another shows a one-sample
click (1e-4 of a quiet band in one frame), not an engine error.
"""
import functools

import numpy as np
import scipy.fft
import torch
from scipy.signal import lfilter, sosfilt

from fast_speech_enhancement_metrics_amd import _cpu, synthetic
from fast_speech_enhancement_metrics_amd import _tables as T
from oracle import stoi_oracle as so
from oracle import ta

FACTOR = 4.0                      # "rounds in another order, not in another kind" (tests/test_srmr_gpu.py)
PHI_TOB, PHI_BARK = 2.0 ** -16, 2.0 ** -24
PHI_OWN = 2.0 ** -8
MARGIN_DB = 0.01                  # every frame's distance from the 40 dB selection threshold, float64
FORMS = ("single", "pair0", "pair1")

# ------------------------------------------------------------------------------------------ transforms


def _pair_powers(fr, parity):
    """[n, N] real frames -> [n, N/2 + 1] powers, two consecutive frames per complex transform (frame a real,
    frame b imaginary) and the Hermitian split, in the frames' precision.  Pairs start at frame ``parity``; a
    frame without a partner is transformed against zeros."""
    n, N = fr.shape
    z0 = np.zeros((parity, N), fr.dtype)
    z1 = np.zeros(((n + parity) % 2, N), fr.dtype)
    f = np.concatenate([z0, fr, z1], 0)
    z = np.empty((f.shape[0] // 2, N), np.complex64 if fr.dtype == np.float32 else np.complex128)
    z.real, z.imag = f[0::2], f[1::2]
    z = scipy.fft.fft(z, axis=1)
    k = np.arange(N // 2 + 1)
    zr, zi = z.real[:, k], z.imag[:, k]
    mr, mi = z.real[:, (-k) % N], z.imag[:, (-k) % N]
    quarter = fr.dtype.type(0.25)
    pa = ((zr + mr) ** 2 + (zi - mi) ** 2) * quarter
    pb = ((zi + mi) ** 2 + (zr - mr) ** 2) * quarter
    out = np.empty((f.shape[0], N // 2 + 1), fr.dtype)
    out[0::2], out[1::2] = pa, pb
    return out[parity:parity + n]


def _powers(fr, form):
    assert form in FORMS and fr.dtype in (np.float32, np.float64)
    if fr.shape[0] == 0:
        return np.zeros((0, fr.shape[1] // 2 + 1), fr.dtype)
    if form == "single":
        z = scipy.fft.rfft(fr, axis=1)
        assert z.real.dtype == fr.dtype
        return z.real ** 2 + z.imag ** 2
    return _pair_powers(fr, int(form[-1]))


# ------------------------------------------------------------------------------------------ third-octave envelopes
_W = so.window()             # hann(257)[1:], float32
_TOB_EDGES = so.band_edges()


def select64(clean10):
    """(keep mask [frames], smallest distance in dB of a frame from the selection threshold) in float64."""
    x = np.asarray(clean10, np.float32).astype(np.float64)
    n = (x.shape[0] - so.WIN) // so.HOP + 1
    if n <= 0:
        return np.zeros(0, bool), np.inf
    fr = x[so.HOP * np.arange(n)[:, None] + np.arange(so.WIN)[None, :]] * _W.astype(np.float64)
    e = 20.0 * np.log10(np.sqrt((fr ** 2).sum(1)) + 1e-9)
    d = e.max() - so.DYN_RANGE - e
    return d < 0, float(np.abs(d).min())


def stft_frames(row, keep, dt):
    """[T, 512] windowed, zero-padded STFT frames of the overlap-added kept frames of one 10 kHz row, in ``dt``."""
    w = _W.astype(dt)
    x = np.asarray(row, np.float32).astype(dt)
    i = np.nonzero(keep)[0]
    nk = i.shape[0]
    fr = x[so.HOP * i[:, None] + np.arange(so.WIN)[None, :]] * w
    blk = np.zeros((nk + 1, so.HOP), dt)            # the overlap-added signal in 128-sample blocks
    blk[:-1] += fr[:, :so.HOP]
    blk[1:] += fr[:, so.HOP:]
    nt = max(nk - 2, 0)
    out = np.zeros((nt, so.N_FFT), dt)
    out[:, 128:256] = blk[1:nt + 1] * w[:so.HOP]
    out[:, 256:384] = blk[2:nt + 2] * w[so.HOP:]
    return out


def tob_rows(clean10, deg10, dt, form="single", promote=None):
    """(kept, tob [2, 15, T]) of one row pair in ``dt``; the selection is always the float64 one.  ``promote``: one
    of "ola", "fft", "bands", the stage (overlap-add and windows; transform and powers; band sums and square root)
    evaluated in float64 instead, its result rounded to ``dt``: which stage carries an error."""
    keep, _ = select64(clean10)
    out = []
    for row in (clean10, deg10):
        fr = stft_frames(row, keep, np.float64 if promote == "ola" else dt).astype(dt)
        p = _powers(fr.astype(np.float64) if promote == "fft" else fr, form).astype(dt)
        if promote == "bands":
            p = p.astype(np.float64)
        bands = np.stack([p[:, lo:hi].sum(1) for lo, hi in _TOB_EDGES], 0) if p.shape[0] else np.zeros((15, 0), dt)
        out.append(np.sqrt(bands).astype(dt))
    return int(keep.sum()), np.stack(out, 0)


def tob64(clean10, deg10):
    return tob_rows(clean10, deg10, np.float64)


# ------------------------------------------------------------------------------------------ Bark bands
_EDGES = np.concatenate([[0], np.cumsum(T.BINS_PER_BAND)])
_PRE = (np.asarray(T.PRE_B, np.float32), np.asarray(T.PRE_A, np.float32))


class _Filter(torch.autograd.Function):
    """One of the two IIRs on a 1-D row from zero state and its adjoint: the same filter on the time-reversed
    gradient.  The recursion itself runs in float64 and its output is rounded to the row's dtype: scipy's
    float32 direct form forms b0 x[n] - 2 b0 x[n-1] + b0 x[n-2] from three rounded products and loses the low
    frequencies' digits there (measured: it alone puts the float32 restatement's error at 2e-3, 20 times the rest
    of the chain's), which is that evaluation order's error, not the format's; the engine takes the second
    difference exactly (csrc/pesq.hip, pre_fir).  This choice only tightens the bar."""

    @staticmethod
    def run(x, kind):
        v = x.detach().numpy()
        if kind == "bp":
            return torch.from_numpy(sosfilt(_cpu._BP_SOS, v.astype(np.float64)).astype(v.dtype))
        return torch.from_numpy(lfilter(_PRE[0].astype(np.float64), _PRE[1].astype(np.float64),
                                        v.astype(np.float64)).astype(v.dtype))

    @staticmethod
    def forward(ctx, x, kind):
        ctx.kind = kind
        return _Filter.run(x, kind)

    @staticmethod
    def backward(ctx, g):
        return _Filter.run(g.flip(0), ctx.kind).flip(0), None


def _bark(x, dtype, level=True):
    """[L] -> Bark bands [F, 49] after level alignment (``level``), taper and pre-emphasis."""
    L = x.numel()
    s = x
    if level:
        u = _Filter.apply(x, "bp")
        s = x * torch.sqrt(1e7 / ((u * u).sum() / (L + 5120) / 1.04684))
    w = torch.ones(L, dtype=dtype)
    w[:15] = torch.arange(1, 16, dtype=dtype) / 16
    w[-15:] = torch.arange(15, 0, -1, dtype=dtype) / 16
    s = torch.nn.functional.pad(_Filter.apply(s * w, "pre"), (0, L % 256))
    z = torch.fft.rfft(s.unfold(0, 512, 256) * torch.hann_window(512, dtype=dtype), dim=1)
    p = z.real.square() + z.imag.square()
    corr = torch.tensor(T.POW_DENS_CORRECTION, dtype=torch.float64) * T.SP_16K
    bands = [p[:, max(int(lo), 1):int(hi)].sum(1) for lo, hi in zip(_EDGES[:-1], _EDGES[1:])]   # (bin 0 is zeroed)
    return torch.stack(bands, 1) * corr.to(dtype)


def frames_of(L: int) -> int:
    Lp = L + L % 256
    return 0 if Lp < 512 else 1 + (Lp - 512) // 256


def bark64(row):
    """(power, bark [F, 49]) of one unpadded 16 kHz row in float64, before the level scale."""
    x = torch.from_numpy(np.array(row, np.float32)).double()
    u = _Filter.run(x, "bp")
    return float((u * u).sum()), _bark(x, torch.float64, level=False).numpy()


# pesq_front's time-parallel pre-emphasis (csrc/pesq.hip phases B-D, tables as csrc/gen_tables.py builds them): a tile
# of 256 chunks of 52 samples from 768 samples before the segment's 48 frames, zero state at the tile's start; the
# all-pole part y[n] = dd[n] - a1 y[n-1] - a2 y[n-2] on the exact second difference dd; per chunk the end state of
# its zero-state response as a functional of the first differences, in the coupled basis (u, v) = T (y1, y2); a
# 4-level Hillis-Steele scan with the chunk transition's powers; the start state back in (y1, y2); the recursion
# again from there.  Every float32 operation in the kernel's order (fused multiply-adds included).
_CH, _WARM, _NF = 52, 768, 48
_TILE = 256 * _CH


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scan_tables():
    a = _PRE[1].astype(np.float64)
    M = np.array([[-a[1], -a[2]], [1.0, 0.0]])
    G = np.zeros((_CH, 2))
    P = np.eye(2)
    for k in range(_CH - 1, -1, -1):
        G[k] = P @ np.array([1.0, 0.0])
        P = M @ P
    r = np.sqrt(a[2])
    c = -a[1] / (2 * r)
    Tm = np.array([[1.0, -r * c], [0.0, r * np.sqrt(1.0 - c * c)]])
    Ti = np.linalg.inv(Tm)
    G2 = G @ Tm.T
    Mch = np.linalg.matrix_power(M, _CH)
    A2 = np.stack([Tm @ np.linalg.matrix_power(Mch, d) @ Ti for d in (1, 2, 4, 8)])
    H2 = G2 - np.vstack([G2[1:], np.zeros((1, 2))])
    return tuple(np.asarray(v, np.float32) for v in (H2, -G2[0], A2, Ti, a))


def _pre_scan_frames(xw):
    """[F, 512] float32: the frames of the tapered row ``xw`` after pesq_front's pre-emphasis, before its b0."""
    H2, B0, A2, Ti, a = _scan_tables()
    L = xw.shape[0]
    F = frames_of(L)
    out = np.zeros((F, 512), np.float32)
    for g in range((F + _NF - 1) // _NF):
        t0 = g * _NF * 256 - _WARM
        tile = np.zeros(_TILE, np.float32)
        lo, hi = max(t0, 0), min(L, t0 + _TILE)
        tile[lo - t0:hi - t0] = xw[lo:hi]
        d = np.diff(tile, prepend=np.float32(0))                      # first differences, zero history at the start
        dd = np.diff(d, prepend=np.float32(0)).reshape(256, _CH)
        d1 = np.concatenate([[np.float32(0)], d[_CH - 1:-1:_CH]])       # d[-1] of each chunk
        dc = d.reshape(256, _CH)
        e = np.stack([B0[0] * d1, B0[1] * d1], 1).astype(np.float32)   # pass 1: zero-state end states (u, v)
        for n in range(_CH):
            e = np.stack([_fma(H2[n, 0], dc[:, n], e[:, 0]), _fma(H2[n, 1], dc[:, n], e[:, 1])], 1)
        for lv in range(4):                                            # the scan
            q = np.zeros_like(e)
            q[1 << lv:] = e[:-(1 << lv)]
            e = np.stack([_fma(A2[lv, i, 0], q[:, 0], _fma(A2[lv, i, 1], q[:, 1], e[:, i])) for i in (0, 1)], 1)
        st = np.zeros_like(e)
        st[1:] = e[:-1]                                                # chunk j starts from chunk j - 1's prefix
        y1 = _fma(Ti[0, 0], st[:, 0], Ti[0, 1] * st[:, 1])
        y2 = _fma(Ti[1, 0], st[:, 0], Ti[1, 1] * st[:, 1])
        y = np.zeros((256, _CH), np.float32)
        for n in range(_CH):                                           # pass 2
            y[:, n] = _fma(-a[1], y1, _fma(-a[2], y2, dd[:, n]))
            y1, y2 = y[:, n], y1
        y = y.reshape(-1)
        y[max(L - t0, 0):] = 0                                         # the row is zero-padded after the filter
        for f in range(g * _NF, min(F, (g + 1) * _NF)):
            o = _WARM + 256 * (f - g * _NF)
            out[f] = y[o:o + 512]
    return out


def bark32(row, form="single", pre="ta"):
    """The float32 statement: (power, bark [F, 49]) float32.  Band-pass: scipy's float32 second-order sections.
    Pre-emphasis ``pre``: "ta", the float32 lfilter order of oracle/c/lfilter_f32.c (b0 x[n] + b1 x[n-1] + b2 x[n-2]
    from three rounded products, then the recursion); "diff", b1 = -2 b0 and b2 = b0 up to their last digit, so the
    numerator is b0 times the second difference (x[n] - x[n-1]) - (x[n-1] - x[n-2]), formed first, the same float32
    recursion on it, and b0 folded into the window; "scan", "diff" with the recursion restarted every 52 samples from
    a state that a float32 scan over the chunks' zero-state responses supplies, as pesq_front runs it
    (``_pre_scan_frames``).  The float32 recursions lose the quiet low bands' digits whichever order they take (band 1
    of a speech row: 5e-2, where a float64 recursion rounded to float32 leaves 2e-4)."""
    x = np.array(row, np.float32)
    L = x.shape[0]
    u = sosfilt(_cpu._BP_SOS.astype(np.float32), x)
    assert u.dtype == np.float32
    power = (u * u).sum(dtype=np.float32)
    w = np.ones(L, np.float32)
    w[:15] = np.arange(1, 16, dtype=np.float32) / np.float32(16)
    w[-15:] = np.arange(15, 0, -1, dtype=np.float32) / np.float32(16)
    win = torch.hann_window(512).numpy()
    F = frames_of(L)
    if pre == "scan":
        fr = _pre_scan_frames(x * w) * (win * _PRE[0][0])
    else:
        if pre == "ta":
            s = ta.lfilter(x * w, _PRE[1], _PRE[0])[0]
        else:
            assert pre == "diff"
            d = np.diff(x * w, prepend=np.float32(0))
            s = ta.lfilter_iir(np.diff(d, prepend=np.float32(0)), _PRE[1])[0]
            win = win * _PRE[0][0]
        s = np.pad(s, (0, L % 256))
        fr = s[256 * np.arange(F)[:, None] + np.arange(512)[None, :]] * win
    p = _powers(fr.astype(np.float32), form)
    corr = (np.asarray(T.POW_DENS_CORRECTION, np.float64) * T.SP_16K).astype(np.float32)
    bands = [p[:, max(int(lo), 1):int(hi)].sum(1, dtype=np.float32) for lo, hi in zip(_EDGES[:-1], _EDGES[1:])]
    return power, np.stack(bands, 1) * corr


# ------------------------------------------------------------------------------------------ norms
def neighbour_err(got, ref, phi):
    """[..., J, T] -> per-element error under the neighbour norm (bands on axis -2, frames on axis -1).  Where
    the three frames are all zero in every band the error is 0 for an exact zero and inf otherwise."""
    got, ref = np.asarray(got, np.float64), np.abs(np.asarray(ref, np.float64))
    pad = np.zeros(ref.shape[:-1] + (1,))
    m3 = np.maximum(np.maximum(np.concatenate([pad, ref[..., :-1]], -1), ref), np.concatenate([ref[..., 1:], pad], -1))
    den = np.maximum(m3, phi * m3.max(axis=-2, keepdims=True))
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, diff / np.where(den > 0, den, 1.0), np.where(diff == 0, 0.0, np.inf))


def own_err(got, ref):
    """[..., J, T] -> per-element error under the own-frame norm."""
    got, ref = np.asarray(got, np.float64), np.abs(np.asarray(ref, np.float64))
    den = np.maximum(ref, PHI_OWN * ref.max(axis=-2, keepdims=True))
    diff = np.abs(got - ref)
    return np.where(den > 0, diff / np.where(den > 0, den, 1.0), np.where(diff == 0, 0.0, np.inf))


# ------------------------------------------------------------------------------------------ tob cases
def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def steady(L, seed, fs=10000):
    """(clean, degraded) [L] float32: a stationary harmonic-plus-noise row, every frame far inside the selection."""
    r = np.random.default_rng(seed)
    t = np.arange(L) / fs
    c = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.2, 0.12, 0.08, 0.04), (220., 570., 1310., 2930.),
                                                                 r.uniform(0, 2 * np.pi, 4)))
    c = c + 0.03 * r.standard_normal(L)
    return _f32(c), _f32(c + 0.05 * r.standard_normal(L))


def _speech10(B, L, seed):
    c, n, _ = synthetic.speech_like_pairs(B, L, 10000, seed=seed)
    return c.numpy().copy(), n.numpy().copy()


EDGE_T = (1, 2, 31, 32, 33, 63, 64, 65)
GAP_L = 8192                         # 63 selection frames
LEVEL_L = 8192
LEVEL_STEPS = (6, 7, 8, 20, 40)
ZERO_RUNS = ((9, 1), (15, 2), (22, 33))   # (first zero STFT frame, count)
SPEC_L = 10000
IMPULSE_PERIOD = 131                 # coprime to 128: impulses fall at every position of the window


def _click(row, centre, amp=0.8):
    row[centre - 3:centre + 4] = amp * np.array([1, -1, 1, -1, 1, -1, 1], np.float32)


def _gap_rows():
    """Four clean rows whose selection leaves gaps (names in GAP_NAMES) and their degraded rows."""
    c, n = _speech10(4, GAP_L, seed=31)
    nv = (GAP_L - 256) // 128 + 1
    c[0, :256] = 0                                    # first frame dropped (digital silence)
    c[1, 128 * (nv - 1):] = 0                         # last frame dropped
    c[2, 128 * 20:128 * 34] = 0                       # frames 20..32 silent, then a click at the centre of every
    for i in range(21, 32, 2):                        # other one: 21, 23, ... kept, 20, 22, ... dropped
        _click(c[2], 128 * i + 128)
    c[3, 128 * 24:128 * 32] *= np.float32(1e-3)       # a -60 dB stretch, one kept frame inside it
    c[3, 128 * 26:128 * 31] = 0
    _click(c[3], 128 * 27 + 128)
    return c, n


GAP_NAMES = ("first_dropped", "last_dropped", "alternate", "single_kept")


def _frame_peaks32(row, keep):
    return np.abs(stft_frames(row, keep, np.float32)).max(1)


def _exponent(v):
    return np.frexp(np.asarray(v, np.float32))[1]


def level_rows(direction, parity):
    """(clean, degraded [5, L], frame index t of the step, quiet STFT frames): the degraded rows step by 2^-k,
    k over LEVEL_STEPS, at one STFT frame boundary.  "down": loud before sample 128 (t + 1), quiet from there on,
    frame t the first all-quiet one next to the half-loud frame t - 1.  "up": quiet before sample 128 (t + 2), frame
    t - 1 the last all-quiet one next to the half-loud frame t.  t has the asked parity and is the first one from 20
    at which the two frames' float32 peak exponents differ by exactly k for every k."""
    c, d = steady(LEVEL_L, 77)
    keep = np.ones((LEVEL_L - 256) // 128 + 1, bool)
    for t in range(20 + (parity - 20) % 2, 50, 2):
        rows = []
        for k in LEVEL_STEPS:
            g = np.ones(LEVEL_L, np.float32)
            if direction == "down":
                g[128 * (t + 1):] = np.float32(2.0 ** -k)
            else:
                g[:128 * (t + 2)] = np.float32(2.0 ** -k)
            rows.append(d * g)
        ok = True
        for k, r in zip(LEVEL_STEPS, rows):
            e = _exponent(_frame_peaks32(r, keep))
            gap = e[t - 1] - e[t] if direction == "down" else e[t] - e[t - 1]
            ok = ok and gap == k
        if ok:
            T_ = keep.sum() - 2
            quiet = np.arange(t, T_) if direction == "down" else np.arange(0, t)
            return np.repeat(c[None], len(LEVEL_STEPS), 0), np.stack(rows), t, quiet
    raise AssertionError("no step position with exact exponent gaps")


def _zero_rows():
    c, d = steady(LEVEL_L, 78)
    rows = []
    for t0, cnt in ZERO_RUNS:
        r = d.copy()
        r[128 * (t0 + 1):128 * (t0 + cnt + 2)] = 0
        rows.append(r)
    return np.repeat(c[None], len(rows), 0), np.stack(rows)


def _spectra_rows():
    c, n = _speech10(2, SPEC_L, seed=11)
    r = np.random.default_rng(5)
    t = np.arange(SPEC_L) / 10000.0
    k_edge = int(_TOB_EDGES[7, 0])                       # first bin of band 7: a third-octave band edge
    tones = np.stack([0.5 * np.sin(2 * np.pi * k_edge * 10000.0 / 512 * t),
                      0.5 * np.sin(2 * np.pi * (k_edge + 20.5) * 10000.0 / 512 * t),   # between two FFT bins
                      np.where(np.arange(SPEC_L) % IMPULSE_PERIOD == 0, 0.8, 0.0)])
    return {"speech": (c, n), "dc100": (c + np.float32(100), n + np.float32(100)),
            "dc1000": (c + np.float32(1000), n + np.float32(1000)),
            "tones": (_f32(tones), _f32(tones + 0.01 * r.standard_normal(tones.shape)))}


@functools.lru_cache(maxsize=None)
def tob_cases():
    """{name: {"family", "clean", "deg" [B, L] float32 (read-only), further keys of the family}}."""
    cases = {}
    for T_ in EDGE_T:                                     # all frames kept: kept = T + 2
        c, d = steady((T_ + 3) * 128, 100 + T_)
        cases[f"edge_T{T_}"] = dict(family="edges", clean=c[None], deg=d[None], T=T_)
    c, d = steady(1024, 99)
    c[200:] = 0                                           # two frames hold signal: kept = 2, nothing written
    cases["edge_kept2"] = dict(family="edges", clean=c[None], deg=d[None], T=0)
    c, d = _gap_rows()
    cases["gaps"] = dict(family="gaps", clean=c, deg=d)
    for direction in ("down", "up"):
        for parity in (0, 1):
            c, d, t, quiet = level_rows(direction, parity)
            cases[f"level_{direction}_{'even' if parity == 0 else 'odd'}"] = dict(
                family="levels", clean=c, deg=d, t=t, quiet=quiet, direction=direction)
    c, d = _zero_rows()
    cases["level_zero_runs"] = dict(family="levels", clean=c, deg=d, zero_runs=ZERO_RUNS)
    for name, (c, d) in _spectra_rows().items():
        cases[f"spec_{name}"] = dict(family="spectra", clean=_f32(c), deg=_f32(d))
    for v in cases.values():
        for k in ("clean", "deg"):
            v[k] = _f32(v[k])
            v[k].setflags(write=False)
    return cases


TOB_FAMILIES = ("edges", "gaps", "levels", "spectra")


@functools.lru_cache(maxsize=None)
def tob_expected(name):
    """The statements of a case, computed once: {"kept": [B], "margin": dB, "ref": list over rows of [2, 15, T]
    float64, "f32": {form: list of [2, 15, T] float32}, "yard": {form: largest neighbour-norm error}}."""
    case = tob_cases()[name]
    B = case["clean"].shape[0]
    out = {"kept": [], "ref": [], "f32": {f: [] for f in FORMS}, "margin": np.inf}
    for b in range(B):
        c, d = case["clean"][b], case["deg"][b]
        kept, ref = tob64(c, d)
        out["kept"].append(kept)
        out["ref"].append(ref)
        out["margin"] = min(out["margin"], select64(c)[1])
        for f in FORMS:
            out["f32"][f].append(tob_rows(c, d, np.float32, f)[1])
    out["yard"] = {f: max([float(neighbour_err(g, r, PHI_TOB).max()) for g, r in zip(out["f32"][f], out["ref"])
                           if r.shape[2]] or [0.0]) for f in FORMS}
    return out


def tob_yardstick(family):
    """The family's float32 yardstick under the neighbour norm: the larger of forms (a) and (b), largest case."""
    return max(max(tob_expected(n)["yard"].values()) for n, c in tob_cases().items() if c["family"] == family)


@functools.lru_cache(maxsize=None)
def own_frame_yardstick():
    """The paired float32 statement's largest own-frame error over the quiet frames of the 2^-6 steps: the largest
    gap the engine leaves unequalised."""
    worst = 0.0
    for name, case in tob_cases().items():
        if "quiet" not in case:
            continue
        e = tob_expected(name)
        row = LEVEL_STEPS.index(6)
        for f in ("pair0", "pair1"):
            err = own_err(e["f32"][f][row][1], e["ref"][row][1])
            worst = max(worst, float(err[:, case["quiet"]].max()))
    return worst


# ------------------------------------------------------------------------------------------ front-end cases
FRONT_LENGTHS = (5248, 5375, 5376, 12544, 12545, 12671, 12672, 24832, 25089, 37001)
FRONT_SPEC_L = 25089                 # two segment seams inside the row
RAGGED = ((5248, 5376, 12545, 12672, 37001), (5375, 12544, 12671, 24832, 25089))
SEAM_FRAMES = (47, 48, 95, 96)
FRONT_FAMILIES = ("lengths", "spectra")


def _speech16(B, L, seed):
    c, n, _ = synthetic.speech_like_pairs(B, L, 16000, seed=seed)
    return c.numpy().copy(), n.numpy().copy()


@functools.lru_cache(maxsize=None)
def front_cases():
    """{name: {"family", "ref", "deg" [B, L] float32 (read-only)}}: both operands of the front end are rows of
    the case (the front end treats the 2 B signals alike)."""
    cases = {}
    for L in FRONT_LENGTHS:
        c, n = _speech16(1, L, seed=L % 1000)
        cases[f"len_{L}"] = dict(family="lengths", ref=c, deg=n)
    L = FRONT_SPEC_L
    c, n = _speech16(2, L, seed=21)
    t = np.arange(L) / 16000.0
    k_edge = int(_EDGES[20])                              # first bin of Bark band 20
    tone1k = 0.4 * np.sin(2 * np.pi * 1000.0 * t)
    tone_edge = 0.4 * np.sin(2 * np.pi * (k_edge - 0.5) * 16000.0 / 512 * t)   # on the edge between bands 19 and 20
    train = np.where(np.arange(L) % IMPULSE_PERIOD == 0, 0.8, 0.0)
    cases["spec"] = dict(family="spectra", ref=np.stack([c[0], c[1], c[0] + np.float32(0.5), _f32(tone1k)]),
                         deg=np.stack([n[0], n[1], _f32(tone_edge), _f32(train)]))
    for v in cases.values():
        for k in ("ref", "deg"):
            v[k] = _f32(v[k])
            v[k].setflags(write=False)
    return cases


FRONT_SPEC_ROWS = ("speech 0", "speech 1", "speech 0 + DC 0.5", "1 kHz tone", "noisy 0", "noisy 1", "band-edge tone",
                   "impulse train")


PRES = ("ta", "diff", "scan")


@functools.lru_cache(maxsize=None)
def front_expected(name):
    """{"power": [2B] float64, "bark": list over the 2 B signals (ref rows first) of [F, 49] float64, "f32_power":
    [2B], "f32": {(pre, form): list of [F, 49]}, "yard": {(pre, form): neighbour-norm error, bands 1..48},
    "yard_power", "yard_band0": largest absolute error of band 0}."""
    case = front_cases()[name]
    rows = list(case["ref"]) + list(case["deg"])
    keys = [(p, f) for p in PRES for f in FORMS]
    out = {"power": [], "bark": [], "f32_power": [], "f32": {k: [] for k in keys}}
    for r in rows:
        p, b = bark64(r)
        out["power"].append(p)
        out["bark"].append(b)
        for k in keys:
            p32, b32 = bark32(r, k[1], k[0])
            out["f32"][k].append(b32)
        out["f32_power"].append(float(p32))
    out["yard"] = {k: max(float(bark_err(g, r).max()) for g, r in zip(out["f32"][k], out["bark"])) for k in keys}
    out["yard_power"] = max(abs(a - b) / b for a, b in zip(out["f32_power"], out["power"]))
    out["yard_band0"] = max(float(np.abs(g[:, 0].astype(np.float64) - r[:, 0]).max())
                            for k in keys for g, r in zip(out["f32"][k], out["bark"]))
    return out


def bark_err(got, ref):
    """[F, 49] -> [48, F] neighbour-norm errors of bands 1..48."""
    return neighbour_err(np.asarray(got, np.float64).T[1:], np.asarray(ref, np.float64).T[1:], PHI_BARK)


def front_yardstick(family, pre="ta"):
    """(Bark yardstick under the neighbour norm with the ``pre`` pre-emphasis order, the larger of forms (a) and
    (b); power yardstick) of a family: its largest case's."""
    names = [n for n, c in front_cases().items() if c["family"] == family]
    return (max(v for n in names for k, v in front_expected(n)["yard"].items() if k[0] == pre),
            max(front_expected(n)["yard_power"] for n in names))


@functools.lru_cache(maxsize=None)
def front_band_yardstick(family):
    """[48]: per Bark band 1..48 the largest neighbour-norm error of any float32 statement (the three pre-emphasis
    orders, all transform forms) over the family, of the band and its two neighbours.  One figure for all bands
    would leave the upper bands unchecked: the float32 recursions lose the quiet low bands' digits (band 1: 6e-2
    sequential, 1e-2 restarted every 52 samples as pesq_front does; band 38: 2e-6 and 6e-6), and the restarts
    raise the floor under a clean row's bands 40..48 from 2e-4 to 8e-4.  A band's figure is one maximum over some
    thousand elements with a long tail; the neighbours even out its luck, the level itself varies slowly with
    the band."""
    worst = np.zeros(48)
    for n, c in front_cases().items():
        if c["family"] == family:
            e = front_expected(n)
            for k in e["f32"]:
                for g, r in zip(e["f32"][k], e["bark"]):
                    worst = np.maximum(worst, bark_err(g, r).max(1))
    pad = np.concatenate([worst[:1], worst, worst[-1:]])
    return np.maximum(np.maximum(pad[:-2], pad[1:-1]), pad[2:])
