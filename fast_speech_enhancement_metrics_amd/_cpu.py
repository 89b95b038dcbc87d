"""CPU mode of the metrics (``use_gpu=False``), the reference's CPU behaviour.

Batched torch/scipy implementation of the same math the HIP engine runs:
  PESQ: fast_se_metrics/PESQ.py:92-245, utils/bark.py:169-204, utils/loudness.py:48-67
  STOI: fast_se_metrics/STOI.py:26-205
The level-alignment band-pass runs as a float64 second-order-section cascade and the
pre-emphasis as a float64 IIR (scipy C loops); spectra via torch.stft.  STOI's
``normalize`` is deterministic here: its 1e-12 * randn term taken in expectation (zero-variance
rows map to 0, rows far below 1e-12 to ~0, as the engine and the oracle).
"""
from __future__ import annotations

import functools
import math
import threading

import numpy as np
import torch
from scipy.signal import butter, lfilter, sosfilt, tf2zpk, zpk2sos

from . import _tables as T

# ----------------------------------------------------------------------------- PESQ constants
_NB = 49
_EDGES = np.concatenate([[0], np.cumsum(T.BINS_PER_BAND)])
_FBANK = torch.zeros(_NB, 256, dtype=torch.float64)
for _i in range(_NB):
    _FBANK[_i, _EDGES[_i]:_EDGES[_i + 1]] = 1.0
_CORR = torch.tensor(T.POW_DENS_CORRECTION, dtype=torch.float64) * T.SP_16K
_THR = torch.tensor(T.ABS_THRESH_POWER, dtype=torch.float64)
_EXP = ((6 / (torch.tensor(T.CENTRE_BARK) + 2.0)).clamp(1.0, 2.0) ** 0.15 * T.ZWICKER_POWER).to(torch.float64)
_WB = torch.tensor(T.WIDTH_BARK, dtype=torch.float64)
_TW = float(_WB[1:].sum())
_bb, _ba = butter(5, [325, 3250], fs=16000, btype="band")
_BP_B = np.asarray(_bb, dtype=np.float32).astype(np.float64)
_BP_A = np.asarray(_ba, dtype=np.float32).astype(np.float64)
_z, _p, _k = tf2zpk(_BP_B, _BP_A)
# numerator is exactly g * (1 - z^-2)^5: place the zeros exactly at +-1
_z = np.array([1.0] * 5 + [-1.0] * 5)
_BP_SOS = zpk2sos(_z, _p, _BP_B[0])
_PRE_B = np.asarray(T.PRE_B, dtype=np.float32).astype(np.float64)
_PRE_A = np.asarray(T.PRE_A, dtype=np.float32).astype(np.float64)
_TAPER = torch.arange(1, 16, dtype=torch.float64) / 16.0


def pesq_frames(L: int) -> int:
    Lp = L + (L % 256)
    return 0 if Lp < 512 else 1 + (Lp - 512) // 256


def bandpass_power(x: np.ndarray) -> np.ndarray:
    """[N, L] -> [N] sum of the squared band-pass output (PESQ.py:94-97, before / (L+5120) / 1.04684)."""
    y = sosfilt(_BP_SOS, x, axis=1)
    return (y * y).sum(axis=1)


def level_scale(power_sum, L: int):
    """1e7 / (power / (L + 5120) / 1.04684): the factor on a row's power (PESQ.py:97-100)."""
    return 1e7 / (power_sum / (L + 5120) / 1.04684)


def pre_emphasize(x: np.ndarray) -> np.ndarray:
    """Edge taper (k/16 on the first and last 15 samples) + the pre-emphasis IIR (PESQ.py:104-113),
    on a copy."""
    x = np.array(x, dtype=np.float64)
    x[:, :15] *= _TAPER.numpy()
    x[:, -15:] *= _TAPER.numpy()[::-1]
    return lfilter(_PRE_B, _PRE_A, x, axis=1)


def power_spectrum(x: torch.Tensor) -> torch.Tensor:
    """[N, L] -> [N, F, 257]: pad by L % 256 (PESQ.py:128-130), Hann-512 / hop-256 |rFFT|^2, the
    DC bin zeroed (PESQ.py:133-136)."""
    pad = x.shape[1] % 256
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
    spec = torch.stft(x, n_fft=512, hop_length=256, win_length=512,
                      window=torch.hann_window(512, dtype=x.dtype, device=x.device),
                      center=False, return_complex=True).abs().square().transpose(1, 2)
    spec[:, :, 0] = 0.0
    return spec


def bark_bands(spec: torch.Tensor) -> torch.Tensor:
    """[N, F, 257] -> [N, F, 49] (bark.py:203-204)."""
    return torch.einsum("ij,klj->kli", _FBANK.to(spec.device), spec[:, :, :-1]) * _CORR.to(spec.device)


def bark_of_rows(x: torch.Tensor) -> torch.Tensor:
    """PESQ.get_bark_bands on [N, L] rows: level alignment, pre-emphasis, spectrum, Bark bands."""
    L = x.shape[1]
    xd = x.detach().to("cpu", torch.float64).numpy()
    xd = xd * np.sqrt(level_scale(bandpass_power(xd), L))[:, None]
    return bark_bands(power_spectrum(torch.from_numpy(pre_emphasize(xd))))


def equalize(c: torch.Tensor, n: torch.Tensor):
    """PESQ.equalize_bark_bands (PESQ.py:142-166) -> (equalised clean, equalised noisy)."""
    thr = _THR.to(c.device)
    silent = (c * (c > thr * 100.0)).sum(2) < 1e7
    keep = (~silent).unsqueeze(-1)
    mc = (c * ((c > thr * 100.0) & keep)).mean(1)
    mn = (n * ((n > thr * 100.0) & keep)).mean(1)
    ratio = ((mn + 1000.0) / (mc + 1000.0)).clamp(0.01, 100.0)
    ec = ratio.unsqueeze(1) * c
    fr = ((ec * (ec > thr)).sum(2) + 5e3) / ((n * (n > thr)).sum(2) + 5e3)
    fr2 = fr.clone()
    fr2[:, 1:] = 0.8 * fr[:, 1:] + 0.2 * fr[:, :-1]
    return ec, fr2.clamp(3e-4, 5.0).unsqueeze(-1) * n


def loudness(p: torch.Tensor) -> torch.Tensor:
    thr, ex = _THR.to(p.device), _EXP.to(p.device)
    v = (2.0 * thr) ** ex * ((0.5 + 0.5 * p / thr) ** ex - 1.0)
    return torch.where(p <= thr, torch.zeros_like(v), v) * T.SL_16K


def frame_disturbances(ec: torch.Tensor, en: torch.Tensor):
    """Per-frame symmetric / asymmetric disturbances after the frame weighting and the clamp at 45
    (PESQ.py:193-224) -> ([B, F], [B, F])."""
    wb = _WB.to(ec.device)
    lc, ln = loudness(ec), loudness(en)
    d = ln - lc
    d = d.sign() * (d.abs() - 0.25 * torch.minimum(lc, ln)).clamp(min=0)
    sym = (math.sqrt(_TW) * _Sqrt0.apply(((wb * d)[:, :, 1:] ** 2).sum(2))).clamp(min=1e-20)  # (same values)
    a = ((en + 50.0) / (ec + 50.0)) ** 1.2
    a = torch.where(a < 3.0, torch.zeros_like(a), a).clamp(max=12.0)
    asym = (wb * d * a)[:, :, 1:].abs().sum(2).clamp(min=1e-20)
    thr = _THR.to(ec.device)
    w = (((ec * (ec > thr)).sum(2) + 1e5) / 1e7) ** 0.04
    return (sym / w).clamp(max=45.0), (asym / w).clamp(max=45.0)


def overlapping_sums(v: torch.Tensor) -> torch.Tensor:
    """[B, F] -> [B]: L6 within 20-frame windows (hop 10), L2 across windows (PESQ.py:168-172)."""
    fr_ = v.unfold(1, 20, 10)
    return (fr_ ** 6).mean(2).pow(1.0 / 6.0).square().mean(1).sqrt()


def mos_of(sd: torch.Tensor, ad: torch.Tensor) -> torch.Tensor:
    """PESQ.py:240-243."""
    m = 4.5 - 0.1 * sd - 0.0309 * ad
    return 0.999 + 4.0 / (1.0 + torch.exp(-1.3669 * m + 3.8224))


def pesq_distances(clean: torch.Tensor, noisy: torch.Tensor):
    """PESQ.get_disturbances: [B, L] 16 kHz -> (symmetric, asymmetric) distances [B] float64."""
    B, L = clean.shape
    F = pesq_frames(L)
    if F < 20:
        raise RuntimeError(f"maximum size for tensor at dimension 1 is {max(F, 0)} but size is 20")
    bark = bark_of_rows(torch.cat([clean, noisy], 0))
    ec, en = equalize(bark[:B], bark[B:])
    sym, asym = frame_disturbances(ec, en)
    return overlapping_sums(sym), overlapping_sums(asym)


def pesq(clean: torch.Tensor, noisy: torch.Tensor) -> torch.Tensor:
    """[B, L] 16 kHz float32 -> MOS [B] float64."""
    return mos_of(*pesq_distances(clean, noisy))


class _BandPass(torch.autograd.Function):
    """The level band-pass of ``bandpass_power`` on [N, L] float64 rows from zero state; its adjoint is the
    same cascade run backwards in time from zero state at the row's end."""

    @staticmethod
    def forward(ctx, x):
        return torch.from_numpy(sosfilt(_BP_SOS, x.detach().numpy(), axis=1))

    @staticmethod
    def backward(ctx, g):
        return torch.from_numpy(sosfilt(_BP_SOS, g.numpy()[:, ::-1], axis=1)[:, ::-1].copy())


class _PreEmphasis(torch.autograd.Function):
    """The pre-emphasis IIR of ``pre_emphasize`` (without the taper) and its adjoint, as _BandPass."""

    @staticmethod
    def forward(ctx, x):
        return torch.from_numpy(lfilter(_PRE_B, _PRE_A, x.detach().numpy(), axis=1))

    @staticmethod
    def backward(ctx, g):
        return torch.from_numpy(lfilter(_PRE_B, _PRE_A, g.numpy()[:, ::-1], axis=1)[:, ::-1].copy())


def pesq_differentiable(clean: torch.Tensor, noisy: torch.Tensor):
    """[B, L] 16 kHz -> (MOS, symmetric distance, asymmetric distance) [B] float64: ``pesq`` as a function
    of the denoised rows under torch's autograd (include/fsem.h, "PESQ with gradients").  The clean rows
    are constants; every decision (audible and silent masks, dead zone, a < 3) is a constant, every clamp
    passes the gradient inside its range, a zero symmetric disturbance takes the subgradient 0."""
    B, L = clean.shape
    F = pesq_frames(L)
    if F < 20:
        raise RuntimeError(f"maximum size for tensor at dimension 1 is {max(F, 0)} but size is 20")
    bc = bark_of_rows(clean)
    y = noisy.to("cpu", torch.float64)
    u = _BandPass.apply(y)
    y = y * level_scale((u * u).sum(1), L).sqrt()[:, None]
    w = torch.ones(L, dtype=torch.float64)
    w[:15] *= _TAPER
    w[-15:] *= _TAPER.flip(0)
    y = _PreEmphasis.apply(y * w)
    if L % 256:
        y = torch.nn.functional.pad(y, (0, L % 256))
    z = torch.fft.rfft(y.unfold(1, 512, 256) * torch.hann_window(512, dtype=torch.float64), dim=2)
    keep = torch.ones(257, dtype=torch.float64)
    keep[0] = 0.0
    ec, en = equalize(bc, bark_bands((z.real.square() + z.imag.square()) * keep))
    sym, asym = frame_disturbances(ec, en)
    sd, ad = overlapping_sums(sym), overlapping_sums(asym)
    return mos_of(sd, ad), sd, ad


# ----------------------------------------------------------------------------- STOI
_SW = torch.hann_window(257)[1:].to(torch.float64)


def _obm() -> torch.Tensor:
    freqs = torch.linspace(0, 5000, 257, dtype=torch.float64)
    k = torch.arange(15, dtype=torch.float64)
    lo = 150 * torch.pow(2.0, (2 * k - 1) / 6)
    hi = 150 * torch.pow(2.0, (2 * k + 1) / 6)
    m = torch.zeros(15, 257, dtype=torch.float64)
    for i in range(15):
        m[i, int(torch.argmin((freqs - lo[i]).abs())):int(torch.argmin((freqs - hi[i]).abs()))] = 1
    return m


_OBM = _obm()
_CLIP = 1 + 10 ** (15 / 20)


def _norm(v: torch.Tensor, dim: int) -> torch.Tensor:
    """STOI.py:113-119 in expectation over its 1e-12 * randn term: the squared norm gains
    N * 1e-24 (N = the normalised dimension's size), the noise averages out of the products."""
    v = v - v.mean(dim=dim, keepdim=True)
    return v / torch.sqrt(v.square().sum(dim=dim, keepdim=True) + v.shape[dim] * 1e-24)


def _estoi_norm(seg: torch.Tensor) -> torch.Tensor:
    """Time, then band normalisation of [S, 15, 30] segments (STOI.py:178-181) in expectation over
    both noise terms: the band normalisation's norm also takes the noise the time normalisation
    left in each element (variance 1e-24 / its row's squared norm, x 14/15 after centring)."""
    c = seg - seg.mean(dim=2, keepdim=True)
    n2 = c.square().sum(dim=2, keepdim=True) + 30e-24
    a = c / n2.sqrt()
    a = a - a.mean(dim=1, keepdim=True)
    q = a.square().sum(dim=1, keepdim=True) + (14 / 15) * (1e-24 / n2).sum(dim=1, keepdim=True) + 15e-24
    return a / q.sqrt()


def stoi_segments(clean: torch.Tensor) -> torch.Tensor:
    """[B] int64: the 30-frame segments of each 10 kHz clean row, kept frames - 31 (0: the row scores NaN)."""
    x = clean.detach().to(torch.float64)
    if x.shape[1] < 256:
        return torch.zeros(x.shape[0], dtype=torch.int64)
    e = 20 * torch.log10((x.unfold(1, 256, 128) * _SW).norm(dim=2) + 1e-9)
    keep = (e.amax(1, keepdim=True) - 40 - e) < 0
    return (keep.sum(1) - 31).clamp(min=0)


def resample64(x: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """[B, n] -> [B, ceil(new n / orig)] float64: the package's resampler (resample.sinc_kernel's float32
    taps) applied in float64, differentiable under autograd."""
    x = x.to(torch.float64)
    if int(orig_freq) == int(new_freq):
        return x
    from .resample import sinc_kernel
    kern, width, orig, new = sinc_kernel(orig_freq, new_freq)
    n = x.shape[1]
    xp = torch.nn.functional.pad(x, (width, width + orig))
    res = torch.nn.functional.conv1d(xp[:, None], kern.to(torch.float64)[:, None], stride=orig)
    return res.transpose(1, 2).reshape(x.shape[0], -1)[:, :-(-new * n // orig)]


class _Sqrt0(torch.autograd.Function):
    """torch.sqrt with the subgradient 0 at 0 (torch's own derivative there is inf, and NaN once it meets
    a zero): the band envelopes of an all-zero estimate get a zero, finite gradient.  Same values."""

    @staticmethod
    def forward(ctx, p):
        s = torch.sqrt(p)
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return torch.where(s > 0, g / (2 * s), torch.zeros_like(g))


def stoi(clean: torch.Tensor, noisy: torch.Tensor):
    """[B, L10] 10 kHz -> (stoi [B], estoi [B]) float64; NaN where no 30-frame segment exists.
    Differentiable with respect to ``noisy`` under autograd (the selection of frames is the clean
    rows'), with the subgradient 0 where a band envelope is 0."""
    B = clean.shape[0]
    out_s = torch.full((B,), float("nan"), dtype=torch.float64)
    out_e = torch.full((B,), float("nan"), dtype=torch.float64)
    x = clean.to(torch.float64)
    y = noisy.to(torch.float64)
    if x.shape[1] < 256:
        raise RuntimeError("STOI input shorter than one 256-sample frame at 10 kHz")
    xf = x.unfold(1, 256, 128) * _SW
    yf = y.unfold(1, 256, 128) * _SW
    e = 20 * torch.log10(xf.norm(dim=2) + 1e-9)
    keep = (e.amax(1, keepdim=True) - 40 - e) < 0
    win512 = torch.zeros(512, dtype=torch.float64)
    win512[128:384] = _SW
    for b in range(B):
        kx, ky = xf[b][keep[b]], yf[b][keep[b]]
        n = kx.shape[0]
        nseg = n - 31
        if nseg <= 0:
            continue
        length = (n + 1) * 128
        ox = torch.zeros(length, dtype=torch.float64)
        oy = torch.zeros(length, dtype=torch.float64)
        idx = (128 * torch.arange(n)[:, None] + torch.arange(256)[None, :]).reshape(-1)
        ox.index_add_(0, idx, kx.reshape(-1))
        oy.index_add_(0, idx, ky.reshape(-1))
        sp = torch.stft(torch.stack([ox, oy]), n_fft=512, hop_length=128, win_length=512, window=win512,
                        center=False, return_complex=True).abs().square()            # [2, 257, T]
        tob = _Sqrt0.apply(torch.matmul(_OBM, sp))                                    # [2, 15, T]
        segs = tob.unfold(2, 30, 1)[:, :, :nseg]                                      # [2, 15, S, 30]
        cx, cy = segs[0].transpose(0, 1), segs[1].transpose(0, 1)                     # [S, 15, 30]
        alpha = cx.norm(dim=2, keepdim=True) / (cy.norm(dim=2, keepdim=True) + 1e-9)
        yc = torch.minimum(cy * alpha, cx * _CLIP)
        out_s[b] = (_norm(cx, 2) * _norm(yc, 2)).sum() / 15 / nseg
        out_e[b] = (_estoi_norm(cx) * _estoi_norm(cy)).sum() / 30 / nseg
    return out_s, out_e


# torch's intra-op thread count is process-wide: concurrent _host_map calls (metric calls from
# several Python threads) share one save / restore, counted under a lock -- the first call in
# saves the caller's setting and sets 1, the last call out restores it.
_threads_lock = threading.Lock()
_threads_depth = 0
_threads_saved = 1


def _threads_enter() -> int:
    """Pool size for a row map (the caller's thread count); torch's intra-op threads -> 1."""
    global _threads_depth, _threads_saved
    with _threads_lock:
        if _threads_depth == 0:
            _threads_saved = torch.get_num_threads()
            torch.set_num_threads(1)
        _threads_depth += 1
        return _threads_saved


def _threads_exit() -> None:
    global _threads_depth
    with _threads_lock:
        _threads_depth -= 1
        if _threads_depth == 0:
            torch.set_num_threads(_threads_saved)


def host_threads() -> int:
    """torch's intra-op thread count as the caller set it (not the 1 of a row map in flight)."""
    with _threads_lock:
        return _threads_saved if _threads_depth > 0 else torch.get_num_threads()


def _host_map(fn, items):
    """[fn(item) for item in items] on up to host_threads() host threads, torch's own intra-op
    parallelism set to 1 meanwhile (rows are independent; scipy's filters and torch's kernels
    release the GIL, so row chunks run concurrently: 2.5x for PESQ and 1.4x for STOI on 8 cores
    against one call with 8 intra-op threads)."""
    items = list(items)
    if min(host_threads(), len(items)) <= 1:
        return [fn(it) for it in items]
    from concurrent.futures import ThreadPoolExecutor
    nt = min(_threads_enter(), len(items))
    try:
        with ThreadPoolExecutor(max(nt, 1)) as ex:
            return list(ex.map(fn, items))
    finally:
        _threads_exit()


def _cat(outs):
    if isinstance(outs[0], tuple):
        return tuple(torch.cat([o[i] for o in outs]) for i in range(len(outs[0])))
    return torch.cat(outs)


def rows_parallel(fn, clean: torch.Tensor, noisy: torch.Tensor):
    """fn(clean, noisy) -> [B] tensor(s), computed over contiguous row chunks on the host's
    threads (one chunk per thread) and concatenated in row order."""
    B = clean.shape[0]
    nt = max(1, min(host_threads(), B))
    bounds = [(i * B // nt, (i + 1) * B // nt) for i in range(nt)]
    return _cat(_host_map(lambda lh: fn(clean[lh[0]:lh[1]], noisy[lh[0]:lh[1]]), bounds))


def per_row(fn, clean: torch.Tensor, noisy: torch.Tensor, lengths: torch.Tensor):
    """Variable-length CPU mode: ``fn`` on each unpadded row alone (batching.py); rows ``fn``
    rejects as too short score NaN.  Returns what ``fn`` returns, stacked over rows."""
    def one(b):
        n = int(lengths[b])
        try:
            return fn(clean[b:b + 1, :n], noisy[b:b + 1, :n])
        except RuntimeError:
            return None

    outs = _host_map(one, range(clean.shape[0]))
    proto = next((o for o in outs if o is not None), None)
    if proto is None:
        proto = torch.zeros(1, dtype=torch.float64) if fn is pesq else (torch.zeros(1, dtype=torch.float64),) * 2
    nan = float("nan")
    if isinstance(proto, tuple):
        return tuple(torch.cat([o[i] if o is not None else torch.full((1,), nan, dtype=torch.float64) for o in outs])
                     for i in range(len(proto)))
    return torch.cat([o if o is not None else torch.full((1,), nan, dtype=torch.float64) for o in outs])


# ----------------------------------------------------------------------------- time alignment
# The opt-in P.862-style delay estimation (not in the reference, PESQ.py:19-22; engine:
# csrc/align.hip, which documents the stages), float64 with FFT cross-correlations.
_TA_FRAME, _TA_FINE, _TA_ITERS = 64, 383, 12


def _ta_envelope(x: np.ndarray) -> np.ndarray:
    nfr = x.shape[0] // _TA_FRAME
    e = np.square(x[:nfr * _TA_FRAME].reshape(nfr, _TA_FRAME)).sum(axis=1)
    if nfr == 0:
        return e
    thr = e.mean()
    for _ in range(_TA_ITERS):
        sel = e <= thr
        if not sel.any():
            break
        mu = e[sel].mean()
        thr = 1.001 * (mu + 2.0 * math.sqrt(np.square(e[sel] - mu).mean()))
    return np.where(e > thr, np.log(np.maximum(e, 1e-300) / max(thr, 1e-300)), 0.0)


def _xcorr_window(a: np.ndarray, b: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """c[j - lo] = sum_k a[k] b[k + j] for lags lo <= j <= hi (zero outside the arrays)."""
    from scipy.signal import correlate
    n = a.shape[0]
    full = correlate(b, a, mode="full", method="fft")  # full[j + n - 1] = sum_k a[k] b[k + j]
    out = np.zeros(hi - lo + 1)
    j = np.arange(lo, hi + 1)
    ok = (j > -n) & (j < b.shape[0])
    out[ok] = full[j[ok] + n - 1]
    return out


def _first_max(c: np.ndarray) -> int:
    """Index of the first maximum above zero, or -1."""
    i = int(np.argmax(c)) if c.size else 0
    return i if c.size and c[i] > 0 else -1


def time_align_row(ref: np.ndarray, deg: np.ndarray, max_delay: int) -> int:
    r = np.asarray(ref, dtype=np.float64)
    d = np.asarray(deg, dtype=np.float64)
    er, ed = _ta_envelope(r), _ta_envelope(d)
    nfr = er.shape[0]
    M = min(-(-max_delay // _TA_FRAME), nfr - 1)
    jc = 0
    if M >= 0 and nfr > 0:
        i = _first_max(_xcorr_window(er, ed, -M, M))
        jc = i - M if i >= 0 else 0
    d0 = _TA_FRAME * jc
    L = r.shape[0]
    wr = np.zeros(L)
    wd = np.zeros(L)
    wr[1:] = np.diff(r)
    wd[1:] = np.diff(d)
    i = _first_max(_xcorr_window(wr, wd, d0 - _TA_FINE, d0 + _TA_FINE))
    return d0 - _TA_FINE + i if i >= 0 else d0


# utterance mode (csrc/align.hip stages 5-9; P.862 sections 10.3-10.5)
_TA_MINSPEECH, _TA_JOIN, _TA_MINUTT, _TA_SEARCH, _TA_MAXU, _TA_CHUNK = 4, 50, 50, 75, 16, 5120
_TA_SPLIT_GAIN, _TA_SPLIT_MIN = 1.2, 16


def _ta_utterances(env: np.ndarray) -> list:
    """[(start, end)] frames: speech runs from MINSPEECH frames, joined across gaps < JOIN, kept
    from MINUTT, at most MAXU."""
    act = np.flatnonzero(env > 0)
    utt = []
    if act.size:
        cut = np.flatnonzero(np.diff(act) > 1)
        rs = np.concatenate([[act[0]], act[cut + 1]])
        re = np.concatenate([act[cut] + 1, [act[-1] + 1]])
        keep = re - rs >= _TA_MINSPEECH
        rs, re = rs[keep], re[keep]
        if rs.size:
            cut = np.flatnonzero(rs[1:] - re[:-1] >= _TA_JOIN)  # a gap of JOIN or more starts a new run
            starts = np.concatenate([[rs[0]], rs[cut + 1]])
            ends = np.concatenate([re[cut], [re[-1]]])
            utt = [(int(a), int(b)) for a, b in zip(starts, ends) if b - a >= _TA_MINUTT]
    if len(utt) > _TA_MAXU:
        utt = utt[:_TA_MAXU - 1] + [(utt[_TA_MAXU - 1][0], utt[-1][1])]
    return utt


def _ta_piece_xcorr(wr, wd, a: int, b: int, lo: int, hi: int) -> np.ndarray:
    """c[D - lo] = sum over n in [a, b) of wr[n] wd[n + D], lo <= D <= hi (wd zero outside)."""
    L = wd.shape[0]
    win = np.zeros(b - a + hi - lo)
    s0 = a + lo
    i0, i1 = max(s0, 0), min(s0 + win.shape[0], L)
    if i1 > i0:
        win[i0 - s0:i1 - s0] = wd[i0:i1]
    return _xcorr_window(wr[a:b], win, 0, hi - lo) if b > a else np.zeros(hi - lo + 1)


# P.862 mode (csrc/align.hip stages 10-12; P.862 sections 10.5-10.6 on the fine stage's pieces)
_TA_HIST_T, _TA_HIST_POW, _TA_REL_MIN, _TA_MAXDEPTH, _TA_MAXSEG = 8, 0.125, 0.05, 2, 32


def _ta_hist(pv: np.ndarray, pl: np.ndarray, a: int, b: int, d0: int):
    """(delay, confidence, voting pieces) of pieces [a, b): the first maximum of the triangle-
    smoothed histogram of the voting pieces' peak lags, weighted by peak^0.125."""
    sel = np.flatnonzero(pl[a:b] >= 0) + a
    if sel.size == 0:
        return d0, 0.0, 0
    H = np.zeros(2 * _TA_FINE + 1)
    for i in sel:  # piece order, as the engine adds them
        H[pl[i]] += pv[i] ** _TA_HIST_POW
    k = np.arange(-_TA_HIST_T, _TA_HIST_T + 1)
    S = np.convolve(H, (_TA_HIST_T + 1 - np.abs(k)).astype(np.float64), mode="same")
    j = int(np.argmax(S))
    return d0 - _TA_FINE + j, float(S[j] / ((_TA_HIST_T + 1) * H.sum())), int(sel.size)


def _ta_split_p862(pv, pl, a: int, b: int, d0: int, depth: int) -> list:
    """[(piece offset from a, delay)]: pieces [a, b) split where both halves (two or more voting
    pieces each) disagree by SPLIT_MIN and are more confident than the whole, recursively."""
    D, c, _ = _ta_hist(pv, pl, a, b, d0)
    if depth < _TA_MAXDEPTH and b - a >= 4:
        best = None
        for sp in range(a + 2, b - 1):
            dL, cL, nL = _ta_hist(pv, pl, a, sp, d0)
            dR, cR, nR = _ta_hist(pv, pl, sp, b, d0)
            ok = nL >= 2 and nR >= 2 and abs(dL - dR) >= _TA_SPLIT_MIN and cL > c and cR > c
            if ok and (best is None or cL + cR > best[0]):
                best = (cL + cR, sp)
        if best is not None:
            sp = best[1]
            right = _ta_split_p862(pv, pl, sp, b, d0, depth + 1)
            return _ta_split_p862(pv, pl, a, sp, d0, depth + 1) + [(sp - a + o, d) for o, d in right]
    return [(0, D)]


def time_align_utt_row(ref: np.ndarray, deg: np.ndarray, max_delay: int, mode: str = "utterance"):
    """(seg_start [n+1], seg_delay [n], row delay) of one row (csrc/align.hip, utterance or P.862
    mode)."""
    r = np.asarray(ref, dtype=np.float64)
    d = np.asarray(deg, dtype=np.float64)
    L = r.shape[0]
    er, ed = _ta_envelope(r), _ta_envelope(d)
    nfr = er.shape[0]
    M = min(-(-max_delay // _TA_FRAME), nfr - 1) if nfr >= 2 else 0
    jrow = 0
    if nfr >= 2:
        i = _first_max(_xcorr_window(er, ed, -M, M))
        jrow = i - M if i >= 0 else 0
    utt = _ta_utterances(er)
    R = [0] + [_TA_FRAME * ((utt[u - 1][1] + utt[u][0]) // 2) for u in range(1, len(utt))] + [L]
    wins = utt if utt else [(0, nfr)]
    wr = np.zeros(L)
    wd = np.zeros(L)
    wr[1:] = np.diff(r)
    wd[1:] = np.diff(d)
    starts, delays = [], []
    for u, (s, e) in enumerate(wins):
        k0, k1 = max(0, s - _TA_SEARCH), min(nfr, e + _TA_SEARCH)
        jlo, jhi = max(-M, jrow - _TA_SEARCH), min(M, jrow + _TA_SEARCH)
        best, arg = 0.0, None
        for j in range(jlo, jhi + 1):
            ks, ke = max(k0, -j), min(k1, nfr - j)
            c = float(np.dot(er[ks:ke], ed[ks + j:ke + j])) if ke > ks else 0.0
            if c > best:
                best, arg = c, j
        d0 = _TA_FRAME * (arg if arg is not None else jrow)
        m = max(1, -(-(R[u + 1] - R[u]) // _TA_CHUNK))
        P = np.stack([_ta_piece_xcorr(wr, wd, R[u] + i * _TA_CHUNK, min(R[u] + (i + 1) * _TA_CHUNK, R[u + 1]),
                                      d0 - _TA_FINE, d0 + _TA_FINE) for i in range(m)])
        if mode == "p862":
            pl = np.array([_first_max(P[i]) for i in range(m)])
            pv = np.array([P[i, j] if j >= 0 else 0.0 for i, j in enumerate(pl)])
            pl[pv < _TA_REL_MIN * pv.max()] = -1
            for off, D in _ta_split_p862(pv, pl, 0, m, d0, 0):
                if not (delays and delays[-1] == D) and len(delays) < _TA_MAXSEG:
                    starts.append(R[u] + off * _TA_CHUNK)
                    delays.append(D)
            continue
        W = P.sum(axis=0)
        iW = _first_max(W)
        segs = [(0, d0 - _TA_FINE + iW if iW >= 0 else d0)]
        if m >= 4:
            left = np.cumsum(P, axis=0)
            cand = []
            for sp in range(2, m - 1):
                lf, rt = left[sp - 1], W - left[sp - 1]
                iL, iR = _first_max(lf), _first_max(rt)
                vL, vR = (lf[iL] if iL >= 0 else 0.0), (rt[iR] if iR >= 0 else 0.0)
                cand.append((vL + vR, sp, vL, iL, vR, iR))
            tot, sp, vL, iL, vR, iR = max(cand, key=lambda t: t[0])  # first maximum
            vW = W[iW] if iW >= 0 else 0.0
            if vL > 0 and vR > 0 and tot > _TA_SPLIT_GAIN * vW and abs(iL - iR) >= _TA_SPLIT_MIN:
                segs = [(0, d0 - _TA_FINE + iL), (sp * _TA_CHUNK, d0 - _TA_FINE + iR)]
        for off, D in segs:
            if not (delays and delays[-1] == D):
                starts.append(R[u] + off)
                delays.append(D)
    starts.append(L)
    lens = np.diff(starts)
    return np.array(starts), np.array(delays), int(delays[int(np.argmax(lens))])


def time_align_utterances(clean: torch.Tensor, noisy: torch.Tensor, lengths=None, max_delay: int = 16000,
                          mode: str = "utterance"):
    """(aligned [B, L] f32, delays [B], n_seg [B], seg_start [B, 33], seg_delay [B, 32]) int32."""
    c = clean.detach().cpu().numpy()
    n = noisy.detach().cpu().numpy()
    B, L = c.shape
    S = 2 * _TA_MAXU
    out = np.zeros((B, L), dtype=np.float32)
    ds = np.zeros(B, dtype=np.int32)
    ns = np.zeros(B, dtype=np.int32)
    st = np.zeros((B, S + 1), dtype=np.int32)
    sd = np.zeros((B, S), dtype=np.int32)
    rows = [L if lengths is None else int(min(max(int(lengths[b]), 0), L)) for b in range(B)]
    res = _host_map(lambda b: time_align_utt_row(c[b, :rows[b]], n[b, :rows[b]], max_delay, mode), range(B))
    for b, (starts, delays, D) in enumerate(res):
        k = len(delays)
        ns[b], ds[b] = k, D
        st[b, :k + 1] = starts
        sd[b, :k] = delays
        for i in range(k):
            a, e, Dk = int(starts[i]), int(starts[i + 1]), int(delays[i])
            lo, hi = max(a, -Dk), min(e, rows[b] - Dk)
            if hi > lo:
                out[b, lo:hi] = n[b, lo + Dk:hi + Dk]
    return tuple(torch.from_numpy(x) for x in (out, ds, ns, st, sd))


def time_align(clean: torch.Tensor, noisy: torch.Tensor, lengths=None, max_delay: int = 16000):
    """(aligned noisy [B, L] float32, delays [B] int32) of 16 kHz rows (rows past lengths[b] 0)."""
    c = clean.detach().cpu().numpy()
    n = noisy.detach().cpu().numpy()
    B, L = c.shape
    out = np.zeros((B, L), dtype=np.float32)
    ds = np.zeros(B, dtype=np.int32)
    rows = [L if lengths is None else int(min(max(int(lengths[b]), 0), L)) for b in range(B)]
    ds[:] = _host_map(lambda b: time_align_row(c[b, :rows[b]], n[b, :rows[b]], max_delay), range(B))
    for b in range(B):
        m, D = rows[b], int(ds[b])
        lo, hi = max(0, -D), min(m, m - D)
        if hi > lo:
            out[b, lo:hi] = n[b, lo + D:hi + D]
    return torch.from_numpy(out), torch.from_numpy(ds)


# bad intervals (csrc/align.hip ta_bad_*; P.862 section 10.7): the P.862 mode's realignment of
# runs of badly scored frames, then the pooling over the better-scored frames
_BAD_THR, _BAD_GAP, _BAD_MIN, _BAD_MAX, _HOP = 30.0, 4, 5, 16, 256


def bad_runs(sym: np.ndarray) -> list:
    """[(f0, f1)]: runs of frames above BAD_THR, joined across gaps < BAD_GAP, from BAD_MIN
    frames, at most BAD_MAX in order."""
    bad = np.flatnonzero(np.asarray(sym) > _BAD_THR)
    if bad.size == 0:
        return []
    cut = np.flatnonzero(np.diff(bad) > 1)
    rs = np.concatenate([[bad[0]], bad[cut + 1]])
    re = np.concatenate([bad[cut] + 1, [bad[-1] + 1]])
    j = np.flatnonzero(rs[1:] - re[:-1] >= _BAD_GAP)
    s = np.concatenate([[rs[0]], rs[j + 1]])
    e = np.concatenate([re[j], [re[-1]]])
    return [(int(a), int(b)) for a, b in zip(s, e) if b - a >= _BAD_MIN][:_BAD_MAX]


def pesq_frame_scores(clean: torch.Tensor, noisy: torch.Tensor):
    """Per-frame (symmetric, asymmetric) disturbances [B, F] of [B, L] 16 kHz rows."""
    B = clean.shape[0]
    bark = bark_of_rows(torch.cat([clean, noisy], 0))
    ec, en = equalize(bark[:B], bark[B:])
    return frame_disturbances(ec, en)


def realign_bad_row(ref: np.ndarray, deg: np.ndarray, aligned: np.ndarray, starts, delays, sym: np.ndarray):
    """([(f0, f1, delay)], second degraded row) of one unpadded row."""
    L = deg.shape[0]
    out = np.array(aligned, dtype=np.float32, copy=True)
    runs = bad_runs(sym)
    if not runs:
        return [], out
    wr = np.zeros(L)
    wd = np.zeros(L)
    wr[1:] = np.diff(np.asarray(ref, dtype=np.float64))
    wd[1:] = np.diff(np.asarray(deg, dtype=np.float64))
    res = []
    for f0, f1 in runs:
        a, e = _HOP * f0, min(_HOP * f1 + _HOP, L)
        k = int(np.searchsorted(starts, a, side="right")) - 1
        d0 = int(delays[min(max(k, 0), len(delays) - 1)])
        i = _first_max(_ta_piece_xcorr(wr, wd, a, e, d0 - _TA_FINE, d0 + _TA_FINE))
        D = d0 - _TA_FINE + i if i >= 0 else d0
        res.append((f0, f1, D))
        lo, hi = max(a, -D), min(e, L - D)
        out[a:e] = 0.0
        if hi > lo:
            out[lo:hi] = deg[lo + D:hi + D]
    return res, out


def pesq_p862_row(ref: np.ndarray, deg: np.ndarray, aligned: np.ndarray, starts, delays):
    """(MOS, [(f0, f1, delay)]) of one unpadded row already aligned by the P.862 mode."""
    L = ref.shape[0]
    if pesq_frames(L) < 20:
        return float("nan"), []
    c = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)).unsqueeze(0)
    s1, a1 = pesq_frame_scores(c, torch.from_numpy(np.ascontiguousarray(aligned, dtype=np.float32)).unsqueeze(0))
    res, second = realign_bad_row(ref, deg, aligned, starts, delays, s1[0].numpy())
    if res:
        s2, a2 = pesq_frame_scores(c, torch.from_numpy(second).unsqueeze(0))
        s1, a1 = s1.clone(), a1.clone()
        for f0, f1, _ in res:
            if float(s2[0, f0:f1].sum()) < float(s1[0, f0:f1].sum()):
                s1[0, f0:f1] = s2[0, f0:f1]
                a1[0, f0:f1] = a2[0, f0:f1]
    return float(mos_of(overlapping_sums(s1), overlapping_sums(a1))[0]), res


def pesq_p862(clean: torch.Tensor, noisy: torch.Tensor, lengths=None, max_delay: int = 16000):
    """(MOS [B] float64, delays [B] int32, n_bad [B] int32, bad [B, 16, 3] int32) of 16 kHz rows:
    the P.862-mode alignment, then the bad-interval realignment."""
    aligned, ds, ns, st, sd = time_align_utterances(clean, noisy, lengths, max_delay, mode="p862")
    c = clean.detach().cpu().float().numpy()
    n = noisy.detach().cpu().float().numpy()
    a = aligned.numpy()
    B, L = c.shape
    rows = [L if lengths is None else int(min(max(int(lengths[b]), 0), L)) for b in range(B)]

    def one(b):
        k = int(ns[b])
        m = rows[b]
        return pesq_p862_row(c[b, :m], n[b, :m], a[b, :m], st[b, :k + 1].numpy(), sd[b, :k].numpy())

    res = _host_map(one, range(B))
    mos = torch.tensor([r[0] for r in res], dtype=torch.float64)
    nb = torch.zeros(B, dtype=torch.int32)
    bad = torch.zeros(B, _BAD_MAX, 3, dtype=torch.int32)
    for b, (_, iv) in enumerate(res):
        nb[b] = len(iv)
        if iv:
            bad[b, :len(iv)] = torch.tensor(iv, dtype=torch.int32)
    return mos, ds, nb, bad


# ----------------------------------------------------------------------------- SDR family
# SI-SDR, SNR and segmental SNR (not in the reference; engine: csrc/sdr.hip, definitions:
# include/fsem.h "SDR"), float64.
def sdr_geometry(sample_rate: int):
    """(hop, win) of the segmental SNR at ``sample_rate``: 7.5 ms hop, 30 ms window."""
    hop = int(sample_rate) * 30 // 4000
    return hop, 4 * hop


def sdr(clean: torch.Tensor, noisy: torch.Tensor, sample_rate: int = 16000, zero_mean: bool = False):
    """[B, n] rows at ``sample_rate`` -> (si_sdr [B], snr [B], seg_snr [B]) float64, in dB."""
    B, n = clean.shape
    nan = torch.full((B,), float("nan"), dtype=torch.float64)
    if n == 0:
        return nan, nan.clone(), nan.clone()
    s = clean.to(torch.float64)
    h = noisy.to(torch.float64)
    d = h - s
    dd = d.square().sum(1)
    snr = 10 * torch.log10(s.square().sum(1) / dd)
    s0, h0 = (s - s.mean(1, keepdim=True), h - h.mean(1, keepdim=True)) if zero_mean else (s, h)
    ss, sh, hh = s0.square().sum(1), (s0 * h0).sum(1), h0.square().sum(1)
    tt = sh / ss * sh
    si = 10 * torch.log10(tt / (hh - tt).clamp_min(0))
    si = torch.where(dd == 0, torch.full_like(si, float("inf")), si)
    si = torch.where((ss == 0) | (hh == 0), nan, si)
    hop, win = sdr_geometry(sample_rate)
    if n >= win:
        t = torch.arange(1, win + 1, dtype=torch.float64)
        w = 0.5 * (1 - torch.cos(2 * math.pi * t / (win + 1)))
        es = (s.unfold(1, win, hop) * w).square().sum(2)
        ed = (d.unfold(1, win, hop) * w).square().sum(2)
        seg = (10 * torch.log10(es / (ed + 1e-10) + 1e-10)).clamp(-10, 35).mean(1)
    else:
        seg = nan.clone()
    bad = ~(torch.isfinite(s).all(1) & torch.isfinite(h).all(1))
    return tuple(torch.where(bad, nan, v) for v in (si, snr, seg))


# ----------------------------------------------------------------------------- LSD
# Log-spectral distance (the reference's LSD.py:32-52; engine: csrc/lsd.hip, definition:
# include/fsem_lsd.h), float64 inside.
def lsd(clean: torch.Tensor, noisy: torch.Tensor) -> torch.Tensor:
    """[B, n] 16 kHz rows -> lsd [B] float32.  The reference's operations (scale, centred 512-point
    STFT with hop 256 and a periodic Hann window, log ratio, root mean square over bins, mean over
    frames) on float64 copies of the rows, on the rows' device; n = 0 is one all-zero frame."""
    s = clean.to(torch.float64)
    h = noisy.to(torch.float64)
    a = (s * h).sum(1, keepdim=True) / (h.square().sum(1, keepdim=True) + 1e-8)
    x = torch.nn.functional.pad(torch.cat([s, h * a]), (256, 256))  # center=True, pad_mode="constant"
    w = torch.hann_window(512, dtype=torch.float64, device=x.device)
    mag = torch.stft(x, n_fft=512, hop_length=256, window=w, center=False, return_complex=True).abs()
    S, H = mag[:s.shape[0]], mag[s.shape[0]:]
    v = torch.log(S.square() / (H + 1e-8).square() + 1e-8).square().mean(1).sqrt().mean(1)
    return v.to(torch.float32)


def lsd64(clean: torch.Tensor, noisy: torch.Tensor) -> torch.Tensor:
    """[B, n] 16 kHz rows -> lsd [B] float64, differentiable with respect to ``noisy`` under autograd:
    ``lsd``'s operations with the magnitudes as roots of re^2 + im^2.  Both roots (the estimate's
    magnitude, the frame's value) take the subgradient 0 at 0 (``_Sqrt0``), as the engine's backward: a
    silent estimate frame, or a silent estimate, gets an exactly zero gradient."""
    s = clean.to(torch.float64)
    h = noisy.to(torch.float64)
    B = s.shape[0]
    a = (s * h).sum(1, keepdim=True) / (h.square().sum(1, keepdim=True) + 1e-8)
    x = torch.nn.functional.pad(torch.cat([s, h * a]), (256, 256))
    w = torch.hann_window(512, dtype=torch.float64, device=x.device)
    z = torch.view_as_real(torch.stft(x, n_fft=512, hop_length=256, window=w, center=False, return_complex=True))
    S2 = z[:B].square().sum(-1)
    H = _Sqrt0.apply(z[B:].square().sum(-1))
    t = torch.log(S2 / (H + 1e-8).square() + 1e-8)
    return _Sqrt0.apply(t.square().mean(1)).mean(1)


# ----------------------------------------------------------------------------- BSS-eval SDR
# The reference's SDR (SDR.py:7-97; engine: csrc/bsssdr.hip, definition: include/fsem_bsssdr.h):
# float32 normalisation as the reference's, then float64: linear correlations for 512 lags and a
# Levinson-Durbin recursion for the Toeplitz system, written out (no linalg.solve, no Cholesky).
def bsssdr(clean: torch.Tensor, noisy: torch.Tensor, load_diag=None, filter_length: int = 512) -> torch.Tensor:
    """[B, n] 16 kHz rows -> SDR [B] float32 in dB.  NaN for a row whose system is singular (a silent
    clean row, n = 0, a prediction error <= 0) or that holds a non-finite sample; all rows of the
    chunk advance through the recursion together."""
    K = filter_length
    B, n = clean.shape
    nan = torch.full((B,), float("nan"), dtype=torch.float32, device=clean.device)
    if n == 0 or B == 0:
        return nan
    s32, h32 = clean.to(torch.float32), noisy.to(torch.float32)
    finite = torch.isfinite(s32).all(1) & torch.isfinite(h32).all(1)
    s32 = torch.where(finite[:, None], s32, torch.zeros_like(s32))
    h32 = torch.where(finite[:, None], h32, torch.zeros_like(h32))
    # the norms in double, rounded to float32; the clamp and the quotient in float32
    ns = s32.double().square().sum(1).sqrt().float().clamp(min=1e-6)
    nh = h32.double().square().sum(1).sqrt().float().clamp(min=1e-6)
    s = (s32 / ns[:, None]).double()
    h = (h32 / nh[:, None]).double()
    nfft = 1 << (n + K - 1).bit_length()  # >= n + K: no wrap-around within K lags
    Sf = torch.fft.rfft(s, n=nfft)
    r = torch.fft.irfft(Sf.abs().square(), n=nfft)[:, :K].contiguous()
    b = torch.fft.irfft(Sf.conj() * torch.fft.rfft(h, n=nfft), n=nfft)[:, :K].contiguous()
    if load_diag is not None:
        r[:, 0] += float(load_diag)
    x, bad = _toeplitz_solve(r, b, ~finite | ~(r[:, 0] > 0))
    coh = (b * x).sum(1)
    ratio = coh / (1.0 - coh).clamp(min=1e-8)
    val = (10.0 * torch.log10(ratio.clamp(min=1e-8))).to(torch.float32)
    return torch.where(bad | ~torch.isfinite(coh), nan, val)


def _toeplitz_solve(r: torch.Tensor, b: torch.Tensor, bad: torch.Tensor):
    """(x [B, K] with R x = b for R[i][j] = r[|i - j|], bad [B]) by the Levinson-Durbin recursion for a
    general right-hand side; ``bad`` marks the rows given as bad and those whose prediction error is <= 0
    at any order (their x is arbitrary but finite arithmetic)."""
    B, K = r.shape
    r0 = torch.where(bad, torch.ones_like(r[:, 0]), r[:, 0])
    E = r0.clone()
    a = torch.zeros(B, K, dtype=torch.float64, device=r.device)  # the predictor [1, a1, ..., am]
    a[:, 0] = 1.0
    x = torch.zeros_like(a)
    x[:, 0] = b[:, 0] / r0
    for m in range(1, K):
        rr = r[:, 1:m + 1].flip(1)  # r[m - i], i = 0 ... m - 1
        acc = (a[:, :m] * rr).sum(1)
        q = (x[:, :m] * rr).sum(1)
        k = -acc / E
        a[:, :m + 1] = a[:, :m + 1] + k[:, None] * a[:, :m + 1].flip(1)
        E = E * (1.0 - k * k)
        bad = bad | ~(E > 0)
        E = torch.where(bad, torch.ones_like(E), E)  # (a row already NaN: keep the arithmetic finite)
        lam = (b[:, m] - q) / E
        x[:, :m + 1] = x[:, :m + 1] + lam[:, None] * a[:, :m + 1].flip(1)
    return x, bad


def bsssdr64(clean: torch.Tensor, noisy: torch.Tensor, load_diag=None) -> torch.Tensor:
    """[1, n] 16 kHz rows -> SDR [1] float64 in dB, differentiable with respect to ``noisy`` under autograd
    (include/fsem.h, "BSS-eval SDR with gradients"); NaN without a graph for a row ``bsssdr`` scores NaN.
    The value is taken at the float32 quotients q = h / nh of ``bsssdr``; the estimate enters the graph as
    h' = q + (d - q (q . d)) / nh with d = h - h.detach() (zero), i.e. with the Jacobian (I - q q^T) / nh of
    the normalisation (d / nh where the norm sits at its clamp).  The system is solved without a graph (the
    recursion writes in place) and coh = 2 b(h') . x - x . R x: at R x = b its value is b . x and its
    gradient the definition's, 2 x . db."""
    K = 512
    n = clean.shape[1]
    nan = torch.full((1,), float("nan"), dtype=torch.float64)
    s32, h32 = clean.detach().to(torch.float32), noisy.detach().to(torch.float32)
    if n == 0 or not bool(torch.isfinite(s32).all() and torch.isfinite(h32).all()):
        return nan
    ns = s32.double().square().sum(1).sqrt().float().clamp(min=1e-6)
    nh_raw = h32.double().square().sum(1).sqrt().float()
    nh = nh_raw.clamp(min=1e-6)
    s = (s32 / ns[:, None]).double()
    q = (h32 / nh[:, None]).double()
    d = noisy.to(torch.float64) - noisy.detach().to(torch.float64)
    if bool(nh_raw < 1e-6):
        h = q + d / nh.double()
    else:
        h = q + (d - q * (q * d).sum(1, keepdim=True)) / nh.double()
    nfft = 1 << (n + K - 1).bit_length()
    Sf = torch.fft.rfft(s, n=nfft)
    r = torch.fft.irfft(Sf.abs().square(), n=nfft)[:, :K].contiguous()
    b = torch.fft.irfft(Sf.conj() * torch.fft.rfft(h, n=nfft), n=nfft)[:, :K]
    if load_diag is not None:
        r[:, 0] += float(load_diag)
    with torch.no_grad():
        x, bad = _toeplitz_solve(r, b.detach().contiguous(), ~(r[:, 0] > 0))
        lag = torch.arange(K)
        xRx = (x[0] * (r[0][(lag[:, None] - lag[None, :]).abs()] @ x[0])).sum()
        if bool(bad) or not bool(torch.isfinite((b * x).sum())):
            return nan
    coh = 2.0 * (b * x).sum(1) - xRx
    ratio = coh / (1.0 - coh).clamp(min=1e-8)
    return 10.0 * torch.log10(ratio.clamp(min=1e-8))


# ----------------------------------------------------------------------------- BSS-eval of mixtures
# SDR, SIR and SAR of E estimates against S sources (include/fsem.h "BSS-eval"; engine:
# csrc/bsseval.hip): float32 normalisation, then float64 FFT correlations, the dense Gram matrix
# of the sources' 512 delays and a Cholesky factorisation per mixture.
BSSEVAL_MAX_SOURCES = 4
BSSEVAL_CRITERIA = {None: 0, "SIR": 1, "SDR": 2}


def _bsseval_mixture(s: torch.Tensor, h: torch.Tensor, K: int = 512):
    """(coh [S, E], coh_all [E]) float64 of one unpadded mixture ([S, n] sources, [E, n] estimates);
    all NaN by the NaN rule."""
    S, n = s.shape
    E = h.shape[0]
    nan = float("nan")
    bad = (torch.full((S, E), nan, dtype=torch.float64), torch.full((E,), nan, dtype=torch.float64))
    s32, h32 = s.to(torch.float32), h.to(torch.float32)
    if n + K - 1 < S * K or not (bool(torch.isfinite(s32).all()) and bool(torch.isfinite(h32).all())):
        return bad

    def unit(x):  # the norm in double, rounded to float32; the clamp and the quotient in float32
        nrm = x.double().square().sum(1).sqrt().float().clamp(min=1e-6)
        return (x / nrm[:, None]).double()

    nfft = 1 << (n + K - 1).bit_length()  # >= n + K: no wrap-around within K lags
    Sf = torch.fft.rfft(unit(s32), n=nfft)
    Hf = torch.fft.rfft(unit(h32), n=nfft)
    C = torch.fft.irfft(Sf.conj()[:, None] * Sf[None], n=nfft)[..., :K]  # C[i, j, k]
    b = torch.fft.irfft(Sf.conj()[:, None] * Hf[None], n=nfft)[..., :K]  # b[i, e, k]
    if not all(bool(C[i, i, 0] > 0) for i in range(S)):
        return bad
    full = torch.cat([C.transpose(0, 1).flip(2)[..., :-1], C], 2)  # lags -(K - 1) ... K - 1: C_ij[-k] = C_ji[k]
    lag = torch.arange(K)[:, None] - torch.arange(K)[None, :] + K - 1
    G = full[:, :, lag].permute(0, 2, 1, 3).reshape(S * K, S * K)  # G[(i, k), (j, l)] = C_ij[k - l]
    d = b.permute(0, 2, 1).reshape(S * K, E)

    def energy(M, rhs):
        L, info = torch.linalg.cholesky_ex(M)
        if int(info) != 0:
            return None
        y = torch.linalg.solve_triangular(L, rhs, upper=False)
        return (y * y).sum(0)

    coh = [energy(G[i * K:(i + 1) * K, i * K:(i + 1) * K], d[i * K:(i + 1) * K]) for i in range(S)]
    if any(c is None for c in coh):
        return bad
    coh = torch.stack(coh)
    coh_all = energy(G, d) if S > 1 else coh[0].clone()
    if coh_all is None or not bool(torch.isfinite(coh).all() and torch.isfinite(coh_all).all()):
        return bad
    return coh, coh_all


def bsseval(sources: torch.Tensor, estimates: torch.Tensor, lengths=None):
    """[B, S, n] sources, [B, E, n] estimates (16 kHz) -> (coh [B, S, E], coh_all [B, E]) float64, the
    energies of the estimates' projections on each source's and on all sources' 512 delays; mixtures
    run on the host's threads.  ``lengths``: [B] ints, mixture b holds lengths[b] samples."""
    B, S, n = sources.shape
    E = estimates.shape[1]
    lens = [n] * B if lengths is None else [int(v) for v in lengths]
    outs = _host_map(lambda m: _bsseval_mixture(sources[m, :, :lens[m]], estimates[m, :, :lens[m]]), range(B))
    if not B:
        return torch.zeros(0, S, E, dtype=torch.float64), torch.zeros(0, E, dtype=torch.float64)
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def bsseval_scores(coh: torch.Tensor, coh_all: torch.Tensor, criterion=None):
    """(sdr, sir, sar [B, E] float32, perm [B, E] int32, sdr_mat, sir_mat [B, S, E] float32) from the
    energies: the clamped ratios in dB and, with criterion "SIR" or "SDR" and E == S, the assignment
    with the largest mean (the first of equal ones in itertools.permutations order)."""
    import itertools
    if criterion not in BSSEVAL_CRITERIA:
        raise ValueError(f"permutation must be one of {list(BSSEVAL_CRITERIA)}, not {criterion!r}")
    B, S, E = coh.shape

    def db(num, den):
        return 10.0 * torch.log10((num / den.clamp(min=1e-8)).clamp(min=1e-8))

    ca = coh_all[:, None, :]
    sd, si, sa = db(coh, 1.0 - coh), db(coh, ca - coh), db(coh_all, 1.0 - coh_all)
    bad = torch.isnan(coh).flatten(1).any(1) | torch.isnan(coh_all).any(1)
    perm = torch.arange(E, dtype=torch.int32).repeat(B, 1)
    if criterion is not None and S == E:
        crit = (si if criterion == "SIR" else sd).tolist()
        for m in range(B):
            if bool(bad[m]):
                continue
            best = None
            for p in itertools.permutations(range(S)):
                v = sum(crit[m][p[e]][e] for e in range(S)) / S
                if best is None or v > best:
                    best, arg = v, p
            perm[m] = torch.tensor(arg, dtype=torch.int32)
    idx = perm.long()[:, None, :]
    nan = torch.full((), float("nan"), dtype=torch.float64)
    sdr = torch.where(bad[:, None], nan, sd.gather(1, idx)[:, 0])
    sir = torch.where(bad[:, None], nan, si.gather(1, idx)[:, 0])
    sar = torch.where(bad[:, None], nan, sa)
    sd = torch.where(bad[:, None, None], nan, sd)
    si = torch.where(bad[:, None, None], nan, si)
    return (sdr.float(), sir.float(), sar.float(), perm, sd.float(), si.float())


# ----------------------------------------------------------------------------- PITSDR
# SI-SDR and SNR of every (source, estimate) pair of a mixture and the assignment (not in the
# reference; engine: csrc/pitsdr.hip, definition: include/fsem.h "PITSDR"), float64 torch ops on the
# whole batch: differentiable with respect to the estimates by torch's own autograd.
PITSDR_MAX_SOURCES = 4
PITSDR_CRITERIA = {None: 0, "SI-SDR": 1, "SNR": 2}


def pitsdr(sources: torch.Tensor, estimates: torch.Tensor, lengths=None, zero_mean: bool = False, criterion=None):
    """[B, S, L] sources, [B, E, L] estimates -> (si_mat, snr_mat [B, S, E] float64, perm [B, E] int32).
    ``lengths``: [B] ints, mixture b holds lengths[b] samples.  The gradient of a NaN or +-inf entry
    is whatever autograd makes of it (the engine leaves such pairs out)."""
    import itertools
    if criterion not in PITSDR_CRITERIA:
        raise ValueError(f"permutation must be one of {list(PITSDR_CRITERIA)}, not {criterion!r}")
    B, S, L = sources.shape
    E = estimates.shape[1]
    s, h = sources.to(torch.float64), estimates.to(torch.float64)
    n = torch.full((B,), L, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths).to(torch.int64)
    n = n.clamp(0, L)
    keep = (torch.arange(L)[None, :] < n[:, None])[:, None, :]  # [B, 1, L]
    zero = torch.zeros((), dtype=torch.float64)
    s, h = torch.where(keep, s, zero), torch.where(keep, h, zero)
    bad = ~(torch.isfinite(s).all(2).all(1) & torch.isfinite(h).all(2).all(1)) | (n == 0)
    dd = torch.stack([(h - s[:, i:i + 1]).square().sum(2) for i in range(S)], 1)  # [B, S, E]
    snr = 10 * torch.log10(s.square().sum(2)[:, :, None] / dd)
    if zero_mean:
        cnt = n.clamp(min=1)[:, None, None]
        s = torch.where(keep, s - s.sum(2, keepdim=True) / cnt, zero)
        h = torch.where(keep, h - h.sum(2, keepdim=True) / cnt, zero)
    ss, hh = s.square().sum(2)[:, :, None], h.square().sum(2)[:, None, :]
    sh = torch.einsum("bil,bel->bie", s, h)
    tt = sh / ss * sh
    si = 10 * torch.log10(tt / (hh - tt).clamp_min(0))
    nan = torch.full((), float("nan"), dtype=torch.float64)
    si = torch.where(dd == 0, torch.full((), float("inf"), dtype=torch.float64), si)
    si = torch.where((ss == 0) | (hh == 0) | bad[:, None, None], nan, si)
    snr = torch.where(bad[:, None, None], nan, snr)
    perm = torch.arange(E, dtype=torch.int32).repeat(B, 1)
    if criterion is not None and S == E:
        mat = (si if criterion == "SI-SDR" else snr).detach()
        ok = ~torch.isnan(mat).flatten(1).any(1)
        crit = mat.tolist()
        for m in range(B):
            if not bool(ok[m]):
                continue
            best = None
            for p in itertools.permutations(range(S)):
                v = sum(crit[m][p[e]][e] for e in range(S)) / S
                if best is None or v > best:
                    best, arg = v, p
            perm[m] = torch.tensor(arg, dtype=torch.int32)
    return si, snr, perm


# ----------------------------------------------------------------------------- Composite family
# CSIG, CBAK, COVL with LLR and WSS (Hu & Loizou 2008; not in the reference; engine:
# csrc/composite.hip, definitions: include/fsem_composite.h), float64, all frames of a chunk of
# rows at once.
_WSS_CENTRE = (50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38,
               1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17,
               3597.63)
_WSS_WIDTH = (70.0,) * 7 + (77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457,
                            199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136)
_COMPOSITE_ROWS = 8  # rows per vectorised pass (bounds the [rows, F, win] temporaries)


def composite_order(sample_rate: int) -> int:
    """LPC order of the LLR: 10 at 8 kHz, 16 at 16 kHz."""
    return 10 if int(sample_rate) < 10000 else 16


@functools.lru_cache(maxsize=4)
def _wss_filters(sample_rate: int, nfft: int) -> torch.Tensor:
    """[25, nfft / 2] float64 critical-band filters."""
    H = nfft // 2
    half = sample_rate / 2
    j = torch.arange(H, dtype=torch.float64)
    rows = []
    for c, b in zip(_WSS_CENTRE, _WSS_WIDTH):
        f0 = math.floor(c * H / half)
        g = torch.exp(-11.0 * ((j - f0) / (b * H / half)) ** 2 + math.log(_WSS_WIDTH[0]) - math.log(b))
        rows.append(torch.where(g > math.exp(-30.0 / (2 * 2.303)), g, torch.zeros_like(g)))
    return torch.stack(rows)


def _lpc(R: torch.Tensor, P: int) -> torch.Tensor:
    """Levinson-Durbin on [..., P + 1] autocorrelations -> prediction-error filters [..., P + 1]."""
    a = torch.zeros_like(R)
    a[..., 0] = 1.0
    E = R[..., 0].clone()
    for i in range(1, P + 1):
        acc = R[..., i] + (a[..., 1:i] * R[..., 1:i].flip(-1)).sum(-1)
        k = -acc / E
        prev = a[..., 1:i].clone()
        a[..., 1:i] = prev + k[..., None] * prev.flip(-1)
        a[..., i] = k
        E = E * (1 - k * k)
    return a


def _nearest_peaks(e: torch.Tensor) -> torch.Tensor:
    """[..., 25] band energies -> [..., 24] nearest peaks (the published search, its quirk kept)."""
    sl = e[..., 1:] - e[..., :-1]
    nb = sl.shape[-1]
    up = sl > 0
    down = sl <= 0
    # first m >= i that does not rise (24 when every later slope rises)
    nxt = torch.full(sl.shape, nb, dtype=torch.int64)
    cur = torch.full(sl.shape[:-1], nb, dtype=torch.int64)
    for i in range(nb - 1, -1, -1):
        cur = torch.where(up[..., i], cur, torch.full_like(cur, i))
        nxt[..., i] = cur
    # last m <= i that does not fall (-1 when every earlier slope falls)
    prv = torch.full(sl.shape, -1, dtype=torch.int64)
    cur = torch.full(sl.shape[:-1], -1, dtype=torch.int64)
    for i in range(nb):
        cur = torch.where(down[..., i], cur, torch.full_like(cur, i))
        prv[..., i] = cur
    at = torch.where(up, nxt - 1, prv + 1)
    return torch.gather(e, -1, at)


def _trimmed_mean(v: torch.Tensor) -> torch.Tensor:
    """[B, F] -> [B]: the mean of the K = (19 F + 10) // 20 smallest, NaN sorting last."""
    F = v.shape[1]
    if F == 0:
        return torch.full((v.shape[0],), float("nan"), dtype=torch.float64)
    K = (19 * F + 10) // 20
    return torch.sort(v, dim=1).values[:, :K].mean(1)


def _llr_wss_seg(s: torch.Tensor, h: torch.Tensor, sample_rate: int):
    """(llr, wss, seg_snr) [B] float64 of [B, n] float64 rows, n >= win."""
    hop, win = sdr_geometry(sample_rate)
    P = composite_order(sample_rate)
    nfft = 1 << (2 * win - 1).bit_length()
    t = torch.arange(1, win + 1, dtype=torch.float64)
    w = 0.5 * (1 - torch.cos(2 * math.pi * t / (win + 1)))
    fs = s.unfold(1, win, hop) * w
    fh = h.unfold(1, win, hop) * w
    fd = (h - s).unfold(1, win, hop) * w
    seg = (10 * torch.log10(fs.square().sum(2) / (fd.square().sum(2) + 1e-10) + 1e-10)).clamp(-10, 35).mean(1)
    Rs = torch.stack([(fs[..., :win - k] * fs[..., k:]).sum(-1) for k in range(P + 1)], -1)
    Rh = torch.stack([(fh[..., :win - k] * fh[..., k:]).sum(-1) for k in range(P + 1)], -1)
    As, Ah = _lpc(Rs, P), _lpc(Rh, P)
    lag = (torch.arange(P + 1)[:, None] - torch.arange(P + 1)[None, :]).abs()
    Tm = Rs[..., lag]  # [B, F, P + 1, P + 1]
    quad = lambda A: torch.einsum("bfi,bfij,bfj->bf", A, Tm, A)  # noqa: E731
    llr = torch.log(quad(Ah) / quad(As))
    G = _wss_filters(int(sample_rate), nfft)
    H = nfft // 2
    es = 10 * torch.log10((torch.fft.rfft(fs, nfft).abs().square()[..., :H] @ G.T).clamp_min(1e-10))
    eh = 10 * torch.log10((torch.fft.rfft(fh, nfft).abs().square()[..., :H] @ G.T).clamp_min(1e-10))

    def weights(e):
        return 20 / (20 + e.max(-1, keepdim=True).values - e[..., :-1]) / (1 + _nearest_peaks(e) - e[..., :-1])

    W = (weights(es) + weights(eh)) / 2
    dsl = (es[..., 1:] - es[..., :-1]) - (eh[..., 1:] - eh[..., :-1])
    wss = (W * dsl.square()).sum(-1) / W.sum(-1)
    return _trimmed_mean(llr), _trimmed_mean(wss), seg


def composite(clean: torch.Tensor, noisy: torch.Tensor, sample_rate: int = 16000, short_ok: bool = False):
    """[B, n] rows at ``sample_rate`` (8000 or 16000) -> (csig, cbak, covl, pesq, llr, wss, seg_snr),
    [B] float64 each.  Rows too short for PESQ: RuntimeError as ``pesq``, or NaN in pesq and the
    composites with ``short_ok``."""
    B, n = clean.shape
    nan = torch.full((B,), float("nan"), dtype=torch.float64)
    if n == 0:
        return tuple(nan.clone() for _ in range(7))
    c16, n16 = clean.to(torch.float32), noisy.to(torch.float32)
    if int(sample_rate) != 16000:
        from .resample import Resample
        rs = Resample(int(sample_rate), 16000)
        c16, n16 = rs(c16), rs(n16)
    if pesq_frames(c16.shape[1]) < 20 and short_ok:
        mos = nan.clone()
    else:
        mos = pesq(c16, n16)
    s = clean.to(torch.float64)
    h = noisy.to(torch.float64)
    hop, win = sdr_geometry(sample_rate)
    if n >= win:
        parts = [_llr_wss_seg(s[i:i + _COMPOSITE_ROWS], h[i:i + _COMPOSITE_ROWS], sample_rate)
                 for i in range(0, B, _COMPOSITE_ROWS)]
        llr, wss, seg = (torch.cat([p[k] for p in parts]) for k in range(3))
    else:
        llr, wss, seg = nan.clone(), nan.clone(), nan.clone()
    csig = (3.093 - 1.029 * llr + 0.603 * mos - 0.009 * wss).clamp(1, 5)
    cbak = (1.634 + 0.478 * mos - 0.007 * wss + 0.063 * seg).clamp(1, 5)
    covl = (1.594 + 0.805 * mos - 0.512 * llr - 0.007 * wss).clamp(1, 5)
    bad = ~(torch.isfinite(s).all(1) & torch.isfinite(h).all(1))
    return tuple(torch.where(bad, nan, v) for v in (csig, cbak, covl, mos, llr, wss, seg))


# ----------------------------------------------------------------------------- Spectral measures
# fwSegSNR, CD and IS (Hu & Loizou's evaluation set; not in the reference; engine:
# csrc/spectral.hip, definitions: include/fsem.h "Spectral"), float64, all frames of a chunk of rows
# at once.  Composite's frames, window, LPC order and band filters.
def spectral_frames(s: torch.Tensor, h: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """[3, B, F] float64 frame values (fwSegSNR_f, CD_f, IS_f) of [B, n] float64 rows, n >= win."""
    hop, win = sdr_geometry(sample_rate)
    P = composite_order(sample_rate)
    nfft = 1 << (2 * win - 1).bit_length()
    H = nfft // 2
    t = torch.arange(1, win + 1, dtype=torch.float64, device=s.device)
    w = 0.5 * (1 - torch.cos(2 * math.pi * t / (win + 1)))
    fs = s.unfold(1, win, hop) * w
    fh = h.unfold(1, win, hop) * w
    Rs = torch.stack([(fs[..., :win - k] * fs[..., k:]).sum(-1) for k in range(P + 1)], -1)
    Rh = torch.stack([(fh[..., :win - k] * fh[..., k:]).sum(-1) for k in range(P + 1)], -1)
    As, Ah = _lpc(Rs, P), _lpc(Rh, P)
    lag = (torch.arange(P + 1)[:, None] - torch.arange(P + 1)[None, :]).abs().to(s.device)
    Ts, Th = Rs[..., lag], Rh[..., lag]  # [B, F, P + 1, P + 1]
    quad = lambda A, Tm: torch.einsum("bfi,bfij,bfj->bf", A, Tm, A)  # noqa: E731
    Es, Eh = quad(As, Ts), quad(Ah, Th)
    is_f = (quad(Ah, Ts) / Eh + torch.log(Eh / Es) - 1).clamp(max=100)

    def cepstrum(A):
        c = [torch.zeros_like(A[..., 0])]
        for m in range(1, P + 1):
            acc = sum((k * c[k] * A[..., m - k] for k in range(1, m)), torch.zeros_like(A[..., 0]))
            c.append(-A[..., m] - acc / m)
        return torch.stack(c[1:], -1)

    cd_f = (10 / math.log(10) * torch.sqrt(2 * (cepstrum(As) - cepstrum(Ah)).square().sum(-1))).clamp(max=10)
    G = _wss_filters(int(sample_rate), nfft).to(s.device)

    def band_sums(fr):
        M = torch.fft.rfft(fr, nfft).abs()[..., :H]
        tot = M.sum(-1, keepdim=True)
        return torch.where(tot > 0, M / tot, torch.zeros_like(M)) @ G.T

    es, eh = band_sums(fs), band_sums(fh)
    err = (es - eh).square().clamp_min(2.0 ** -52)
    W = es ** 0.2
    on = W > 0
    term = torch.where(on, W * 10 * torch.log10(torch.where(on, es.square() / err, torch.ones_like(es))),
                       torch.zeros_like(W))
    den = W.sum(-1)
    fw_f = torch.where(den > 0, (term.sum(-1) / den).clamp(-10, 35), torch.full_like(den, float("nan")))
    return torch.stack([fw_f, cd_f, is_f])


def spectral(clean: torch.Tensor, noisy: torch.Tensor, sample_rate: int = 16000, return_frames: bool = False):
    """[B, n] rows at ``sample_rate`` (8000 or 16000) -> (fwsegsnr, cd, is), [B] float64 each; with
    ``return_frames`` also the [3, B, F] float64 frame values.  Torch ops on the rows' device."""
    B, n = clean.shape
    hop, win = sdr_geometry(sample_rate)
    F = (n - win) // hop + 1 if n >= win else 0
    nan = torch.full((B,), float("nan"), dtype=torch.float64, device=clean.device)
    if F == 0 or B == 0:
        out = (nan, nan.clone(), nan.clone())
        return out + (torch.zeros(3, B, 0, dtype=torch.float64, device=clean.device),) if return_frames else out
    s = clean.to(torch.float64)
    h = noisy.to(torch.float64)
    fr = torch.cat([spectral_frames(s[i:i + _COMPOSITE_ROWS], h[i:i + _COMPOSITE_ROWS], sample_rate)
                    for i in range(0, B, _COMPOSITE_ROWS)], 1)
    bad = ~(torch.isfinite(s).all(1) & torch.isfinite(h).all(1))
    out = tuple(torch.where(bad, nan, v) for v in (fr[0].mean(1), _trimmed_mean(fr[1]), _trimmed_mean(fr[2])))
    return out + (fr,) if return_frames else out


# ----------------------------------------------------------------------------- SRMR
# The speech-to-reverberation modulation energy ratio (include/fsem.h "SRMR"; engine:
# csrc/srmr.hip) in float64: scipy's lfilter for the gammatone's four first-order complex sections
# and for the eight modulation biquads.
SRMR_CHANNELS, SRMR_MODS = 23, 8
_SRMR_EARQ, _SRMR_MINBW = 9.26449, 24.7


def srmr_geometry(sample_rate: int):
    """(hop, window) in samples: 64 ms and 256 ms."""
    return math.ceil(0.064 * sample_rate), math.ceil(0.256 * sample_rate)


@functools.lru_cache(maxsize=4)
def _srmr_filters(sample_rate: int):
    """(poles p_i, gains g_i, ERB(cf_i)) of the 23 channels (descending cf), the 8 modulation
    filters' (b, a) and their lower band edges L_k."""
    fs = float(sample_rate)
    c = _SRMR_EARQ * _SRMR_MINBW
    i = np.arange(1, SRMR_CHANNELS + 1)
    cf = -c + np.exp(i * (np.log(125 + c) - np.log(fs / 2 + c)) / SRMR_CHANNELS) * (fs / 2 + c)
    erb = cf / _SRMR_EARQ + _SRMR_MINBW
    p = np.exp((-2 * np.pi * 1.019 * erb + 2j * np.pi * cf) / fs)

    def G(q):
        u = q * np.exp(-2j * np.pi * cf / fs)
        return u * (1 + 4 * u + u * u) / (1 - u) ** 4

    g = np.abs(G(p) + G(p.conj())) / 2
    mcf = 4.0 * 32.0 ** (np.arange(SRMR_MODS) / 7.0)
    W0 = np.tan(np.pi * mcf / fs)
    B0 = W0 / 2
    a = np.stack([1 + B0 + W0 ** 2, 2 * W0 ** 2 - 2, 1 - B0 + W0 ** 2], 1)
    b = np.stack([B0, np.zeros_like(B0), -B0], 1)
    return p, g, erb, b / a[:, :1], a / a[:, :1], mcf - B0 * fs / (2 * np.pi)


def srmr_energies(x: np.ndarray, sample_rate: int) -> np.ndarray:
    """A[i, k] of [B, n] float64 rows with at least one frame: [B, 23, 8]."""
    wi, wl = srmr_geometry(sample_rate)
    B, n = x.shape
    F = (n - wl) // wi + 1
    nend = (F - 1) * wi + wl
    p, g, _, mb, ma, _ = _srmr_filters(sample_rate)
    w2 = np.square(0.54 - 0.46 * np.cos(2 * np.pi * np.arange(wl) / wl))
    V = np.zeros(nend)
    for f in range(F):
        V[f * wi:f * wi + wl] += w2
    A = np.empty((B, SRMR_CHANNELS, SRMR_MODS))
    for i in range(SRMR_CHANNELS):
        y = lfilter(np.array([0, p[i], 4 * p[i] ** 2, p[i] ** 3]) / g[i], [1.0], x.astype(np.complex128), axis=-1)
        for _ in range(4):
            y = lfilter([1.0], [1.0, -p[i]], y, axis=-1)
        e = np.abs(y)
        for k in range(SRMR_MODS):
            m = lfilter(mb[k], ma[k], e, axis=-1)[:, :nend]
            A[:, i, k] = np.square(m) @ V / F
    return A


def srmr_bands(A: np.ndarray, sample_rate: int) -> np.ndarray:
    """K* of [B, 23, 8] energies: the 90 % bandwidth rule, [B] ints."""
    _, _, erb, _, _, L = _srmr_filters(sample_rate)
    out = np.empty(A.shape[0], dtype=np.int64)
    for b in range(A.shape[0]):
        ac = A[b].sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            cum = np.cumsum(100 * ac[::-1] / ac.sum())
            over = np.nonzero(cum > 90)[0]
            bw = erb[SRMR_CHANNELS - 1 - over[0]] if len(over) else erb[0]
            out[b] = 8 if bw > L[7] else 7 if bw > L[6] else 6 if bw > L[5] else 5
    return out


def srmr_score(A: np.ndarray, sample_rate: int) -> np.ndarray:
    """SRMR of [B, 23, 8] energies: the 90 % bandwidth rule and the ratio."""
    K = srmr_bands(A, sample_rate)
    out = np.full(A.shape[0], np.nan)
    for b in range(A.shape[0]):
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b] = A[b, :, :4].sum() / A[b, :, 4:K[b]].sum()
    return out


def srmr(rows: torch.Tensor, sample_rate: int = 16000, return_energies: bool = False):
    """[B, n] rows at ``sample_rate`` (8000 or 16000) -> SRMR, [B] float64; with
    ``return_energies`` also the [B, 23, 8] float64 energies A.  Rows without a frame or with a
    non-finite sample are NaN."""
    B, n = rows.shape
    wi, wl = srmr_geometry(sample_rate)
    score = torch.full((B,), float("nan"), dtype=torch.float64)
    A = torch.full((B, SRMR_CHANNELS, SRMR_MODS), float("nan"), dtype=torch.float64)
    if n >= wl and B:
        x = rows.detach().to("cpu", torch.float64).numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            a = srmr_energies(x, sample_rate)
            s = srmr_score(a, sample_rate)
        s[~np.isfinite(x).all(1)] = np.nan
        score, A = torch.from_numpy(s), torch.from_numpy(a)
    return (score, A) if return_energies else score


def srmr_gradient(x: np.ndarray, sample_rate: int, A: np.ndarray, g: np.ndarray) -> np.ndarray:
    """d (sum_b g[b] SRMR_b) / dx of [B, n] float64 rows with at least one frame, given their energies A: the
    closed form of include/fsem.h "SRMR with gradients", K* taken as a constant.  Every adjoint recurrence
    is lfilter on the reversed row.  Rows whose score is not finite get zeros."""
    wi, wl = srmr_geometry(sample_rate)
    B, n = x.shape
    F = (n - wl) // wi + 1
    nend = (F - 1) * wi + wl
    p, gain, _, mb, ma, _ = _srmr_filters(sample_rate)
    w2 = np.square(0.54 - 0.46 * np.cos(2 * np.pi * np.arange(wl) / wl))
    V = np.zeros(nend)
    for f in range(F):
        V[f * wi:f * wi + wl] += w2
    K = srmr_bands(A, sample_rate)
    c = np.zeros((B, SRMR_MODS))
    for b in range(B):
        N, D = A[b, :, :4].sum(), A[b, :, 4:K[b]].sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            if np.isfinite(np.float32(N / D)):
                c[b, :4] = g[b] / D
                c[b, 4:K[b]] = -g[b] * N / (D * D)
    dx = np.zeros((B, n))
    if not c.any():
        return dx
    for i in range(SRMR_CHANNELS):
        taps = np.array([0, p[i], 4 * p[i] ** 2, p[i] ** 3]) / gain[i]
        y = lfilter(taps, [1.0], x.astype(np.complex128), axis=-1)
        for _ in range(4):
            y = lfilter([1.0], [1.0, -p[i]], y, axis=-1)
        e = np.abs(y)
        de = np.zeros((B, nend))
        for k in range(SRMR_MODS):
            if not c[:, k].any():
                continue
            m = lfilter(mb[k], ma[k], e, axis=-1)[:, :nend]
            q = (2.0 * c[:, k, None] / F) * m * V
            # r[t] = q[t] - a1 r[t + 1] - a2 r[t + 2], then b0 (r[t] - r[t + 2]): the filter itself, reversed
            de += lfilter(mb[k], ma[k], q[:, ::-1], axis=-1)[:, ::-1]
        a = np.zeros((B, n), dtype=np.complex128)
        live = e[:, :nend] > 0
        a[:, :nend] = np.where(live, de * y[:, :nend] / np.where(live, e[:, :nend], 1.0), 0.0)  # |y| = 0: 0
        a = a[:, ::-1]
        for _ in range(4):
            a = lfilter([1.0], [1.0, -np.conj(p[i])], a, axis=-1)
        dx += np.real(lfilter(np.conj(taps), [1.0], a, axis=-1))[:, ::-1]
    return dx


class _Srmr64(torch.autograd.Function):
    """SRMR [B] float64 of [B, n] float64 rows; the backward is srmr_gradient on the saved rows and energies."""

    @staticmethod
    def forward(ctx, rows, sample_rate):
        score, A = srmr(rows, sample_rate, return_energies=True)
        ctx.rows, ctx.A, ctx.sample_rate = rows.detach(), A, sample_rate
        return score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        rows, sr = ctx.rows, ctx.sample_rate
        B, n = rows.shape
        grad = torch.zeros(B, n, dtype=torch.float64)
        x = rows.to(torch.float64).numpy()
        ok = np.isfinite(x).all(1) if n else np.zeros(B, dtype=bool)
        if n >= srmr_geometry(sr)[1] and ok.any():
            with np.errstate(invalid="ignore", over="ignore"):
                dx = srmr_gradient(x[ok], sr, ctx.A.numpy()[ok], g.to(torch.float64).numpy()[ok])
            grad[torch.from_numpy(ok)] = torch.from_numpy(np.ascontiguousarray(dx))
        return grad, None


def srmr64(rows: torch.Tensor, sample_rate: int = 16000) -> torch.Tensor:
    """SRMR [B] float64 of [B, n] float64 host rows, as ``srmr``, carrying the gradient with respect to the
    rows (include/fsem.h "SRMR with gradients"): an autograd function of its own around the closed form.
    A row without a frame, with a non-finite sample or with a non-finite score gets a zero gradient row."""
    return _Srmr64.apply(rows.to(torch.float64), int(sample_rate))


# ----------------------------------------------------------------------------- DNSMOS
# The reference's DNSMOS network (DNSMOS.py) in float32 torch ops from the checkpoint's tensors
# (a dict of state-dict names -> float32 CPU tensors); engine: csrc/dnsmos.hip.
DNSMOS_SEGMENT, DNSMOS_HOP = 144160, 16000
_DNSMOS_POLY = ((0.0052439, -0.39604546, 0.04602535), (1.22083953, 1.60915514, 1.11546468),
                (-0.08397278, -0.13166888, -0.06766283))
_DNSMOS_POOL_AFTER = (6, 9, 12)  # max-pool follows conv_layers.6, .9 and .12


def dnsmos_segments(n: int) -> int:
    """Segments of a row of n samples: the row doubled until it holds 144160 samples, then
    (n' - 144160) // 16000 + 1; 0 for an empty row."""
    if n < 1:
        return 0
    while n < DNSMOS_SEGMENT:
        n *= 2
    return (n - DNSMOS_SEGMENT) // DNSMOS_HOP + 1


def dnsmos_row_segments(row: torch.Tensor) -> torch.Tensor:
    """[S, 144160] float32 segments of one unpadded 1-D row (periodic continuation x[i mod n])."""
    n = row.numel()
    m = n
    while m < DNSMOS_SEGMENT:
        m *= 2
    return row.to(torch.float32).repeat(m // n).unfold(0, DNSMOS_SEGMENT, DNSMOS_HOP)


def dnsmos_features(w: dict, segs: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """[S, 900, 161] log-power image of [S, 144160] segments: log10(max(re^2 + im^2, 1e-12))."""
    fr = segs.to(dtype).unfold(1, 320, 160)                                    # [S, 900, 320]
    re = fr @ w["conv_real_stft.weight"].reshape(161, 320).to(dtype).T
    im = fr @ w["conv_imag_stft.weight"].reshape(161, 320).to(dtype).T
    return torch.log10(torch.clamp_min(re.square() + im.square(), 1e-12))


def dnsmos_network(w: dict, image: torch.Tensor) -> torch.Tensor:
    """[S, 3] raw outputs of the convolution stack and the dense layers on [S, 900, 161] images."""
    F = torch.nn.functional
    h = image.unsqueeze(1)
    for i in (0, 2, 4, 6, 9, 12, 15):
        h = F.relu(F.conv2d(h, w[f"conv_layers.{i}.weight"], w[f"conv_layers.{i}.bias"], padding=1))
        if i in _DNSMOS_POOL_AFTER:
            h = F.max_pool2d(h, 2)
    h = h.amax(dim=(2, 3))
    h = F.relu(F.linear(h, w["output_layers.0.weight"], w["output_layers.0.bias"]))
    h = F.relu(F.linear(h, w["output_layers.2.weight"], w["output_layers.2.bias"]))
    return F.linear(h, w["output_layers.4.weight"], w["output_layers.4.bias"])


def dnsmos_raw(w: dict, row: torch.Tensor) -> torch.Tensor:
    """[S, 3] float32 raw network outputs of one unpadded 1-D row (two segments at a time)."""
    segs = dnsmos_row_segments(row)
    with torch.no_grad():
        return torch.cat([dnsmos_network(w, dnsmos_features(w, segs[i:i + 2])) for i in range(0, segs.shape[0], 2)])


def dnsmos(w: dict, rows: torch.Tensor, lengths=None) -> torch.Tensor:
    """[B, 3] float32 (SIG, BAK, OVRL) of [B, L] rows; NaN for a row of no samples and for a row
    with a non-finite sample among those its segments read."""
    B, L = rows.shape
    c0, c1, c2 = (torch.tensor(c, dtype=torch.float32) for c in _DNSMOS_POLY)

    def one(b):
        n = L if lengths is None else int(lengths[b])
        row = rows[b, :n]
        S = dnsmos_segments(n)
        used = n if n <= DNSMOS_SEGMENT else DNSMOS_HOP * (S - 1) + DNSMOS_SEGMENT
        if n < 1 or not bool(torch.isfinite(row[:used]).all()):
            return torch.full((1, 3), float("nan"), dtype=torch.float32)
        raw = dnsmos_raw(w, row)
        poly = c0 + c1 * raw + c2 * raw.square()
        return poly.double().mean(0, keepdim=True).float()

    return torch.cat(_host_map(one, range(B))) if B else torch.empty(0, 3, dtype=torch.float32)
