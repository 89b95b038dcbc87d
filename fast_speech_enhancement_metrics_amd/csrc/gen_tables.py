"""Generate csrc/fsem_tables.inc -- constant tables of the HIP engine (build-time tool).

Everything is computed in float64 and rounded once to float32:
  * P.862 band tables (fast_se_metrics/utils/bark.py, loudness.py) and derived per-band
    constants (loudness exponents exactly as the reference's float32 torch ops compute them);
  * the PESQ level-alignment band-pass (scipy butter(5, [325, 3250], fs=16000), PESQ.py:80)
    as a cascade of second-order sections, and the pre-emphasis filter (PESQ.py:84-88) as FIR
    then all-pole (states y[n-1], y[n-2]), both defined by their float32 coefficients like the
    reference, in state-space form (z' = M z + K u), plus the chunked-scan tables used by the
    time-parallel IIR:
      G[n]  = M^(CH-1-n) K          (end state of a CH-sample chunk from zero state)
      A[d]  = M^(CH*d), d=1,2,4,8    (state carry over d chunks, Hillis-Steele levels)
  * FFT twiddles, Hann windows (torch.hann_window values), STOI 1/3-octave band edges.

Usage: python gen_tables.py  (writes next to this file)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from fast_speech_enhancement_metrics_amd import _tables as T  # noqa: E402

CH = 52          # samples per lane chunk in the PESQ front-end tile (pesq.hip)
SCAN_LEVELS = (1, 2, 4, 8)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def fmt(vals, per_line=6):
    vals = np.asarray(vals).ravel()
    out = []
    for i in range(0, len(vals), per_line):
        out.append("  " + ", ".join(repr(float(v)) + ("f" if vals.dtype == np.float32 else "")
                                     for v in vals[i:i + per_line]) + ",")
    return "\n".join(out)


def arr(name, vals, ctype="float", shape=None, qual="static constexpr"):
    vals = np.asarray(vals)
    if ctype == "float":
        vals = f32(vals)
    dims = "".join(f"[{d}]" for d in (shape or vals.shape))
    if ctype == "int":
        body = "\n".join("  " + ", ".join(str(int(v)) for v in vals.ravel()[i:i + 16]) + ","
                         for i in range(0, vals.size, 16))
    elif ctype == "double":
        body = "\n".join("  " + ", ".join(repr(float(v)) for v in vals.ravel()[i:i + 4]) + ","
                         for i in range(0, vals.size, 4))
    else:
        body = fmt(vals)
    return f"{qual} {ctype} {name}{dims} = {{\n{body}\n}};\n"


def df2t(b, a):
    """TDF-II state space of a (float32-defined) filter, in float64."""
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = b / a[0]
    a = a / a[0]
    n = len(a) - 1
    M = np.zeros((n, n))
    for i in range(n):
        M[i, 0] = -a[i + 1]
        if i + 1 < n:
            M[i, i + 1] = 1.0
    K = b[1:] - a[1:] * b[0]
    return b, a, M, K


def cascade_sections(a):
    """Pair the roots of a(z) into 2nd-order sections, ordered by pole radius (ascending)."""
    poles = np.roots(a)
    cplx = sorted([p for p in poles if p.imag > 1e-9], key=abs)
    real = sorted([p.real for p in poles if abs(p.imag) <= 1e-9], key=abs)
    secs = [(-2.0 * p.real, abs(p) ** 2) for p in cplx]
    for i in range(0, len(real), 2):
        secs.append((-(real[i] + real[i + 1]), real[i] * real[i + 1]))
    secs.sort(key=lambda s: s[1])
    prod = np.array([1.0])
    for a1, a2 in secs:
        prod = np.convolve(prod, [1.0, a1, a2])
    assert np.allclose(prod, a, rtol=0, atol=1e-9), (prod, a)
    return secs


def cascade_state_space(secs):
    """State space of the section cascade, numerators (1 - z^-2), unit gain.

    Section k (TDF-II): y = u + s0;  s0' = s1 - a1*y;  s1' = -u - a2*y  (u = input).
    States ordered section-major.  Returns (M, K); output = last section's y.
    """
    n = 2 * len(secs)
    M = np.zeros((n, n))
    K = np.zeros(n)
    Cu = np.zeros(n)      # u_k = Cu . z + Du * x
    Du = 1.0
    for k, (a1, a2) in enumerate(secs):
        i = 2 * k
        yC = Cu.copy()
        yC[i] += 1.0
        yD = Du
        M[i] += -a1 * yC
        M[i, i + 1] += 1.0
        K[i] = -a1 * yD
        M[i + 1] += -Cu - a2 * yC
        K[i + 1] = -Du - a2 * yD
        Cu, Du = yC, yD
    return M, K


def scan_tables(M, K, ch):
    n = M.shape[0]
    G = np.zeros((ch, n))
    P = np.eye(n)
    for k in range(ch - 1, -1, -1):       # G[k] = M^(ch-1-k) K
        G[k] = P @ K
        P = M @ P
    Mch = np.linalg.matrix_power(M, ch)
    A = [np.linalg.matrix_power(Mch, d) for d in SCAN_LEVELS]
    return G, A


SPEC_GW, SPEC_GO = 32, 15  # bins per band in the sparse filter table; its first bin is f0 - SPEC_GO
SPEC_CENTRE = (50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38,
               1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17,
               3597.63)
SPEC_WIDTH = (70.0,) * 7 + (77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457,
                            199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136)


def spectral_tables(sr: int):
    """(window [win], sparse filters [25, SPEC_GW], first bins [25]) of SpectralMeasures at `sr`, float64."""
    hop = sr * 30 // 4000
    win = 4 * hop
    H = 256 if sr == 8000 else 512
    half = sr / 2.0
    t = np.arange(win, dtype=np.float64)
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * (t + 1.0) / (win + 1.0)))
    floor = np.exp(-30.0 / (2.0 * 2.303))
    g = np.zeros((25, SPEC_GW))
    j0 = np.zeros(25, dtype=np.int64)
    for i, (c, b) in enumerate(zip(SPEC_CENTRE, SPEC_WIDTH)):
        f0 = int(np.floor(c * H / half))
        bw = b * H / half
        j = np.arange(H)
        full = np.exp(-11.0 * ((j - f0) / bw) ** 2 + np.log(SPEC_WIDTH[0]) - np.log(b))
        full[full <= floor] = 0.0
        j0[i] = f0 - SPEC_GO
        for q in range(SPEC_GW):
            if 0 <= j0[i] + q < H:
                g[i, q] = full[j0[i] + q]
        inside = np.zeros(H, dtype=bool)
        inside[max(j0[i], 0):min(j0[i] + SPEC_GW, H)] = True
        assert not full[~inside].any(), (sr, i)  # nothing of the filter lies outside the sparse window
    return w, g, j0


def main():
    from scipy.signal import butter
    import torch

    lines = ["// GENERATED by gen_tables.py -- do not edit.  Constant tables of libfsem.", ""]
    lines.append(f"#define FSEM_PESQ_CH {CH}")
    edges = np.concatenate([[0], np.cumsum(T.BINS_PER_BAND)])
    lines.append(arr("kBandEdge", edges, "int"))
    corr = np.asarray(T.POW_DENS_CORRECTION) * T.SP_16K
    lines.append(arr("kBarkCorr", corr))
    thr = np.asarray(T.ABS_THRESH_POWER, dtype=np.float64)
    lines.append(arr("kThresh", thr))
    lines.append(arr("kHalfInvThresh", 0.5 / thr.astype(np.float32).astype(np.float64)))  # 0.5 / float32(T)
    # loudness.py:45-46: exp = 6 / (tensor(centre) + 2.0); clamp(1,2)**0.15 * 0.23, float32 ops
    c32 = torch.tensor(T.CENTRE_BARK)
    e = (6 / (c32 + 2.0)).clamp(min=1.0, max=2.0) ** 0.15 * T.ZWICKER_POWER
    e = e.numpy().astype(np.float32)
    lines.append(arr("kLoudExp", e))
    lines.append(arr("kLoud2TE", (2.0 * thr) ** e.astype(np.float64) * T.SL_16K))  # (2T)^e * Sl
    wb = np.asarray(T.WIDTH_BARK)
    lines.append(arr("kWidthBark", wb))
    tw = wb[1:].sum()
    lines.append(f"static constexpr double kTotalWidth = {float(tw)!r};")
    lines.append(f"static constexpr float kSl = {T.SL_16K!r}f;")

    # bark-tile MFMA K-step ranges (16 bands per tile, 4 bins per K-step)
    tiles = []
    for t in range(4):
        b0, b1 = 16 * t, min(16 * t + 16, 49)
        lo, hi = edges[b0], edges[b1]
        tiles.append((lo // 4, (hi + 3) // 4))
    lines.append(arr("kBarkTileK", np.array(tiles), "int"))
    band_of_bin = np.zeros(256, dtype=np.int64)
    for i in range(49):
        band_of_bin[edges[i]:edges[i + 1]] = i
    lines.append(arr("kBandOfBin", band_of_bin, "int"))

    # PESQ.py:80-81 band-pass, defined by its float32 (b, a) like the reference.  The float32
    # numerator is exactly g * (1 - z^-2)^5, so the filter is realised as a cascade of five
    # sections (1 - z^-2) / (1 + a1 z^-1 + a2 z^-2) (poles of the float32 denominator,
    # conjugate pairs / the two real poles paired) and an output gain g.  The companion
    # (direct-form) state basis is far too ill-conditioned for the chunk scan in float32
    # (||M^60|| ~ 1e4); the cascade basis keeps ||M^k|| < 6.
    bb, ba = butter(5, [325, 3250], fs=16000, btype="band")
    b32 = np.asarray(bb, dtype=np.float32).astype(np.float64)
    a32 = np.asarray(ba, dtype=np.float32).astype(np.float64)
    g = b32[0]
    assert np.allclose(b32 / g, [1, 0, -5, 0, 10, 0, -10, 0, 5, 0, -1], rtol=0, atol=1e-12)
    secs = cascade_sections(a32)
    lines.append(f"static constexpr float kBpGain = {float(np.float32(g))!r}f;")
    lines.append(arr("kBpSecA", np.array(secs)))
    M, K = cascade_state_space(secs)
    G, A = scan_tables(M, K, CH)
    lines.append(arr("kBpG", G))
    lines.append(arr("kBpScan", np.stack(A), qual="__constant__ static const"))
    # PESQ.py:84-88 pre-emphasis, evaluated as the reference's lfilter does: the FIR part first,
    # w[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] (its float32 numerator sums to exactly 0: a DC offset
    # cancels in w), then the all-pole part y[n] = w[n] - a1 y[n-1] - a2 y[n-2].  The scan states
    # are (y[n-1], y[n-2]) driven by w.  The transposed direct form's states carry b0 x instead:
    # with a DC offset hundreds of times the signal, its chunk-scan sums of those large states
    # lost the signal (PESQ 0.12 off the reference at +100; tools/sim_preemph.py).
    # The scan itself runs in the coupled (normal) form of the all-pole part, (u, v) = T (y[n-1],
    # y[n-2]) with u = y1 - r c y2, v = r s y2 (poles r e^(+-i theta), c = cos theta, s = sin
    # theta): ||M^k|| = r^k.  In the companion basis (y1, y2) itself the two states of the
    # 71 Hz resonance are nearly equal and ||M^52|| ~ 8, which cost a factor 10 in accuracy
    # (tools/sim_preemph.py: 6.9e-5 vs 6.6e-6 relative against the sequential filter).  The
    # start state goes back to (y1, y2) by T^-1 (kPreToY) for the direct-form pass 2.
    b2, a2, _, _ = df2t(T.PRE_B, T.PRE_A)
    lines.append(arr("kPreB", b2))
    lines.append(arr("kPreA", a2))
    M2 = np.array([[-a2[1], -a2[2]], [1.0, 0.0]])
    K2 = np.array([1.0, 0.0])
    rr = np.sqrt(a2[2])
    cc = -a2[1] / (2 * rr)
    ss = np.sqrt(1.0 - cc * cc)
    Tm = np.array([[1.0, -rr * cc], [0.0, rr * ss]])
    Gy, Ay = scan_tables(M2, K2, CH)
    G2 = Gy @ Tm.T
    A2 = [Tm @ A @ np.linalg.inv(Tm) for A in Ay]
    lines.append(arr("kPreToY", np.linalg.inv(Tm)))
    lines.append(arr("kPreG", G2))
    lines.append(arr("kPreScan", np.stack(A2), qual="__constant__ static const"))
    # Pass-1 functionals of all 12 scan states over the chunk's first differences
    # d[n] = x[n] - x[n-1] (one 48-byte row per sample, read by scalar loads: s_load_dwordx4
    # runs feed v_fmac_f32 with an SGPR operand, no literal moves), plus one boundary row.
    #   band-pass  e = sum_n G[n] x[n] = S x[-1] + sum_m C[m] d[m],  C[m] = sum_{n>=m} G[n],
    #              S = C[0] (the untapered input);
    #   pre-emph.  e = sum_n G2[n] (d[n] - d[n-1]) = sum_m (G2[m] - G2[m+1]) d[m] - G2[0] d[-1]
    #              (its all-pole part driven by the second difference, pesq.hip pre_fir).
    # One subtraction per sample serves both filters, and a DC offset never enters a sum.
    C = np.cumsum(G[::-1], axis=0)[::-1]
    H2 = G2 - np.vstack([G2[1:], np.zeros((1, G2.shape[1]))])
    lines.append(arr("kScanG", np.concatenate([C, H2], axis=1), qual="static __constant__"))
    lines.append(arr("kScanB", np.concatenate([C[0], -G2[0]]), qual="static __constant__"))

    # torch.hann_window(512) (periodic) and torch.hann_window(257)[1:] -- exact float32 values
    lines.append(arr("kHann512", torch.hann_window(512).numpy()))
    lines.append(arr("kHann256s", torch.hann_window(257).numpy()[1:]))
    k = np.arange(512)
    lines.append(arr("kTwRe", np.cos(2 * np.pi * k / 512)))
    lines.append(arr("kTwIm", -np.sin(2 * np.pi * k / 512)))

    # STOI.py:26-47 one-third octave bands (fs 10 kHz, 512-pt FFT, 15 bands from 150 Hz)
    freqs = np.linspace(0, 5000, 257)
    kk = np.arange(15, dtype=np.float64)
    flo = 150 * np.power(2.0, (2 * kk - 1) / 6)
    fhi = 150 * np.power(2.0, (2 * kk + 1) / 6)
    obe = np.array([[int(np.argmin(np.abs(freqs - flo[i]))), int(np.argmin(np.abs(freqs - fhi[i])))]
                    for i in range(15)])
    lines.append(arr("kObmEdge", obe, "int"))
    # stoi_tob band sums: lane l sums one piece (<= 12 consecutive bins) of one band of one
    # signal; each band's pieces, padded with empty ones to a power-of-two group (1, 2 or 4 lanes),
    # sit aligned inside a 16-lane row (largest groups first), so a two-level in-row DPP
    # reduction (row_shl 1, 2) gathers every band at its head lane.  Row: signal, band, bin_lo,
    # bin_hi, group size, is_head.
    pieces12 = [[0, 0, 0, 0, 1, 0] for _ in range(64)]
    for sig in range(2):
        groups = []
        for j in range(15):
            lo, hi = int(obe[j, 0]), int(obe[j, 1])
            npc = -(-(hi - lo) // 12)
            groups.append((1 << (npc - 1).bit_length(), j, lo, hi, npc))
        groups.sort(key=lambda g: -g[0])
        pos = 32 * sig
        for gs, j, lo, hi, npc in groups:
            assert pos % gs == 0 and pos // 16 == (pos + gs - 1) // 16
            for q in range(gs):
                a = lo + (hi - lo) * q // npc if q < npc else lo
                b = lo + (hi - lo) * (q + 1) // npc if q < npc else lo
                pieces12[pos + q] = [sig, j, a, b, gs, 1 if q == 0 else 0]
            pos += gs
        assert pos <= 32 * (sig + 1)
    assert max(r[3] - r[2] for r in pieces12) <= 12
    lines.append(arr("kObmPiece", np.array(pieces12), "int"))

    # torchaudio Resample(16000, 10000) kernel [5, 28] (base.py:13; fused into the STOI kernels)
    from fast_speech_enhancement_metrics_amd.resample import sinc_kernel
    rk, width, orig, new = sinc_kernel(16000, 10000)
    assert (width, orig, new) == (10, 8, 5) and tuple(rk.shape) == (5, 28)
    lines.append(arr("kRs16k10k", rk.numpy()))

    # SpectralMeasures (spectral.hip; include/fsem.h "Spectral"): per rate (8 kHz, 16 kHz) the frame
    # window w[t] = 0.5 (1 - cos(2 pi (t + 1) / (win + 1))) and the 25 critical-band filters as a
    # sparse table, SPEC_GW bins per band from bin f0_i - SPEC_GO (the filters are zero outside
    # +-14 bins after the threshold; asserted); and the split-step twiddles W_1024^j of the
    # 1024-point real transform.  The formulas of composite.hip's composite_tables.
    lines.append(f"#define FSEM_SPEC_GW {SPEC_GW}")
    lines.append(f"#define FSEM_SPEC_GO {SPEC_GO}")
    for tag, sr in (("8k", 8000), ("16k", 16000)):
        win, g, j0 = spectral_tables(sr)
        lines.append(arr(f"kSpecWin{tag}", win, qual="__constant__ static const"))
        lines.append(arr(f"kSpecG{tag}", g, qual="__constant__ static const"))
        lines.append(arr(f"kSpecJ0{tag}", j0, "int", qual="__constant__ static const"))
    j = np.arange(512)
    lines.append(arr("kSpecTw", np.stack([np.cos(np.pi * j / 512), np.sin(np.pi * j / 512)], axis=1),
                     qual="__constant__ static const"))

    out = os.path.join(HERE, "fsem_tables.inc")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
