/*
 * fsem_composite.h -- C-ABI of libfsem_composite.so, the MI355X (gfx950) engine behind
 * fast_speech_enhancement_metrics_amd.Composite.
 *
 * A library of its own beside libfsem.so: libfsem.so's entry set and workspace sizes are pinned
 * entry by entry (fsem_version() stays 11), so the composite entries live here, link against
 * libfsem.so and call its PESQ and resampling entries.  Conventions (device pointers, workspace,
 * stream, row addressing, `lengths`, error codes) are those of fsem.h.  Both libraries are built
 * together and carry the same build id (fast_speech_enhancement_metrics_amd/_build.py); the host
 * layer refuses a stale one.
 */
#ifndef FSEM_COMPOSITE_H
#define FSEM_COMPOSITE_H

#include "fsem.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- Composite: CSIG, CBAK, COVL, LLR, WSS
 * Replaces nothing in the reference.  The composite measures of Hu &
 * Loizou 2008 with their ingredients, seven numbers per row pair.  No implementation of Loizou's
 * composite.m was available to compare with: agreement with it is by definition only.  0-based
 * indices throughout.
 *
 * Notation.  Per row, s is the clean row's first n samples and s^ the denoised row's.  Rows are
 * scored at `sample_rate` for LLR, WSS and SegSNR.
 *
 * Frames.  These are exactly SegSNR's frames:
 *  - hop = sample_rate * 30 / 4000 (integer division), win = 4 hop.
 *  - w[t] = 0.5 (1 - cos(2 pi (t + 1) / (win + 1))).
 *  - The F = (n - win) / hop + 1 complete frames (fsem_sdr_frames).
 *  - Frame f of a signal x is w[t] x[f hop + t].
 *
 * LLR of a frame.
 *  - Order P is 10 at 8 kHz and 16 at 16 kHz.
 *  - R_x[k] = sum_t x[t] x[t + k] for k = 0 ... P, over the windowed frame, unnormalised.
 *  - A_x = [1, a_1 ... a_P] is the prediction-error filter from Levinson-Durbin on R_x.
 *  - T is the (P + 1) x (P + 1) Toeplitz matrix of R_s.
 *  - LLR_f = ln((A_s^ T A_s^') / (A_s T A_s')).
 *  - There is no per-frame clamp.
 *  - A frame with R[0] == 0 in either signal is NaN, by 0 / 0.
 *
 * WSS of a frame.
 *  - nfft is 512 at 8 kHz and 1024 at 16 kHz (2^nextpow2(2 win)).  H = nfft / 2.
 *  - Power spectrum: S_x[j] = |FFT_nfft(frame)[j]|^2 for j = 0 ... H - 1.
 *  - The 25 critical bands have centre frequencies (Hz): 50, 120, 190, 260, 330, 400, 470, 540,
 *    617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16,
 *    1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63.
 *  - Their bandwidths (Hz): 70 (x7), 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423,
 *    153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465,
 *    346.136 (Loizou's comp_wss.m: 25 values, seven of 70 Hz).
 *  - Filter i:
 *      g_i[j] = exp(-11 ((j - floor(c_i H / (rate / 2))) / (b_i H / (rate / 2)))^2 + ln b_0 - ln b_i);
 *      g_i[j] is set to 0 where it is <= exp(-30 / (2 * 2.303)).
 *  - Band energy: e_x[i] = 10 log10(max(sum_j S_x[j] g_i[j], 1e-10)).
 *  - Slopes: sl_x[i] = e_x[i + 1] - e_x[i] for i = 0 ... 23.
 *  - Nearest peak of band i, the published code's own search with its quirk kept:
 *      if sl[i] > 0: m = i; while m < 24 and sl[m] > 0: m += 1; pk[i] = e[m - 1].
 *      else:         m = i; while m >= 0 and sl[m] <= 0: m -= 1; pk[i] = e[m + 1].
 *  - Weights: W_x[i] = 20 / (20 + max(e_x) - e_x[i]) * 1 / (1 + pk_x[i] - e_x[i]); W = (W_s + W_s^) / 2.
 *  - WSS_f = sum_i W[i] (sl_s[i] - sl_s^[i])^2 / sum_i W[i].
 *
 * Row values of LLR and WSS.
 *  - Sort the F frame values ascending, with NaN after every number, as `sort` does.
 *  - Take the mean of the first K = (19 F + 10) / 20 (integer division).  That is round(0.95 F) with
 *    halves rounded up: F = 30 gives 29, not 28.
 *  - The result is NaN when F = 0, or when a NaN lies among the K.
 *
 * SegSNR.  The definition of fsem_sdr_f32's seg_snr (fsem.h), the mean over all F frames.
 *
 * PESQ.  What fsem_pesq_wb_f32 gives for the same rows: wideband MOS-LQO, no time alignment.  8 kHz
 * rows are resampled to 16 kHz first (fsem_resample_f32 / fsem_resample_rows_f32, as the PESQ
 * class does).
 *
 * Composites, each clamped to [1, 5]:
 *   CSIG = 3.093 - 1.029 LLR + 0.603 PESQ - 0.009 WSS
 *   CBAK = 1.634 + 0.478 PESQ - 0.007 WSS + 0.063 SegSNR
 *   COVL = 1.594 + 0.805 PESQ - 0.512 LLR - 0.007 WSS
 * A NaN ingredient gives a NaN composite.
 *
 * Non-finite and short rows.  A row with a non-finite sample, or of length 0, is NaN in all seven
 * outputs; other rows are unaffected.  Rows too short for PESQ behave as in fsem_pesq_wb_f32: NaN in
 * that row's pesq (and composites) with `lengths`, FSEM_ESHORT in the whole-batch form (before any
 * launch); with `lengths` their llr, wss and seg_snr are still scored.
 *
 * Precision: the window product is float32; the autocorrelation sums, Levinson-Durbin, the two
 * quadratic forms and the logarithm are double; the spectra and band energies are float32, the
 * slopes, weights and WSS_f double; per-frame values are stored as float32 and the row means
 * accumulated in double.
 *   ref, deg : [batch, length] float32 (row stride ld); the PESQ stage reads rows as
 *              fsem_pesq_wb_f32 does (16-byte pieces, readable up to ceil4(length) floats); the
 *              composite's own kernels read 4 bytes at a time, any alignment
 *   lengths  : NULL or [batch] int32 per-row lengths (Conventions)
 *   csig, cbak, covl, pesq, llr, wss, seg_snr : [batch] float32 outputs
 * A row's scores are bitwise the same whatever the batch size, the row's position, `length`, `ld` and
 * the stream (no atomics whose order can change a result: integer histogram counts only; every sum
 * has one order, fixed by sample_rate).
 * sample_rate 8000 or 16000; others give FSEM_ERATE and the queries return 0.
 */
int64_t fsem_composite_chunk(int32_t sample_rate);  /* samples per launch chunk (16 hops); 0 when unsupported */
size_t fsem_composite_workspace_bytes(int64_t batch, int64_t length, int32_t sample_rate);
int fsem_composite_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                       const int32_t *lengths, int32_t sample_rate, float *csig, float *cbak, float *covl,
                       float *pesq, float *llr, float *wss, float *seg_snr, void *ws, size_t ws_bytes,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FSEM_COMPOSITE_H */
