/*
 * fsem_bsssdr.h -- C-ABI of libfsem_bsssdr.so, the MI355X (gfx950) engine behind
 * fast_speech_enhancement_metrics_amd.BSSSDR (the reference's fast_se_metrics.SDR).
 *
 * A library of its own beside libfsem.so, libfsem_composite.so and libfsem_lsd.so: their entry sets
 * and workspace sizes are pinned entry by entry (fsem_version() stays 11), so these entries live
 * here.  The library calls nothing of libfsem.so (it shares its headers only) and does not link
 * against it.  Conventions (device pointers, workspace, stream, row addressing, `lengths`, error
 * codes) are those of fsem.h.  The four libraries are built together and carry the same build id
 * (fast_speech_enhancement_metrics_amd/_build.py); the host layer refuses a stale one.
 */
#ifndef FSEM_BSSSDR_H
#define FSEM_BSSSDR_H

#include "fsem.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------ BSS-eval SDR with a 512-tap distortion filter
 * The reference's fast_se_metrics.SDR (SDR.py:7-97), the quantity of
 * torchmetrics.functional.audio.signal_distortion_ratio with filter_length = 512, zero_mean = False.
 * Rows are scored as 16 kHz rows; the host layer resamples other rates first.  0-based indices.
 *
 * Per row pair, s is the clean row's first n samples and h the denoised row's.
 *  - Normalisation: s' = s / max(|s|, 1e-6), h' = h / max(|h|, 1e-6).  The norms |.| are the roots
 *    of the sums of squares in double, rounded to float32; the maximum and the quotient are float32
 *    (a correctly rounded division), as the reference takes them.  Everything below is double.
 *  - Correlations, k = 0 ... 511: r[k] = sum_t s'[t] s'[t + k], b[k] = sum_t s'[t] h'[t + k]; samples
 *    outside [0, n) are zero whatever the memory past n holds.  (Linear correlations: the reference's
 *    transform length n_fft >= 2 n - 1 rules out wrap-around and is no part of the definition.)
 *    load_diag, where given, is added to r[0].
 *  - Solve: R x = b with R[i][j] = r[|i - j|], by the Levinson-Durbin recursion for a general
 *    right-hand side; coh = b . x.
 *  - SDR = 10 log10(max(coh / max(1 - coh, 1e-8), 1e-8)): within [-80, +80] dB up to rounding;
 *    identical rows give +80, a silent denoised row -80.
 *
 * No special cases beyond these: a row whose system is singular -- r[0] == 0 (a silent clean row,
 * n == 0) or a prediction error of the recursion that is <= 0 at any order -- is NaN, and so is a
 * row with a non-finite sample, in that row only.  (The reference raises for the whole batch.)
 *
 * Order of the sums (each has one order, which depends on n alone): the sums of squares per
 * chunk of fsem_bsssdr_norm_chunk() samples, the chunks in ascending order; the correlations per
 * chunk of fsem_bsssdr_chunk() samples (a chunk's t range in four consecutive quarters of each
 * 2048-sample piece, t ascending within a quarter, the quarters added as ((q0 + q1) + q2) + q3),
 * the chunks in ascending order.  The norms come from a first pass, so the float32 quotients above
 * are formed exactly as stated.
 *   ref, deg : [batch, length] float32 (row stride ld), readable up to ceil4(length) floats per row
 *   lengths  : NULL or [batch] int32 per-row lengths (Conventions)
 *   sdr      : [batch] float32 output, dB
 * A row's score is bitwise the same whatever the batch size, the row's position, `length`, `ld`,
 * the alignment and the stream (no atomics).
 * FSEM_EINVAL for null pointers, batch < 1, length < 1, ld < length, length > 2^29 or a load_diag
 * that is not finite; FSEM_EWORKSPACE for a workspace that is too small; both before any launch.
 */
int64_t fsem_bsssdr_filter_length(void);  /* 512 */
int64_t fsem_bsssdr_chunk(void);          /* samples per record of partial correlations */
int64_t fsem_bsssdr_norm_chunk(void);     /* samples per record of the two sums of squares */
size_t fsem_bsssdr_workspace_bytes(int64_t batch, int64_t length);  /* 0 for arguments fsem_bsssdr_f32 refuses */
int fsem_bsssdr_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                    const int32_t *lengths, float *sdr, void *ws, size_t ws_bytes, void *stream);
/* The same with load_diag added to r[0] (fsem_bsssdr_f32 is load_diag = 0). */
int fsem_bsssdr_load_diag_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                              const int32_t *lengths, double load_diag, float *sdr, void *ws, size_t ws_bytes,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FSEM_BSSSDR_H */
