/*
 * fsem_lsd.h -- C-ABI of libfsem_lsd.so, the MI355X (gfx950) engine behind
 * fast_speech_enhancement_metrics_amd.LSD.
 *
 * A library of its own beside libfsem.so and libfsem_composite.so: their entry sets and workspace
 * sizes are pinned entry by entry (fsem_version() stays 11), so the LSD entries live here.  The
 * library calls nothing of libfsem.so (it shares its headers only) and does not link against it.
 * Conventions (device pointers, workspace, stream, row addressing, `lengths`, error codes) are
 * those of fsem.h.  The three libraries are built together and carry the same build id
 * (fast_speech_enhancement_metrics_amd/_build.py); the host layer refuses a stale one.
 */
#ifndef FSEM_LSD_H
#define FSEM_LSD_H

#include "fsem.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- LSD: log-spectral distance
 * The reference's fast_se_metrics.LSD (LSD.py:32-52), after the URGENT challenge's evaluation.
 * Rows are scored as 16 kHz rows; the host layer resamples other rates first.  0-based indices.
 *
 * Per row pair, s is the clean row's first n samples and h the denoised row's.
 *  - Scale: a = sum(s h) / (sum(h h) + 1e-8), h' = a h.
 *  - Frames: nfft = 512, hop = 256, periodic Hann window w[t] = 0.5 (1 - cos(2 pi t / 512)),
 *    centred with zero padding: frame f covers samples 256 f - 256 ... 256 f + 255, samples outside
 *    [0, n) are zero whatever the memory past n holds.  F = 1 + n / 256 frames (integer division).
 *  - Magnitudes S[f][k], H[f][k] of s and h' for the bins k = 0 ... 256.
 *  - LSD = (1 / F) sum_f sqrt((1 / 257) sum_k ln(S^2 / (H + 1e-8)^2 + 1e-8)^2).
 *
 * What follows from the definition is kept, without special cases: both rows silent, or a silent
 * clean row, give ln 1e8 = 18.42068; n = 0 is one all-zero frame and gives the same; a silent
 * estimate gives a large finite value; a negative a acts as |a|.  A row with a non-finite sample
 * is NaN, in that row only.
 *
 * Precision: sum(s h) and sum(h h) in double (products of float32 samples are exact in double),
 * and so are a, a h, the window products and the 512-point transform (one complex transform of
 * w s + i w a h, split into the two spectra; a frame of one signal that is all zero gets an
 * exactly zero spectrum).  The log ratio weighs bins 100 dB below a frame's peak like any other
 * (the upper half of the spectrum of rows resampled from 8 kHz), where a float32 transform's
 * rounding is a tenth of the bin.  The squared magnitudes are rounded to float32; the root, the
 * ratio S^2 / (H + 1e-8)^2 + 1e-8 and its logarithm are float32; the sum over bins and the sum over
 * frames are double; one float32 value per frame in the workspace.
 *   ref, deg : [batch, length] float32 (row stride ld), readable up to ceil4(length) floats per
 *              row; read in 16-byte pieces where both operands and ld allow, else 4 bytes at a
 *              time, with the same result bit for bit
 *   lengths  : NULL or [batch] int32 per-row lengths (Conventions)
 *   lsd      : [batch] float32 output
 * A row's score is bitwise the same whatever the batch size, the row's position, `length`, `ld`,
 * the alignment and the stream (no atomics; every sum has one order).
 * FSEM_EINVAL for null pointers, batch < 1, length < 1, ld < length or length > 2^29;
 * FSEM_EWORKSPACE for a workspace that is too small; both before any launch.
 */
int64_t fsem_lsd_frames(int64_t length);  /* 1 + length / 256; 0 for a negative length */
int64_t fsem_lsd_chunk(void);             /* samples per record of the two scale sums */
size_t fsem_lsd_workspace_bytes(int64_t batch, int64_t length);  /* 0 for arguments fsem_lsd_f32 refuses */
int fsem_lsd_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                 const int32_t *lengths, float *lsd, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FSEM_LSD_H */
