/*
 * fsem_dnsmos.h -- C-ABI of libfsem_dnsmos.so, the MI355X (gfx950) engine behind
 * fast_speech_enhancement_metrics_amd.DNSMOS.
 *
 * A library of its own beside libfsem.so, libfsem_composite.so, libfsem_lsd.so and libfsem_bsssdr.so
 * (their entry sets and workspace sizes are pinned; fsem_version() stays 11).  It calls nothing of
 * libfsem.so (it shares its headers only) and does not link against it.  Conventions (device
 * pointers, workspace, stream, row addressing, `lengths`, error codes) are those of fsem.h.  The
 * libraries are built together and carry the same build id; the host layer refuses a stale one.
 */
#ifndef FSEM_DNSMOS_H
#define FSEM_DNSMOS_H

#include "fsem.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- DNSMOS: SIG, BAK, OVRL
 * The reference's fast_se_metrics.DNSMOS (DNSMOS.py): a no-reference MOS estimate of 16 kHz rows from
 * a small convolutional network (checkpoint SIG_BAK_OVR, 22 tensors).  0-based indices.
 *
 * Segments.  A row of n samples is read as the periodic signal x[i mod n] (the reference doubles the
 * row until it holds 144160 samples, reaching n' = n 2^k; nothing is materialised here).  It has
 * S = (n' - 144160) / 16000 + 1 segments (integer division); segment s starts at sample 16000 s.
 * Samples at or past n are never read, whatever the memory holds.
 *
 * Per segment:
 *  - Front end: frame f (f = 0 ... 899) covers the 320 samples from 160 f.  re, im = the checkpoint's
 *    two 161 x 320 matrices times the frame (products of float32 values summed in double, rounded once
 *    to float32), then log10(max(re^2 + im^2, 1e-12)) with the power in float32: the image [900][161].
 *    No underflow to -inf: an all-zero segment is -12 everywhere (the reference computes this stage
 *    under half-precision autocast, where 1e-12 is 0 and quiet bins become -inf, hence NaN scores).
 *  - conv1 (1 -> 128, 3 x 3, padding 1) + ReLU in float32 from the image, rounded to f16; then
 *    conv2 (128 -> 64), conv3 (64 -> 64), conv4 (64 -> 32) + 2 x 2 max-pool, conv5 (32 -> 32) + pool,
 *    conv6 (32 -> 32) + pool, conv7 (32 -> 64): 3 x 3, padding 1, ReLU; f16 operands through
 *    v_mfma_f32_16x16x32_f16 with float32 accumulation, bias and ReLU in float32, activations stored
 *    as f16 (NHWC).  Pooling floors (900 -> 450 -> 225 -> 112 rows, 161 -> 80 -> 40 -> 20 columns).
 *  - The maximum of conv7's output over its 112 x 20 positions: 64 float32 values.
 *  - Dense 64 -> 128 -> 64 -> 3 with ReLU between, float32: the raw outputs r[3].
 *  - SIG, BAK, OVRL of the segment: c + b1 r + b2 r^2 with the reference's constants, float32.
 * A row's scores are the means over its segments (summed in double, segment 0 first).
 *
 * A row with a non-finite sample among those its segments read (all n of a row of at most 144160
 * samples; the first 16000 (S - 1) + 144160 of a longer one, as in the reference) is NaN in all
 * three scores, in that row only; the front end flags the segment, nothing relies on NaN passing
 * through ReLU and pooling.  A row with no samples is NaN (the reference never returns on it).
 *
 * Weights.  fsem_dnsmos_pack_weights_f32 turns the 22 float32 tensors (device pointers, state-dict
 * layout, in state-dict order:
 *   conv_real_stft.weight [161][320], conv_imag_stft.weight [161][320],
 *   conv_layers.{0,2,4,6,9,12,15}.{weight [Cout][Cin][3][3], bias [Cout]},
 *   output_layers.{0,2,4}.{weight [out][in], bias [out]})
 * into one device blob of fsem_dnsmos_weights_bytes() bytes: f16 convolution weights ordered
 * [tap][Cout][Cin] (the MFMA B operand reads 8 consecutive Cin), float32 transposed STFT matrices,
 * float32 conv1 weights, biases and dense layers.  `tensors` is a HOST array of 22 device pointers.
 * Once per device; the blob is read-only afterwards.
 *
 * Workspace.  The engine processes P segments per pass, P = the largest count (at most
 * FSEM_DNSMOS_MAX_PASS = 16) whose buffers fit ws_bytes, and loops over the passes on the stream.
 * fsem_dnsmos_min_workspace_bytes() is the size for P = 1; fsem_dnsmos_workspace_bytes(batch, length)
 * the recommended size, for P = min(16, the batch's largest possible segment count): it does not
 * grow with the batch beyond that cap.  Every workspace from the minimum upward gives bitwise the
 * same scores.  Without `lengths` every row has fsem_dnsmos_segments(length) segments; with
 * `lengths` the row's own count, and S_total is the sum over the rows (segments ordered row by row).
 *   deg         : [batch, length] float32 (row stride ld), 4-byte loads (any alignment)
 *   lengths     : NULL or [batch] int32 per-row lengths (Conventions)
 *   weights     : the packed blob
 *   sig_bak_ovr : [batch][3] float32 output
 *   features    : [S_total][900][161] float32 output (the log-power image)
 *   raw         : [S_total][3] float32 output (the network's outputs before the polynomial)
 * A row's scores are bitwise the same whatever the batch size, the row's position, `length`, `ld`,
 * the alignment, the workspace size and the stream (no float atomics; every sum has one order).
 * FSEM_EINVAL for null pointers, batch < 1, length < 1, ld < length or length > 2^29;
 * FSEM_EWORKSPACE for a workspace below the minimum (or a blob that is too small); both before any
 * launch.
 */
#define FSEM_DNSMOS_MAX_PASS 16
#define FSEM_DNSMOS_NUM_TENSORS 22

int64_t fsem_dnsmos_segments(int64_t length);  /* 0 for length < 1 */
size_t fsem_dnsmos_weights_bytes(void);
int fsem_dnsmos_pack_weights_f32(const float *const *tensors, void *blob, size_t blob_bytes, void *stream);
size_t fsem_dnsmos_min_workspace_bytes(void);
size_t fsem_dnsmos_workspace_bytes(int64_t batch, int64_t length);  /* 0 for arguments fsem_dnsmos_f32 refuses */
int fsem_dnsmos_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                    const void *weights, float *sig_bak_ovr, void *ws, size_t ws_bytes, void *stream);
int fsem_dnsmos_features_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                             const void *weights, float *features, void *ws, size_t ws_bytes, void *stream);
int fsem_dnsmos_raw_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                        const void *weights, float *raw, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FSEM_DNSMOS_H */
