/*
 * fsem.h -- C-ABI of libfsem.so, the MI355X (gfx950) engine behind
 * fast_speech_enhancement_metrics_amd.PESQ / .STOI.
 *
 * The reference (kcoost/fast_speech_enhancement_metrics) is a pure-Python/PyTorch
 * library with no FFI layer; its drop-in boundary is the metric class API
 *   BaseMetric.__call__(clean, denoised) -> list[dict]      fast_se_metrics/base.py:41-43
 * Each entry point below replaces the reference computation named next to it; the
 * Python host layer (fast_speech_enhancement_metrics_amd/base.py, PESQ.py, STOI.py) keeps
 * the reference's class API and calls these through ctypes.
 *
 * Conventions
 *  - every pointer argument is DEVICE memory owned by the caller (torch tensors);
 *  - the library allocates nothing: scratch space comes from `ws` (size from the
 *    matching *_workspace_bytes query); work is enqueued asynchronously on `stream`
 *    (a hipStream_t; NULL = the default stream) and the call returns immediately;
 *  - signals are float32 rows: element (b, t) of a batch lives at ptr[b * ld + t]; the
 *    PESQ and STOI entries read rows in 16-byte pieces, so each row must be readable up to
 *    ceil4(length) floats (values past `length` are never used);
 *  - per-row lengths (variable-length batches): the PESQ and STOI entries take
 *    `lengths`, a DEVICE int32[batch] array or NULL.  NULL means every row has `length`
 *    samples.  Otherwise row b holds lengths[b] samples (clamped to [0, length]; `length`
 *    is then the row capacity, sizing workspace and layouts) and its result is that of the
 *    reference called on the unpadded row alone; rows too short for the metric give NaN
 *    (instead of FSEM_ESHORT, which only the whole-batch form returns);
 *  - rows are at most 2^29 samples long (9.3 h at 16 kHz), before and after any resampling:
 *    the kernels address rows with 32-bit byte offsets; longer rows give FSEM_EINVAL;
 *  - input domain (tests/test_edges_ref_gpu.py against the reference's own outputs,
 *    tests/golden/edges_16k.npz, tone_probe_10k.npz, lowpass_10k.npz; every figure below is
 *    per row, profiles/r4_g/edges_rows.log):
 *      PESQ: any finite scale (the PESQ front end shifts tiles whose peak lies outside
 *        [2^-40, 2^40] by a power of two; measured at common scales 1e-15 and 1e18: within
 *        5.6e-5 of the reference in every row) and DC offsets (the pre-emphasis runs FIR first,
 *        as the reference; +100 / +1000 on both signals: within 2.1e-3 in every row).
 *      STOI/ESTOI: scale-invariant from about 1e-10 to 1e17; below, the reference's own
 *        result is its 1e-12 * randn term (two seeds differ by 1e-2 around 0) and the engine
 *        returns that term's expectation (0; within 3.5e-3 of the reference in every row);
 *        above, float32 |X|^2 overflows and both give NaN.  DC offsets up to 1000x the signal:
 *        within 9.7e-3 in every row (the reference's own re-evaluations of those rows -- the
 *        same input scaled by 0.6 ... 1.3, another seed -- spread by up to 2.3e-2); a denoised
 *        signal 80-100 dB below the clean one in its upper bands: within 2.5e-4.  Pure tones
 *        (envelopes flat to ~1e-6, scores near 0): within 6.1e-3 (STOI) / 1.6e-2 (ESTOI) of the
 *        reference in every row, each inside twice that row's own re-evaluation spread
 *        (1.1e-2 / 2.1e-2 on the worst row);
 *  - return 0 on success or a negative FSEM_E* code (fsem_strerror() for text);
 *  - re-entrant across streams / devices (launches use the current HIP device).
 */
#ifndef FSEM_H
#define FSEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSEM_OK 0
#define FSEM_EINVAL -1        /* bad argument (sizes, null pointers)               */
#define FSEM_EWORKSPACE -2    /* workspace smaller than *_workspace_bytes()        */
#define FSEM_ELAUNCH -3       /* HIP launch / runtime error                        */
#define FSEM_ESHORT -4        /* input too short for the metric (see each entry)  */
#define FSEM_ERATE -5         /* unsupported sample-rate pair (see resampling)      */

const char *fsem_strerror(int code);
/* (fsem_spectral_*, fsem_srmr_*, fsem_bsseval_* and fsem_pitsdr_* joined at ABI 11 without a bump: entries that take no workspace
 * add to the set and change no existing entry, workspace size or layout.) */
int fsem_version(void);  /* 11: + fsem_sdr_*; 10: + fsem_pesq_wb_frames_f32; 9: + fsem_pesq_bad_intervals_*, fsem_pesq_pool_f32; 8: + fsem_time_align_p862_*; 7: + fsem_host_buffer_mapped; 6: + fsem_build_id; 5: + fsem_time_align_utt_*; 4: + fsem_pre_emphasize_f32; 3: time alignment, distances */
/* Content hash (16 hex digits) of the sources, headers and compile flags this library was built
 * from (fast_speech_enhancement_metrics_amd/_build.py source_hash); the host layer refuses a
 * library whose id differs from its own tree's.  "unknown" for builds outside _build.py. */
const char *fsem_build_id(void);
/* 1 when the page-locked host buffer p is mapped into the device address space at the same
 * address (so an entry may write its scores straight into it), else 0.  Host-side query, no
 * kernel. */
int fsem_host_buffer_mapped(const void *p);

/* ---------------------------------------------------------------- resampling
 * torchaudio.transforms.Resample(orig, new) (sinc_interp_hann, width 6,
 * rolloff 0.99) as used by BaseMetric.prepare_audio   fast_se_metrics/base.py:13,19-20
 * out: [rows, fsem_resample_length(n_in, orig, new)] with row stride ld_out.
 * Any rate pair whose filter has at most 8192 taps (taps = 2 * ceil(6 * o / (0.99 * min(o, n))) + o
 * for the reduced pair o -> n = orig / g -> new / g): every common audio rate (8, 11.025, 16,
 * 22.05, 24, 32, 44.1, 48, 88.2, 96 kHz) to 16 or 10 kHz.  Longer filters (e.g. 44100 -> 16001)
 * give FSEM_ERATE here and in every entry that resamples (fsem_resample_length returns -1).
 * rows: any count (launches are sliced internally; no grid-dimension limit reaches the caller).
 */
int64_t fsem_resample_length(int64_t n_in, int32_t orig_freq, int32_t new_freq);
int fsem_resample_f32(const float *in, int64_t rows, int64_t n_in, int64_t ld_in,
                      float *out, int64_t ld_out, int32_t orig_freq, int32_t new_freq,
                      void *stream);
/* Ragged rows: row r is resampled as its first lengths[r] samples alone (zeros past them, as
 * BaseMetric.__call__'s zero-padded rows), giving fsem_resample_length(lengths[r], ...) samples;
 * the rest of the row, up to fsem_resample_length(n_in, ...), is written as zeros.
 * FSEM_ERATE if orig_freq == new_freq. */
int fsem_resample_rows_f32(const float *in, int64_t rows, int64_t n_in, int64_t ld_in,
                           const int32_t *lengths, float *out, int64_t ld_out, int32_t orig_freq,
                           int32_t new_freq, void *stream);

/* ---------------------------------------------------------------- PESQ-wb
 * Whole-metric entry: replaces PESQ.compute_metric    fast_se_metrics/PESQ.py:232-245
 * (get_disturbances :174-230 + MOS mapping :240-243) for 16 kHz input.
 *   ref, deg : [batch, length] float32 (row stride ld)  -- clean / denoised
 *   mos      : [batch] float32 output
 *   lengths  : NULL or [batch] int32 per-row lengths (see Conventions)
 * FSEM_ESHORT when the padded length yields < 20 frames (the reference's
 * unfold(1, 20, 10) raises RuntimeError there, PESQ.py:169); with `lengths`, such rows
 * give NaN.
 */
size_t fsem_pesq_workspace_bytes(int64_t batch, int64_t length);
int fsem_pesq_frames(int64_t length);  /* F = 1 + (L + L%256 - 512) / 256 (PESQ.py:128-133) */
int fsem_pesq_wb_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                     int64_t ld, const int32_t *lengths, float *mos, void *ws, size_t ws_bytes,
                     void *stream);

/* Stage entries (same math, split for parity tests of intermediates):
 * front: replaces PESQ.align_level's filtered power (PESQ.py:92-98) and
 *        PESQ.get_bark_bands (PESQ.py:123-140) up to BarkFilterBank.forward
 *        (bark.py:203-204), BEFORE the level scale:
 *          bark  [2*batch, 49, Fld] float32, band-major (signal s, band k, frame f at
 *                (s*49 + k)*Fld + f; signals 0..B-1 ref, B..2B-1 deg), unscaled,
 *                F = fsem_pesq_frames(length), Fld = F rounded up to a multiple of 32
 *                (frames F..Fld-1 unused); a shorter row fills its first
 *                fsem_pesq_frames(lengths[b]) frames
 *          power [2*batch] float32 = sum_t filtered^2 (not yet / (L+5120) / 1.04684)
 * back:  replaces PESQ.py:142-245 on those tensors -> mos [batch].
 */
size_t fsem_pesq_front_workspace_bytes(int64_t batch, int64_t length);
int fsem_pesq_front_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                        int64_t ld, const int32_t *lengths, float *bark, float *power, void *ws,
                        size_t ws_bytes, void *stream);
/* front_y10: the joint entry's front end -- as front, and also writes the rows' 10 kHz
 *        resampled signals (STOI's BaseMetric resampler, base.py:19-20) from the same tiles:
 *          y10 [2*batch, y_ld] float32, row 2b = clean b, 2b+1 = denoised b, first
 *          ceil(5*length_b/8) samples written; y_ld >= ceil(5*length/8), y_ld % 4 == 0;
 *          vad NULL or [batch, vad_ld, 2] float32: the clean rows' STOI voice-activity
 *          quarter sums (remove_silent_frames' frame energies, STOI.py:92-99, per 64-sample
 *          block m: {sum (w[64(m&1)+t] y[64m+t])^2, sum (w[128+64(m&1)+t] y[64m+t])^2}, w =
 *          hann(257)[1:]) for every complete block; vad_ld >= floor(L10/64)+1 rounded up to 64.
 */
int fsem_pesq_front_y10_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                            int64_t ld, const int32_t *lengths, float *bark, float *power,
                            float *y10, int64_t y_ld, float *vad, int64_t vad_ld, void *ws,
                            size_t ws_bytes, void *stream);
size_t fsem_pesq_back_workspace_bytes(int64_t batch, int64_t length);
int fsem_pesq_back_f32(const float *bark, const float *power, int64_t batch, int64_t length,
                       const int32_t *lengths, float *mos, void *ws, size_t ws_bytes,
                       void *stream);
/* distances: the back end's intermediates instead of the scores -- replaces
 *        PESQ.get_disturbances (PESQ.py:174-230) on the front end's tensors:
 *          dist   [2, batch] float32: symmetric distance (row 0) and asymmetric distance (row 1)
 *                 after get_overlapping_sums (PESQ.py:227-228); NaN for rows under 20 frames
 *          frames NULL or [batch, 2, Fcap] float32 (Fcap = fsem_pesq_frames(length)): per-frame
 *                 symmetric / asymmetric disturbances after the frame weighting and the clamp at
 *                 45 (PESQ.py:222-224); row b fills its first fsem_pesq_frames(lengths[b]) frames
 */
/* pre-emphasis: replaces the lfilter of PESQ.pre_emphasize (PESQ.py:111; the edge taper of
 *        :108-109 is the caller's, applied in place as the reference does) on any [rows, length]
 *        float32 rows: y = lfilter(x, a = (1, -1.9444777, 0.94597794), b = (2.740826,
 *        -5.4816519, 2.740826)) in torchaudio's float32 evaluation order (FIR then the all-pole
 *        loop).  y [rows, length] float32, row stride ld_out (y may equal x only if ld_out == ld).
 */
int fsem_pre_emphasize_f32(const float *x, int64_t rows, int64_t length, int64_t ld, float *y,
                           int64_t ld_out, void *stream);
size_t fsem_pesq_distances_workspace_bytes(int64_t batch, int64_t length);
int fsem_pesq_distances_f32(const float *bark, const float *power, int64_t batch, int64_t length,
                            const int32_t *lengths, float *dist, float *frames, void *ws,
                            size_t ws_bytes, void *stream);
/* wb_frames (ABI 10): fsem_pesq_wb_f32 with the distances and per-frame disturbances of
 *        fsem_pesq_distances_f32 beside the scores (dist [2, batch], frames [batch, 2, Fcap] as
 *        there), from the rows as given: the whole-metric path's range handling, where the
 *        stage entries need rows of moderate range.  Workspace: fsem_pesq_workspace_bytes.
 *        Used by the P.862 mode's bad-interval realignment (fsem_pesq_bad_intervals_f32).
 */
int fsem_pesq_wb_frames_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                            int64_t ld, const int32_t *lengths, float *mos, float *dist, float *frames,
                            void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- STOI / ESTOI
 * Whole-metric entry: replaces STOI.compute_stoi + compute_metric
 *   fast_se_metrics/STOI.py:153-205 (after BaseMetric resampling to 10 kHz,
 *   base.py:19-20, when sample_rate != 10000).
 *   ref, deg    : [batch, length] float32 at `sample_rate` (row stride ld)
 *   lengths     : NULL or [batch] int32 per-row lengths at `sample_rate` (Conventions)
 *   stoi, estoi : [batch] float32 outputs; NaN where no 30-frame segment exists
 *                 (the reference warns there, STOI.py:163-165).
 */
size_t fsem_stoi_workspace_bytes(int64_t batch, int64_t length, int32_t sample_rate);
int fsem_stoi_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                  int64_t ld, const int32_t *lengths, int32_t sample_rate, float *stoi,
                  float *estoi, void *ws, size_t ws_bytes, void *stream);

/* Intermediates of the 10 kHz STOI pipeline for parity tests:
 *   kept  [batch] int32   -- frames kept by remove_silent_frames (STOI.py:88-111)
 *   tob   [2*batch, 15, tmax] float32 third-octave band envelopes (STOI.py:121-125),
 *         rows 0..B-1 ref, B..2B-1 deg; frames >= kept-2 are left untouched.
 * Input must already be at 10 kHz (length = 10 kHz samples).
 */
int fsem_stoi_tob_f32(const float *ref10, const float *deg10, int64_t batch,
                      int64_t length10, int64_t ld, int32_t *kept, float *tob, int64_t tmax,
                      void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- joint PESQ + STOI
 * Both metrics of 16 kHz pairs from ONE read of the inputs: replaces the
 * reference's two calls PESQ(16000).compute_metric (PESQ.py:232-245) and
 * STOI(16000)(...) (base.py:19-20 resampling + STOI.py:153-205).  The PESQ front end's LDS
 * tiles also feed the fused 16 -> 10 kHz resampler.  Scores are bitwise those of
 * fsem_pesq_wb_f32 and fsem_stoi_f32(sample_rate = 16000) on the same rows.
 *   lengths : NULL or [batch] int32 per-row lengths (Conventions)
 *   mos, stoi, estoi : [batch] float32 outputs
 * FSEM_ESHORT (whole-batch form) when either metric's minimum length is not met.
 */
size_t fsem_pesq_stoi_workspace_bytes(int64_t batch, int64_t length);
int fsem_pesq_stoi_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                       int64_t ld, const int32_t *lengths, float *mos, float *stoi, float *estoi,
                       void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- time alignment (opt-in)
 * NOT in the reference, whose PESQ has no time alignment (fast_se_metrics/PESQ.py:19-22); the
 * PESQ(..., time_align=True) extension calls this before the PESQ entries.
 * Per row pair of 16 kHz signals, after ITU-T P.862 section 10 (restated in
 * oracle/align_oracle.py; parity against P.862 implementations unpinned):
 *   crude delay from 4 ms voice-activity log envelopes (|delay| <= max_delay samples, rounded
 *   up to 4 ms frames), then the sample lag within +-383 of it maximising the cross-correlation
 *   of the signals' first differences.  delay[b] = D > 0: deg lags ref, deg[n] ~ ref[n - D].
 *   ref, deg    : [batch, length] float32 (row stride ld, ld % 4 == 0, 16-byte aligned rows)
 *   lengths     : NULL or [batch] int32 per-row lengths (Conventions)
 *   delay       : NULL or [batch] int32 output (at least one of delay / deg_aligned)
 *   deg_aligned : NULL or [batch, length] float32 output (row stride ld_out, ld_out % 4 == 0,
 *                 16-byte aligned rows):
 *                 deg_aligned[b][n] = deg[b][n + D] where 0 <= n + D < lengths[b], else 0
 *                 (not in place: deg_aligned must not overlap deg)
 * Cost: dominated by the fine search (fast correlation per 1280-sample block); see csrc/align.hip.
 */
size_t fsem_time_align_workspace_bytes(int64_t batch, int64_t length);
int fsem_time_align_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                        int64_t ld, const int32_t *lengths, int32_t max_delay, int32_t *delay,
                        float *deg_aligned, int64_t ld_out, void *ws, size_t ws_bytes,
                        void *stream);

/* utterance mode (ABI 5): P.862's per-utterance alignment (sections 10.3-10.5, restated in
 * oracle/align_oracle.py steps 5-9; parity against P.862 implementations unpinned):
 *   utterances of the reference (envelope speech runs of 16 ms or more, joined across gaps < 200 ms, at
 *   least 200 ms, at most 16 per row) each own a region of the row (boundaries in the middle of
 *   the gaps); per utterance a crude delay (envelope correlation over the utterance +-300 ms,
 *   within +-300 ms of the row's crude delay), then the fine delay of its region as above; a
 *   region splits once at a 5120-sample piece boundary when two delays (>= 16 samples apart)
 *   raise the summed correlation peak by 20 %.  Consecutive segments of equal delay are merged.
 *   delay     : NULL or [batch] int32: the row's longest segment's delay (first of equals)
 *   n_seg     : NULL or [batch] int32 segment counts (1 .. FSEM_ALIGN_MAX_SEGMENTS)
 *   seg_start : NULL or [batch, FSEM_ALIGN_MAX_SEGMENTS + 1] int32: segment k of row b covers
 *               samples [seg_start[b][k], seg_start[b][k + 1]); seg_start[b][n_seg[b]] = lengths[b]
 *   seg_delay : NULL or [batch, FSEM_ALIGN_MAX_SEGMENTS] int32 delays (n_seg, seg_start and
 *               seg_delay: all three or none; at least one of delay / n_seg / deg_aligned)
 *   deg_aligned[b][n] = deg[b][n + D_k] for n in segment k where 0 <= n + D_k < lengths[b], else 0
 * Other arguments as fsem_time_align_f32.
 */
#define FSEM_ALIGN_MAX_SEGMENTS 32
size_t fsem_time_align_utt_workspace_bytes(int64_t batch, int64_t length);
int fsem_time_align_utt_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                            int64_t ld, const int32_t *lengths, int32_t max_delay, int32_t *delay,
                            int32_t *n_seg, int32_t *seg_start, int32_t *seg_delay,
                            float *deg_aligned, int64_t ld_out, void *ws, size_t ws_bytes,
                            void *stream);

/* P.862 mode (ABI 8): the utterance mode's stages up to the per-piece correlations, then P.862's
 * histogram fine alignment and recursive utterance split (sections 10.5-10.6, restated in
 * oracle/align_oracle.py steps 10-12 on the 5120-sample pieces instead of P.862's 64 ms frames;
 * parity against P.862 implementations unpinned): every piece whose correlation peak reaches
 * 5 % of its utterance's largest votes for its peak lag with weight peak^0.125; a range of
 * pieces takes the first maximum of its triangle-smoothed (+-8 lags) vote histogram as delay and
 * that maximum's share of the votes as confidence; a range splits at the piece boundary whose two
 * halves (two or more votes each, delays >= 16 samples apart) are both more confident than the
 * whole, the largest summed confidence first, and each half is tried once more (up to 4 segments
 * per utterance; at most FSEM_ALIGN_MAX_SEGMENTS per row, later ones merging into the last).
 * Arguments, outputs and workspace rules as fsem_time_align_utt_f32.  Replaces nothing in the
 * reference (its PESQ has no time alignment, fast_se_metrics/PESQ.py:19-22).
 */
size_t fsem_time_align_p862_workspace_bytes(int64_t batch, int64_t length);
int fsem_time_align_p862_f32(const float *ref, const float *deg, int64_t batch, int64_t length,
                             int64_t ld, const int32_t *lengths, int32_t max_delay, int32_t *delay,
                             int32_t *n_seg, int32_t *seg_start, int32_t *seg_delay,
                             float *deg_aligned, int64_t ld_out, void *ws, size_t ws_bytes,
                             void *stream);

/* bad intervals (ABI 9): P.862's realignment of bad intervals after the perceptual model (section
 * 10.7, restated in oracle/align_oracle.py steps 13-15; parity against P.862 implementations
 * unpinned), for the P.862 mode's rows.  Replaces nothing in the reference.
 *   deg_aligned : [batch, length] float32 (row stride ld_out): fsem_time_align_p862_f32's output
 *   frames      : [batch, 2, Fcap] float32 (Fcap = fsem_pesq_frames(length)): the per-frame
 *                 disturbances of (ref, deg_aligned), fsem_pesq_wb_frames_f32's (or
 *                 fsem_pesq_distances_f32's)
 *   n_seg, seg_start, seg_delay : that alignment's segments
 *   n_bad       : [batch] int32 output: intervals per row (0 .. FSEM_PESQ_MAX_BAD)
 *   bad         : [batch, FSEM_PESQ_MAX_BAD, 3] int32 output: {first frame, end frame, delay} --
 *                 runs of frames with symmetric disturbance > 30, joined across gaps < 4 frames,
 *                 from 5 frames long, in order; delay: the first maximum of the first-difference
 *                 correlation over the interval's samples [256 f0, min(256 f1 + 256, lengths[b]))
 *                 within +-383 of the delay of the segment holding its first sample (that delay
 *                 when no lag correlates positively)
 *   deg_second  : [batch, length] float32 output (row stride ld_out; may be deg_aligned itself):
 *                 deg[b][n + delay_i] for n in interval i (0 <= n + delay_i < lengths[b], else 0),
 *                 deg_aligned[b][n] elsewhere
 * pool: the MOS of each row from the first frames, an interval taking frames2 (the per-frame
 *   disturbances of (ref, deg_second)) when their symmetric sum over it is smaller; the pooling
 *   and mapping of fsem_pesq_wb_f32 (PESQ.py:168-172, 240-243).  dist: [2, batch] the first
 *   distances (NaN there gives NaN); rows under 20 frames give NaN.
 */
#define FSEM_PESQ_MAX_BAD 16
size_t fsem_pesq_bad_intervals_workspace_bytes(int64_t batch, int64_t length);
int fsem_pesq_bad_intervals_f32(const float *ref, const float *deg, const float *deg_aligned, int64_t batch,
                                int64_t length, int64_t ld, const int32_t *lengths, const float *frames,
                                const int32_t *n_seg, const int32_t *seg_start, const int32_t *seg_delay,
                                int32_t *n_bad, int32_t *bad, float *deg_second, int64_t ld_out, void *ws,
                                size_t ws_bytes, void *stream);
int fsem_pesq_pool_f32(const float *frames, const float *frames2, const float *dist, int64_t batch,
                       int64_t length, const int32_t *lengths, const int32_t *n_bad, const int32_t *bad,
                       float *mos, void *stream);

/* ---------------------------------------------------------------- SDR: SI-SDR, SNR, segmental SNR
 * (ABI 11) Replaces nothing in the reference, which has no energy-ratio metric.  Three numbers in
 * dB per row pair, from ONE read of the inputs, at the rows' own `sample_rate` (no resampling);
 * s = the clean row's first n samples, s^ = the denoised row's, d = s^ - s, n = the row's length:
 *   snr     : 10 log10(sum s^2 / sum d^2)
 *   si_sdr  : 10 log10(T / N), T = (sum s s^)^2 / sum s^2, N = max(sum s^^2 - T, 0) (Le Roux et al.
 *             2019); zero_mean != 0 removes each row's own mean over its n samples first (SI-SDR
 *             only).  NaN when sum s^2 == 0 or sum s^^2 == 0; +inf when s^ == s sample for sample
 *             (snr too); -inf when sum s s^ == 0 with sum s^^2 > 0.  The sums are accumulated in
 *             double: accurate while the true value lies within +-100 dB; beyond, the sign and "at
 *             least 100 dB in magnitude, or +-inf" hold.
 *   seg_snr : Hu & Loizou's segmental SNR.  hop = sample_rate * 30 / 4000 samples (integer division:
 *             120 at 16 kHz, 165 at 22.05 kHz), win = 4 hop, w[t] = 0.5 (1 - cos(2 pi (t + 1) /
 *             (win + 1))), t < win; the F = (n - win) / hop + 1 complete frames (0 when n < win);
 *             per frame v = clamp(10 log10(sum (w s)^2 / (sum (w d)^2 + 1e-10) + 1e-10), -10, 35);
 *             the mean of v over the frames, NaN when F == 0.  The 1e-10 terms make it scale
 *             dependent by definition: the documented domain is float rows up to int16 range
 *             (|x| <= 32768).  float32 sums per window quarter.
 * A row holding a non-finite sample gives NaN in all three (other rows are unaffected), and so does
 * a row of length 0.  There is no FSEM_ESHORT: short rows are NaN in seg_snr only.
 *   ref, deg : [batch, length] float32 (row stride ld); rows readable up to ceil4(length) floats;
 *              16-byte loads when both base pointers are 16-byte aligned and ld % 4 == 0, else
 *              4-byte loads (same scores)
 *   lengths  : NULL or [batch] int32 per-row lengths (Conventions)
 *   si_sdr, snr, seg_snr : [batch] float32 outputs
 * A row's scores are bitwise the same whatever the batch size, the row's position, `length` and the
 * stream (no atomics; every sum has one order, fixed by sample_rate).
 * sample_rate 4000 ... 192000 Hz; others give FSEM_ERATE and the queries return 0.
 */
int64_t fsem_sdr_hop(int32_t sample_rate);                     /* 0 when unsupported */
int64_t fsem_sdr_frames(int64_t length, int32_t sample_rate);  /* F above */
int64_t fsem_sdr_chunk(int32_t sample_rate);  /* samples per launch chunk: k * hop, from sample_rate only */
size_t fsem_sdr_workspace_bytes(int64_t batch, int64_t length, int32_t sample_rate);
int fsem_sdr_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                 const int32_t *lengths, int32_t sample_rate, int32_t zero_mean, float *si_sdr, float *snr,
                 float *seg_snr, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------- Spectral: fwSegSNR, CD, IS
 * (ABI 11: fsem_version() stays 11; these entries take no workspace and change no other entry.)
 * Replaces nothing in the reference.  Three measures of Hu & Loizou's evaluation set per row pair:
 * the frequency-weighted segmental SNR (fwSegSNR, dB), the LPC cepstral distance (CD, dB) and the
 * Itakura-Saito distance (IS), with their per-frame values as a caller-provided output.  No
 * implementation of Loizou's comp_fwseg.m, comp_cep.m and comp_is.m was available to compare with:
 * agreement with them is by definition only.  0-based indices throughout.
 *
 * Shared with Composite.  Per row, s and s^ are the first n samples of the clean and the denoised
 * row.  The window w, hop, win, the F complete frames, the LPC order P, nfft (512 or 1024),
 * H = nfft / 2 and the 25 band filters g_i[j] with their threshold are exactly those of
 * include/fsem_composite.h (frames: SegSNR's, F = fsem_sdr_frames(n, sample_rate)).
 *
 * LPC quantities.  As for LLR: R_x[k] = sum_t x[t] x[t + k] over the windowed frame,
 * A_x = [1, a_1 ... a_P] from Levinson-Durbin on R_x, T_x the Toeplitz matrix of R_x.
 *
 * CD_f.
 *  - Cepstrum of 1 / A(z): c[1] = -a[1]; c[m] = -a[m] - sum_{k=1}^{m-1} (k / m) c[k] a[m - k], m = 2 ... P.
 *  - CD_f = min(10, (10 / ln 10) sqrt(2 sum_{m=1}^{P} (c_s[m] - c_s^[m])^2)).
 *
 * IS_f.
 *  - E_x = A_x T_x A_x'.
 *  - IS_f = min(100, (A_s^ T_s A_s^') / E_s^ + ln(E_s^ / E_s) - 1).
 *
 * NaN frames (CD, IS).  A frame with R[0] == 0 in either signal is NaN in CD_f and IS_f, by 0 / 0,
 * as for LLR.
 *
 * fwSegSNR_f.
 *  - M_x[j] = |FFT_nfft(frame)[j]|, j < H.
 *  - m_x = M_x / sum_j M_x, or all zeros when that sum is 0.
 *  - e_x[i] = sum_j m_x[j] g_i[j].
 *  - err[i] = max((e_s[i] - e_s^[i])^2, 2^-52).
 *  - W[i] = e_s[i]^0.2.
 *  - v = sum_i W[i] 10 log10(e_s[i]^2 / err[i]) / sum_i W[i], over the bands with W[i] > 0.
 *  - fwSegSNR_f = clamp(v, -10, 35); NaN when no band has W[i] > 0 (a digitally silent clean frame).
 *
 * Row values.
 *  - CD and IS follow Composite's rule for LLR: the mean of the K = (19 F + 10) / 20 smallest frame
 *    values, NaN sorted last; NaN when a NaN lies among the K or when F = 0.
 *  - fwSegSNR is the mean of all F frame values; NaN when any frame is NaN or when F = 0.  A row kept
 *    NaN by silent clean frames is a convention: callers can take their own mean of `frames`.
 *  - A row holding a non-finite sample among its first n (also in the tail that no frame covers), or
 *    a row of length 0, is NaN in all three scores; other rows are unaffected.  The row kernel scans
 *    the row's samples itself.  The frame values of such a row are whatever the arithmetic gives.
 *  - The reduction, for recomputing a score from `frames` bit for bit: thread t of 256 adds its
 *    values v[t], v[t + 256], ... in that order in double -- for CD and IS only those below the
 *    K-th smallest value x_K in the floats' order; the 256 sums are added by halving
 *    (u[i] += u[i + h] for i < h; h = 128, 64 ... 1); CD and IS then add c x_K, c the number of
 *    copies of x_K among the K smallest; the total is divided by K (fwSegSNR: F) in double and
 *    rounded to float32.
 *
 * Precision.  The window product is float32.  The autocorrelation, Levinson-Durbin, the cepstrum,
 * the quadratic forms, ln and sqrt are double.  The spectra, magnitudes, their normalisation and the
 * band sums are float32.  The band log ratio and the weighted mean are double.  Frame values are
 * stored as float32; the row sums are accumulated in double in the one order above.  Clean and
 * denoised never share one complex transform (a silent frame has an exactly zero spectrum).
 *   ref, deg : [batch, length] float32 (row stride ld >= length); read 4 bytes at a time, at any
 *              alignment
 *   lengths  : NULL or [batch] int32 per-row lengths (Conventions)
 *   frames   : [3][batch][ldf] float32, required; plane k holds measure k (fwSegSNR, CD, IS): row b,
 *              frame f at frames[(k * batch + b) * ldf + f]; ldf >= max(F, 1), F of `length`; with
 *              `lengths`, the entries past a row's own F are left unwritten
 *   fwsegsnr, cd, is_ : [batch] float32 outputs
 * Null pointers, ldf < F, batch < 0, ld < length and rows past 2^29 samples give FSEM_EINVAL before
 * any launch; sample_rate other than 8000 or 16000 gives FSEM_ERATE (fsem_spectral_order: 0).
 * batch == 0 gives FSEM_OK with nothing launched; length == 0 gives FSEM_OK with no frame kernel
 * launched and every score NaN.  No hidden device allocation, no workspace, no atomics whose order
 * can change a result (integer histogram counts only).  A row's three scores and its frame values
 * are bitwise the same whatever the batch size, the row's position, `length`, `ld`, `ldf` and the
 * stream.
 */
int fsem_spectral_order(int32_t sample_rate);  /* LPC order P: 10 at 8000, 16 at 16000, 0 otherwise */
int fsem_spectral_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                      const int32_t *lengths, int32_t sample_rate, float *frames, int64_t ldf, float *fwsegsnr,
                      float *cd, float *is_, void *stream);

/* ---------------------------------------------------------------- SRMR
 * The speech-to-reverberation modulation energy ratio of a row (Falk, Zheng & Chan 2010), a
 * no-reference measure: SRMRpy's full path (fast=False, norm=False, 23 channels, low_freq=125,
 * min_cf=4, max_cf=128) with one change, the envelope (below).  An extension: the reference has no
 * such measure.  Rows are scored at sample_rate fs, 8000 or 16000 Hz; a row holds n samples x[0 .. n).
 *
 * Centre frequencies.  EarQ = 9.26449, minBW = 24.7, c = EarQ minBW.  For i = 1 ... 23:
 *   cf_i = -c + exp(i (ln(125 + c) - ln(fs / 2 + c)) / 23) (fs / 2 + c)
 * (descending, cf_23 = 125); ERB(f) = f / EarQ + minBW.
 *
 * Analytic gammatone.  p_i = exp((-2 pi 1.019 ERB(cf_i) + j 2 pi cf_i) / fs).  Channel i has the complex
 * impulse response h_i[m] = m^3 p_i^m / g_i, m >= 0 (the impulse-invariant sampling of t^3 e^{st}):
 *   G_p(z) = p z^-1 (1 + 4 p z^-1 + p^2 z^-2) / (1 - p z^-1)^4,
 * run from a zero state as the three-tap numerator followed by four first-order recurrences;
 * g_i = |G_p(z0) + G_conj(p)(z0)| / 2 at z0 = exp(j 2 pi cf_i / fs), the gain at cf_i of the real filter
 * Re h.  y_i = h_i * x.
 *
 * Envelope.  e_i[t] = |y_i[t]|.  (SRMRpy takes |hilbert(.)| of Slaney's real four-biquad cascade, a
 * whole-row DFT per channel; Im y_i is the quadrature gammatone, which approximates that Hilbert
 * transform.  The effect on the score: INTEGRATION.md section 13.)
 *
 * Modulation filters.  mcf_k = 4 32^(k / 7), k = 0 ... 7; Q = 2; W0 = tan(pi mcf_k / fs), B0 = W0 / Q;
 * b = [B0, 0, -B0], a = [1 + B0 + W0^2, 2 W0^2 - 2, 1 - B0 + W0^2]; m_ik = the filter (b / a[0], a / a[0])
 * applied to e_i from a zero state.
 *
 * Frames.  wl = ceil(0.256 fs) (4096 / 2048), wi = ceil(0.064 fs) (1024 / 512),
 * w[m] = 0.54 - 0.46 cos(2 pi m / wl); F = 1 + (n - wl) / wi when n >= wl, else 0.
 *   E[i, k, f] = sum_m (w[m] m_ik[f wi + m])^2,   A[i, k] = mean_f E[i, k, f]
 *             = (1 / F) sum_t m_ik[t]^2 V[t],  V[t] = sum_f w^2[t - f wi] over the row's own F frames.
 *
 * Score.  ac_i = sum_k A[i, k], total = sum_i ac_i.  Walking i = 23, 22, ... (upward in frequency) and
 * adding 100 ac_i / total, i* is the first i at which the sum is > 90; BW = ERB(cf_i*).
 * L_k = mcf_k - tan(pi mcf_k / fs) / Q fs / (2 pi); K* = 8 if BW > L_7, else 7 if BW > L_6, else 6 if
 * BW > L_5, else 5 (SRMRpy leaves K* undefined below L_4; elsewhere the rule is SRMRpy's).
 *   SRMR = sum_i sum_{k < 4} A[i, k] / sum_i sum_{4 <= k < K*} A[i, k].
 *
 * Row conventions.  A row with F = 0 (n = 0 included) or with a non-finite sample among its first n is
 * NaN, other rows are unaffected (the score kernel scans the row's samples itself; the energies of a
 * row without a frame are NaN, those of a row with a non-finite sample whatever the arithmetic
 * gives); a digitally silent row is NaN by 0 / 0.  Samples past a row's length are never read into a
 * result.
 *
 * Precision and order.  The gammatone is float32 complex (its constants p^k are formed in double and
 * rounded once), the envelope float32; the modulation filters' coefficients, state, squares and sums
 * are double.  The kernel walks a row in tiles of 4096 samples: a gammatone lane takes 16 samples, a
 * modulation lane a (filter, 128-sample segment) pair, states are carried by scans whose order depends
 * on the sample index alone; a lane adds its m^2 V[t] in sample order, the 32 lanes of a filter are
 * added in a fixed butterfly.  Sums over k and i run upward.  No floating-point atomics.
 *   deg      : [batch, length] float32 (row stride ld >= length); read 4 bytes at a time, at any alignment
 *   lengths  : NULL or [batch] int32 per-row lengths (Conventions)
 *   energies : [batch][23][8] float64, required: A[i, k] of row b at energies[(b * 23 + i - 1) * 8 + k]
 *   srmr     : [batch] float32 output
 * Null pointers, batch < 0, ld < length and rows past 2^29 samples give FSEM_EINVAL before any launch;
 * sample_rate other than 8000 or 16000 gives FSEM_ERATE (fsem_srmr_channels: 0).  batch == 0 gives
 * FSEM_OK with nothing launched; length == 0 gives FSEM_OK with every score NaN.  No hidden device
 * allocation, no workspace.  A row's score and energies are bitwise the same whatever the batch size,
 * the row's position, `length`, `ld` and the stream.
 */
int fsem_srmr_channels(int32_t sample_rate);  /* gammatone channels: 23 at 8000 or 16000, 0 otherwise (host query) */
int fsem_srmr_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                  int32_t sample_rate, double *energies, float *srmr, void *stream);

/* ---------------------------------------------------------------- BSS-eval (SDR, SIR, SAR of mixtures)
 * The energy ratios of mir_eval.separation.bss_eval_sources with a 512-tap distortion filter, for
 * mixtures of several sources; fsem_bsssdr_f32 (fsem_bsssdr.h) is its one-source SDR.  An extension:
 * the reference has no such metric.  Rows are scored as 16 kHz rows; 0-based indices.
 *
 * A mixture b has S sources s_i (i < S <= 4), E estimates h_e (e < E <= 4) and n = lengths[b] samples.
 *  - Normalisation, every row, exactly as fsem_bsssdr.h states it: x' = x / max(|x|, 1e-6), the norm in
 *    double rounded to float32, a float32 quotient.  Everything below is double.
 *  - Correlations, k = 0 ... 511, samples outside [0, n) zero:
 *      C_ij[k] = sum_t s'_i[t] s'_j[t + k] for all S^2 ordered pairs (C_ij[-k] = C_ji[k]),
 *      b_ie[k] = sum_t s'_i[t] h'_e[t + k].
 *  - Projections: coh[i, e] = b_ie^T T_i^-1 b_ie with T_i = Toeplitz(C_ii) (fsem_bsssdr_f32's coh of the
 *    pair (i, e)); coh_all[e] = d^T G^-1 d with the S 512 x S 512 Gram matrix
 *    G[(i, k), (j, l)] = C_ij[k - l] and d[(i, k)] = b_ie[k]: the energy of the projection of h'_e on
 *    the 512 delays of all sources.  For S == 1, coh_all[e] is coh[0, e] itself.
 *  - Scores, every denominator and every ratio clamped below at 1e-8 (all values within [-80, 80] dB):
 *      SDR[i, e] = 10 log10(coh / (1 - coh)),  SIR[i, e] = 10 log10(coh / (coh_all[e] - coh)),
 *      SAR[e] = 10 log10(coh_all / (1 - coh_all)).
 *    These are bss_eval_sources' energies of s_target, e_interf and e_artif for the unit-norm estimate:
 *    |e_interf|^2 = coh_all - coh (one source's span lies inside the span of all), |e_artif|^2 =
 *    1 - coh_all.  A silent estimate gives -80 / -80 / -80; an estimate without interference (S == 1
 *    included) has SIR = 80 + 10 log10(coh).
 *  - NaN rule.  All outputs of a mixture are NaN (perm: the identity), and only that mixture's, when
 *    any of its samples is non-finite, a source is silent (C_ii[0] == 0), n + 511 < S 512 (the delayed
 *    sources cannot be independent; checked from n), or a recursion breaks down (a prediction-error
 *    matrix that is not positive definite).  Exactly collinear sources are outside the definition:
 *    whether rounding lets the recursion run through is not specified.
 *  - Assignment.  With criterion 1 (SIR, as mir_eval) or 2 (SDR) and E == S, over the S! assignments
 *    p (estimate e <-> source p[e]) in itertools.permutations order, the one with the largest mean over
 *    e of the criterion's matrix entry [p[e], e] (summed over ascending e, divided by S, in double);
 *    equal means keep the earlier assignment.  Otherwise p[e] = e.  Per estimate: SDR[p[e], e],
 *    SIR[p[e], e], SAR[e], perm[e] = p[e].
 *
 * Two entries: fsem_bsseval_f32 forms the projections' energies, fsem_bsseval_scores_f32 turns them
 * into scores (so SDRi needs no second scoring of the sources, and a test can hand it energies).
 *   src, est : [batch, n_src, length] and [batch, n_est, length] float32; source row (b, i) starts at
 *              src + (b n_src + i) ld, the estimates likewise; read 4 bytes at a time, at any alignment
 *   lengths  : NULL or [batch] int32, one length per MIXTURE (Conventions)
 *   norms    : [batch, n_src + n_est] float32 output, the rows' norms, sources first
 *   corr     : [batch, fsem_bsseval_corr_doubles(n_src, n_est, length)] float64, the entry's only
 *              scratch.  On return a mixture's block begins with the summed C_ij (all ordered pairs,
 *              i-major: C_ij at (i n_src + j) 512) and then b_ie (at (n_src^2 + i n_est + e) 512), 512
 *              doubles each; the per-chunk partial records and the norms' records follow.
 *   coh      : [batch, n_src, n_est] float64;  coh_all : [batch, n_est] float64
 *   criterion: 0 none, 1 SIR, 2 SDR
 *   sdr, sir, sar : [batch, n_est] float32;  perm : [batch, n_est] int32
 *   sdr_mat, sir_mat : NULL or [batch, n_src, n_est] float32
 * Order of the sums (each depends on n alone): the sums of squares per chunk of 8192 samples, the
 * correlations per chunk of 32768 samples exactly as fsem_bsssdr_f32 orders them (four consecutive
 * quarters of each 2048-sample piece, added as ((q0 + q1) + q2) + q3), chunks in ascending order; the
 * recursions are (block) Levinson recursions of one wave, their inner products added over the lanes'
 * blocks l, l + 64, ... in ascending order and then by one xor butterfly.  No atomics, no hidden
 * allocation.  A mixture's outputs are bitwise the same whatever the batch size, the mixture's
 * position, `length`, `ld` and the stream.
 * FSEM_EINVAL before any launch for null pointers (sdr_mat, sir_mat and lengths may be NULL), batch < 0,
 * n_src or n_est outside 1 ... 4, length < 1, ld < length, length > 2^29, a criterion outside 0 ... 2,
 * and, for the scores, n_est > n_src (p[e] = e names no source).  batch == 0 is FSEM_OK with nothing
 * launched.
 */
int fsem_bsseval_max_sources(void);  /* 4 (host query) */
int64_t fsem_bsseval_corr_doubles(int32_t n_src, int32_t n_est, int64_t length);  /* per mixture; 0 for refused arguments */
int fsem_bsseval_f32(const float *src, const float *est, int64_t batch, int32_t n_src, int32_t n_est, int64_t length,
                     int64_t ld, const int32_t *lengths, float *norms, double *corr, double *coh, double *coh_all,
                     void *stream);
int fsem_bsseval_scores_f32(const double *coh, const double *coh_all, int64_t batch, int32_t n_src, int32_t n_est,
                            int32_t criterion, float *sdr, float *sir, float *sar, int32_t *perm, float *sdr_mat,
                            float *sir_mat, void *stream);

/* ---------------------------------------------------------------- PITSDR (SI-SDR and SNR of mixtures, with gradients)
 * The scale-invariant SDR and the SNR of every estimate against every source of a mixture, the best
 * assignment, and the gradient of both matrices with respect to the estimates.  An extension: the
 * reference has no such metric.  Rows are scored at their own sample_rate (no resampling); 0-based.
 *
 * A mixture b has S sources s_i (i < S <= 4), E estimates h_e (e < E <= S) and n = lengths[b] samples.
 *  - Pair scores.  SNR[i, e] = 10 log10(sum s_i^2 / sum (h_e - s_i)^2).  SI-SDR[i, e] is si_sdr of "SDR"
 *    above for the pair (s_i, h_e), zero_mean and every NaN / +-inf rule included.  All sums in double
 *    (products of float32 samples are exact there).
 *  - Non-finite samples.  A mixture with a non-finite sample among its (S + E) n, or with n == 0, is NaN
 *    in every entry of both matrices (perm: the identity); other mixtures are unaffected.
 *  - Assignment.  With criterion 1 (SI-SDR) or 2 (SNR), E == S and no NaN in the mixture's criterion
 *    matrix: over the S! assignments p (estimate e <-> source p[e]) in itertools.permutations order, the
 *    one with the largest mean over e of the matrix entry [p[e], e] (the double values, summed over
 *    ascending e, divided by S); equal means keep the earlier assignment, a NaN mean (+inf and -inf
 *    entries) never wins.  Otherwise p[e] = e.  perm[b, e] = p[e].
 *  - Gradient.  With k = 20 / ln 10 and incoming gradients G_si, G_snr [batch, S, E] of the two matrices,
 *      grad[b, e, t] = sum_i A[i, e] s_i[t] + C[e] h_e[t] + K[e]  for t < n, 0 for n <= t < length
 *      A[i, e] = k G_si[i, e] (1 / sh + sh / (ss nn)) + k G_snr[i, e] / dd
 *      C[e]    = -k sum_i (G_si[i, e] / nn + G_snr[i, e] / dd)
 *      K[e]    = -sum_i A_si[i, e] mean(s_i) - C_si[e] mean(h_e)  with zero_mean (the SI-SDR terms of A
 *                and C alone), else 0
 *    with ss = sum s_i^2, sh = sum s_i h_e, nn = sum h_e^2 - sh^2 / ss (the centred sums with zero_mean)
 *    and dd = sum (h_e - s_i)^2.  A pair's SI-SDR (SNR) terms are left out when its SI-SDR (SNR) is not
 *    finite; a NaN mixture's gradient is zero.  A, C and K are formed in double from the forward's
 *    totals and rounded to float32; the sum over i (ascending, K first, C h last) is float32 FMAs.
 *
 *   src, est : [batch, n_src, length] and [batch, n_est, length] float32; source row (b, i) starts at
 *              src + (b n_src + i) ld, estimate row (b, e) at est + (b n_est + e) ld.  16-byte loads
 *              where both bases are 16-byte aligned and ld % 4 == 0 (only inside the first n samples),
 *              4-byte loads otherwise: the same results.  No sample past n is read.
 *   lengths  : NULL or [batch] int32, one length per MIXTURE (Conventions)
 *   criterion: 0 none, 1 SI-SDR, 2 SNR
 *   sums     : [batch, fsem_pitsdr_sums_doubles(n_src, n_est, length, sample_rate)] float64, the entries'
 *              only scratch, owned by the caller.  A mixture's block: the totals, then one record per
 *              chunk of fsem_pitsdr_chunk samples, each ss[S], hh[E], s1[S], h1[E], sh[S E], dd[S E]
 *              (pair (i, e) at i E + e; s1, h1 the plain sums).  fsem_pitsdr_f32 leaves the totals
 *              there; fsem_pitsdr_grad_f32 reads them (same batch, shape, length and lengths).
 *   si_mat, snr_mat : [batch, n_src, n_est] float32;  perm : [batch, n_est] int32
 *   g_si, g_snr : [batch, n_src, n_est] float32
 *   grad     : [batch, n_est, length] float32, row (b, e) at grad + (b n_est + e) grad_ld; every one of
 *              the `length` elements of each row is written (16-byte stores where src, est and grad are
 *              16-byte aligned and ld % 4 == grad_ld % 4 == 0)
 * Order of the sums: per chunk, thread t of 256 adds the float4s t, t + 256, ... in ascending order,
 * the wave's 64 values by a fixed exchange, the four waves as ((w0 + w1) + w2) + w3; the chunks in
 * ascending order.  No atomics, no hidden allocation.  A mixture's outputs are bitwise the same
 * whatever the batch size, the mixture's position, `length`, `ld`, the loads' width and the stream.
 * FSEM_EINVAL before any launch for null pointers (lengths may be NULL), batch < 0, n_src outside
 * 1 ... 4, n_est outside 1 ... n_src, length < 1, length > 2^29, ld < length, grad_ld < length, a criterion
 * outside 0 ... 2; then FSEM_ERATE for a sample_rate outside 4000 ... 192000 (the queries return 0).
 * batch == 0 is FSEM_OK with nothing launched.
 */
int fsem_pitsdr_max_sources(void);                /* 4 (host query) */
int64_t fsem_pitsdr_chunk(int32_t sample_rate);   /* samples per chunk: 8192 at every supported rate */
int64_t fsem_pitsdr_sums_doubles(int32_t n_src, int32_t n_est, int64_t length, int32_t sample_rate);  /* per mixture: (2 S + 2 E + 2 S E) (1 + chunks); 0 for refused arguments */
int fsem_pitsdr_f32(const float *src, const float *est, int64_t batch, int32_t n_src, int32_t n_est, int64_t length,
                    int64_t ld, const int32_t *lengths, int32_t sample_rate, int32_t zero_mean, int32_t criterion,
                    double *sums, float *si_mat, float *snr_mat, int32_t *perm, void *stream);
int fsem_pitsdr_grad_f32(const float *src, const float *est, int64_t batch, int32_t n_src, int32_t n_est,
                         int64_t length, int64_t ld, const int32_t *lengths, int32_t zero_mean, const double *sums,
                         const float *g_si, const float *g_snr, float *grad, int64_t grad_ld, void *stream);

/* ---------------------------------------------------------------- STOI with gradients
 * STOI and ESTOI of fsem_stoi_f32 as a function to train against: the scores, and the gradient of
 *   L = sum_b (g_stoi[b] STOI_b + g_estoi[b] ESTOI_b)
 * with respect to the denoised rows at the input rate.  (Joined at ABI 11 without a bump, as above.)
 * The function differentiated is STOI above with the reference's 1e-12 * randn terms in expectation, as
 * the forward takes them: the resampler, the selection of frames by the CLEAN rows' energies (a constant),
 * the overlap-add of the kept frames, the STFT, the band envelopes sqrt(sum |Z|^2), the segments'
 * equalisation alpha = |x| / (|y| + 1e-9), the clipping min(alpha y, (1 + 10^(15/20)) x), both
 * normalisations with their N 1e-24 regularisers and the (14/15) sum 1e-24 / n2 term of the band
 * normalisation, all differentiated as written.
 *  - Clean rows are constants: no gradient with respect to ref.
 *  - A row without a 30-frame segment (scores NaN) and a row with a non-finite denoised sample among its
 *    lengths[b] samples get a gradient row of exact zeros; no other row is touched.
 *  - Where a denoised band envelope is exactly 0 (e.g. an all-zero row) the square root has no
 *    derivative: the subgradient 0 is taken there, so an all-zero estimate has a zero, finite gradient.
 *    Likewise |y| = 0 in alpha.  At the clipping's min the side alpha y < (1 + 10^(15/20)) x is the
 *    denoised one (ties have measure zero).
 *  - With lengths, grad[b, lengths[b] .. length) is zero and row b's gradient is that of the unpadded row.
 *  - A row's gradient does not depend on the batch it is in, and two calls give the same bits: every
 *    sum is a gather or a store-then-sum in a fixed order; no atomics, no hidden allocation.
 *
 *   state    : [fsem_stoi_state_floats(batch, length, sample_rate)] float32, owned by the caller, 256-byte
 *              aligned.  Its head is the workspace of fsem_stoi_f32, laid out as that entry lays it
 *              out (fsem_stoi_workspace_bytes: per row the VAD sums, the kept frame indices and count, both
 *              envelope sets [2, 15, tmax], the segment block sums and both 10 kHz rows [2, ceil64(L10)]),
 *              which fsem_stoi_state_f32 leaves filled; its tail is the backward's scratch: per row one
 *              flag, the kept position of each frame [ceil64(frames)], the envelope derivatives [ceil((tmax - 29) / 64), 15, 96], the frame derivatives
 *              [tmax, 256] and, unless sample_rate is 10000, the 10 kHz row's derivative [ceil64(L10)]
 *              (L10 = ceil(length * 10000 / sample_rate), tmax = (L10 - 256) / 128 - 1): about
 *              (2 + 0.23 + 2 + 1) L10 * 4 bytes per row beside the forward's (2 + 0.23) L10 * 4,
 *              e.g. 0.87 MB per 4 s row at 16 kHz, 0.36 MB of it the forward's.
 *   fsem_stoi_state_f32 : the scores of fsem_stoi_f32, bitwise (the same kernels on the state's head).
 *              FSEM_ESHORT as there.
 *   fsem_stoi_grad_f32  : reads the state fsem_stoi_state_f32 left for the same deg, batch, length, ld,
 *              lengths and sample_rate, writes the tail, and writes every element of grad[b, 0 .. length)
 *              (row b at grad + b grad_ld).  It may be called again on the same state.
 *   segments : NULL or [batch] int32: the 30-frame segments of each row (kept frames - 31; 0: the row
 *              scores NaN and gets no gradient).
 *   g_stoi, g_estoi : [batch] float32 device arrays.
 * FSEM_EINVAL before any launch for null pointers (lengths may be NULL), batch < 0, length <= 0,
 * length > 2^29, ld < length, grad_ld < length; then FSEM_ERATE for a rate without a resampling kernel
 * (fsem_stoi_state_floats returns 0 for any of these).  batch == 0 is FSEM_OK with nothing launched.
 */
int64_t fsem_stoi_state_floats(int64_t batch, int64_t length, int32_t sample_rate);  /* 0 for refused arguments */
int fsem_stoi_state_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                        const int32_t *lengths, int32_t sample_rate, float *stoi_out, float *estoi_out,
                        int32_t *segments, float *state, void *stream);
int fsem_stoi_grad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                       int32_t sample_rate, float *state, const float *g_stoi, const float *g_estoi,
                       float *grad, int64_t grad_ld, void *stream);

/* ---------------------------------------------------------------- PESQ with gradients
 * The wideband PESQ of fsem_pesq_wb_f32 as a function to train against: the scores, and the gradient of
 *   L = sum_b (g_mos[b] MOS_b + g_sym[b] d_sym_b + g_asym[b] d_asym_b)
 * with respect to the denoised rows at 16 kHz.  (Joined at ABI 11 without a bump, as above.)
 * The function differentiated is "PESQ" above taken as a function of the denoised row x of length L:
 * u = BP(x) from zero state and P = sum u^2; sigma = 1e7 (L + 5120) 1.04684 / P; the row times sqrt(sigma),
 * times the 15-sample edge tapers, through the pre-emphasis IIR, padded by L % 256; Hann-512 frames at hop
 * 256, |rFFT|^2 with bin 0 zeroed and bin 256 unused; the Bark contraction; then the band and frame
 * equalisation, the loudness, the dead zone, both disturbances, the frame weighting, the L6 / L2 pooling and
 * the MOS mapping.  The equalisation of ranges cancels exactly, so the scores do not depend on the scale of x
 * and <grad, x> = 0.
 *  - Clean rows are constants: no gradient with respect to ref.
 *  - The decisions are constants of the function: the audible masks (> thr, > 100 thr), the silent-frame
 *    mask, p <= thr in the loudness, the dead zone's clamp at 0 and its sign, a < 3 -> 0.
 *  - Every clamp passes the gradient inside its range and 0 outside: the band ratio 0.01 .. 100, the frame
 *    ratio 3e-4 .. 5, a <= 12, the floor 1e-20 and the cap 45.
 *  - The symmetric disturbance sqrt(sum (w d)^2) takes the subgradient 0 where the sum is 0 (every band in
 *    the dead zone), and so does any root or power whose argument is 0; |.| has derivative 0 at 0.  The
 *    pooling runs in double, as the forward's.
 *  - A gradient row of exact zeros goes to: a row with fewer than 20 frames; a row whose score is not
 *    finite (zero band-pass power); a row with a non-finite sample among its lengths[b] samples; a row
 *    with a tile the forward's range path had to rescale (peaks outside 2^+-40).  No other row is touched,
 *    and the scores of these rows stay what fsem_pesq_wb_f32 gives.
 *  - With lengths, grad[b, lengths[b] .. length) is zero and row b's gradient is that of the unpadded row,
 *    with its own taper position and its own L % 256 padding.
 *  - A row's gradient does not depend on the batch it is in, and two calls give the same bits: every
 *    sum is a gather or a store-then-sum in a fixed order; no atomics, no hidden allocation.
 *
 *   state    : [fsem_pesq_state_floats(batch, length)] float32, owned by the caller, 256-byte aligned.  Its
 *              head is the workspace of fsem_pesq_wb_f32, laid out as that entry lays it out (the power
 *              partials, the range shifts, flags and worklist, both signals' unscaled Bark bands
 *              [2 batch, 49, ceil32(frames)], the back end's scratch), which fsem_pesq_state_f32 leaves filled;
 *              its tail is the backward's scratch: per row 6 frame rows and one of doubles, the band
 *              gradients [49, ceil32(frames)], a coefficient and a flag, and two rows of ceil256(length)
 *              samples (the pre-emphasised row and the gradient with respect to it): 1.69 MB per 10 s
 *              row, 0.26 MB of it the forward's.
 *   fsem_pesq_state_f32 : mos [batch] bitwise that of fsem_pesq_wb_f32 on the same batch (the same kernels
 *              on the state's head); dist, NULL or [2, batch], bitwise that of fsem_pesq_wb_frames_f32.
 *              FSEM_ESHORT as there.
 *   fsem_pesq_grad_f32  : reads the state fsem_pesq_state_f32 left for the same deg, batch, length, ld and
 *              lengths, writes the tail, and writes every element of grad[b, 0 .. length) (row b at
 *              grad + b grad_ld).  It may be called again on the same state.
 *   g_mos, g_sym, g_asym : [batch] float32 device arrays; g_sym and g_asym may be NULL (zeros).
 * FSEM_EINVAL before any launch for null pointers (lengths, dist, g_sym and g_asym may be NULL), batch < 0,
 * length <= 0, length > 2^29, ld < length, grad_ld < length (fsem_pesq_state_floats returns 0 for any of
 * these).  batch == 0 is FSEM_OK with nothing launched.
 */
int64_t fsem_pesq_state_floats(int64_t batch, int64_t length);  /* 0 for refused arguments */
int fsem_pesq_state_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                        const int32_t *lengths, float *mos, float *dist, float *state, void *stream);
int fsem_pesq_grad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                       float *state, const float *g_mos, const float *g_sym, const float *g_asym,
                       float *grad, int64_t grad_ld, void *stream);

/* ---------------------------------------------------------------- LSD with gradients
 * The gradient of L = sum_b g_lsd[b] LSD_b with respect to the denoised rows at 16 kHz, LSD as
 * fsem_lsd.h defines it (the forward entry fsem_lsd_f32 lives in libfsem_lsd.so; rows at another
 * rate take fsem_lsd_grad_rate_f32, below).  (Joined at
 * ABI 11 without a bump, as above.)  Per row, with s, h the first n samples, sh = sum s h, hh = sum h h,
 * a = sh / (hh + 1e-8), y = a h, F = 1 + n / 256, S_k and H_k the 512-point spectra of w s and w y in
 * frame f (bins 0 .. 256), q_k = |S_k|^2 / (|H_k| + 1e-8)^2, t_k = ln(q_k + 1e-8),
 * v_f = sqrt(sum_k t_k^2 / 257), LSD = sum_f v_f / F:
 *   d LSD / d|H_k| = t_k / (257 v_f F) * (-2 q_k / ((|H_k| + 1e-8)(q_k + 1e-8))),  G_k = that * H_k / |H_k|
 *   xbar_t = Re sum_{k=0..256} G_k e^{+2 pi i k t / 512} (the adjoint of the one-sided transform: no factor 2
 *            on the inner bins), times w_t, overlap-added over the frames: ybar
 *   D = sum_t ybar_t h_t,  d LSD / d h_t = a ybar_t + D (s_t - 2 a h_t) / (hh + 1e-8),  grad = g_lsd[b] times that.
 *  - Clean rows are constants: no gradient with respect to ref.
 *  - |H_k| = 0 takes the subgradient 0: a silent estimate frame, or a silent estimate, gives exact zeros.
 *    A frame with v_f = 0 contributes 0.  S = 0, a silent clean frame, gives 0 by the formula.
 *  - A row with a non-finite sample in either operand among its lengths[b] samples (its score is NaN) gets
 *    a gradient row of exact zeros; no other row is touched.
 *  - With lengths, grad[b, lengths[b] .. length) is zero and row b's gradient is that of the unpadded row.
 *    Columns of grad at or past `length` (grad_ld > length) are not written.
 *  - Precision: everything is double up to the one rounding of the float32 store -- the sums, a, the window
 *    products, both transforms, D -- and, unlike the forward's float32 log term, so are the root, the ratio
 *    and the logarithm of each bin: the backward divides by v_f, and on near-identical rows t is of order
 *    1e-6, where a float32 logarithm has lost most of its digits.
 *  - No atomics; every sum has one order that depends on n alone; each overlap-added sample has at most
 *    two addends.  A row's gradient is bitwise the same whatever the batch size, the row's position,
 *    `length`, `ld`, `grad_ld`, the alignment (16-byte or 4-byte loads and stores) and the stream.
 *  - Nothing of the forward call is kept: the entry recomputes sh, hh and a with the forward's own kernels
 *    (bitwise the forward's a), so zero bytes of state outlive fsem_lsd_f32.
 *
 *   ref, deg : as fsem_lsd_f32 takes them ([batch, length] float32, row stride ld, readable up to
 *              ceil4(length) floats per row)
 *   g_lsd    : [batch] float32 device array
 *   state    : [fsem_lsd_grad_state_floats(batch, length)] float32, owned by the caller, 256-byte aligned:
 *              scratch (every part is written by the call that reads it; it may be reused across calls and
 *              need not be kept): the twiddles, per row the scale, the chunk sums, one share of D per 16
 *              frames and the first half-frame of every 16th frame, and ybar in double [ceil4(length)]:
 *              about 8.6 bytes per sample.
 *   grad     : [batch, length] float32, row b at grad + b grad_ld; every element of [b, 0 .. length) is
 *              written.
 * FSEM_EINVAL before any launch for null pointers (lengths may be NULL), batch < 1, length < 1, ld < length,
 * grad_ld < length or length > 2^29 (fsem_lsd_grad_state_floats returns 0 for such batch and length).
 */
int64_t fsem_lsd_grad_state_floats(int64_t batch, int64_t length);  /* 0 for arguments the entry refuses */
int fsem_lsd_grad_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                      const int32_t *lengths, const float *g_lsd, float *state,
                      float *grad, int64_t grad_ld, void *stream);

/* The same gradient for rows at another rate: ref, deg [batch, length] at sample_rate, grad [batch, length]
 * the gradient with respect to deg at that rate, lengths at that rate.  The function differentiated is LSD of
 * the rows resampled to 16 kHz (the taps of fsem_resample_rows_f32, each row as the row alone) WITHOUT the
 * float32 rounding of the resampled rows: the entry resamples both rows itself with the sums in double, keeps
 * them in double in the state, runs the kernels of fsem_lsd_grad_f32 on double rows, and pulls the gradient
 * back through the transposed resampler in double; the float32 store of grad is the only rounding.  Rows
 * resampled from 8 kHz have an upper half-spectrum 100 dB below a frame's peak, where the float32 rounding of
 * a stored 16 kHz row (1e-7 of the peak) is a tenth of a bin: the gradient taken at such stored rows is 0.6 to
 * 1.8 per cent away from this one on the tests' 8 kHz rows.  The scores stay those of fsem_lsd_f32 on the
 * float32 rows the forward resampler stores.  Conventions, promises and refusals as above; in addition
 * FSEM_ERATE for a rate without a resampling kernel and FSEM_EINVAL where the resampled length exceeds 2^29
 * (fsem_lsd_grad_rate_state_floats returns 0 for both); sample_rate == 16000 is fsem_lsd_grad_f32 itself.
 * The state adds both 16 kHz rows in double: about 24.6 bytes per 16 kHz sample. */
int64_t fsem_lsd_grad_rate_state_floats(int64_t batch, int64_t length, int32_t sample_rate);
int fsem_lsd_grad_rate_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                           const int32_t *lengths, int32_t sample_rate, const float *g_lsd, float *state,
                           float *grad, int64_t grad_ld, void *stream);

/* The transpose of fsem_resample_rows_f32 (and of fsem_resample_f32: lengths NULL), for any rate pair
 * those take: g_out [rows, fsem_resample_length(n_in, ...)] (row stride ld_out) is the gradient with
 * respect to the resampled rows, grad_in [rows, n_in] (row stride ld_in) the gradient with respect to the
 * rows that were resampled, each row as the row alone: row r's first lengths[r] inputs collect the terms
 * of its fsem_resample_length(lengths[r], ...) outputs, in ascending output order, with the forward's
 * float32 taps, summed in double and rounded once; grad_in[r, lengths[r] .. n_in) is zero.  One thread
 * per input sample, no atomics.  FSEM_EINVAL for null pointers (lengths may be NULL), rows < 0, n_in < 0,
 * n_in > 2^29, ld_in < n_in or ld_out below the output length; FSEM_ERATE as the forward gives it (a
 * filter above 8192 taps, orig_freq == new_freq); both before any launch. */
int fsem_resample_rows_grad_f32(const float *g_out, int64_t rows, int64_t n_in, int64_t ld_out,
                                const int32_t *lengths /* NULL: whole rows */, float *grad_in, int64_t ld_in,
                                int32_t orig_freq, int32_t new_freq, void *stream);

/* ---------------------------------------------------------------- BSS-eval SDR with gradients
 * The 512-tap BSS-eval SDR of fsem_bsssdr.h as a function to train against: the scores, and the gradient of
 * L = sum_b g_sdr[b] SDR_b with respect to the denoised rows at 16 kHz.  (The forward entries live in
 * libfsem_bsssdr.so, whose entry set is pinned; these joined the core at ABI 11 without a bump, as above.)
 * Notation of fsem_bsssdr.h: s', h' the float32 quotients as doubles, r, b the correlations, x the solution
 * of R x = b, coh = b . x, nh the float32 clamped norm of the estimate.  b is linear in h' and R does not
 * depend on it, so d coh / d h'[u] = 2 y[u] with
 *   y[u] = sum_{k = 0 .. 511} x[k] s'[u - k],  u in [0, n)   (s' = 0 outside [0, n)),
 * a causal 512-tap FIR of the clean row by the solved filter; through the normalisation, h' . y = coh, so
 *   d SDR / d h[u] = D (2 / nh) (y[u] - coh h'[u])      the estimate's norm not clamped
 *   d SDR / d h[u] = D (2 / nh)  y[u]                   its float32 norm < 1e-6: nh is the constant 1e-6
 *   D = (10 / ln 10) / (coh (1 - coh))                  no clamp active
 *   D = (10 / ln 10) / coh                              1 - coh < 1e-8: the denominator is the constant 1e-8
 *   D = 0                                               coh / max(1 - coh, 1e-8) < 1e-8: the score is the constant -80
 * and grad[b, u] = g_sdr[b] times that.
 *  - The float32 quotients are part of the definition: the gradient is taken at them, as the score is; the
 *    float32 rounding of the norm is treated as smooth (d nh / d h = h / nh).  load_diag changes R only.
 *  - Clean rows are constants: no gradient with respect to ref.
 *  - A row whose score is NaN (a singular system, a non-finite sample among its lengths[b] samples) gets a
 *    gradient row of exact zeros, and so does a row with D = 0 (a silent estimate); no other row is touched.
 *  - With lengths, grad[b, lengths[b] .. length) is zero and row b's gradient is that of the unpadded row;
 *    what the memory past lengths[b] holds, NaN included, does not reach the output.  Columns of grad at or
 *    past `length` (grad_ld > length) are not written.
 *  - Precision: double throughout (the FIR on the vector FMA pipe, by the forward's own inner loop) up to the
 *    one rounding of the float32 store: y - coh h' cancels to the order of 1 - coh.
 *  - No atomics; every output has one owner and one order of its 512 terms.  A row's gradient is bitwise the
 *    same whatever the batch size, the row's position, `length`, `ld`, `grad_ld`, the alignment and the stream.
 *
 *   ref, deg : as fsem_bsssdr_f32 takes them ([batch, length] float32, row stride ld; no sample at or past
 *              lengths[b] is read by the backward)
 *   state    : [fsem_bsssdr_state_floats(batch, length)] float32, owned by the caller, 256-byte aligned.  Its
 *              head is the workspace of fsem_bsssdr_load_diag_f32, laid out as that entry lays it out; its
 *              tail is one record per row: x [512] float64, coh, and the row's flags (a NaN score; the
 *              estimate's float32 norm below 1e-6, by the forward's own comparison): 4112 bytes per row.
 *   fsem_bsssdr_state_f32 : sdr [batch] bitwise that of fsem_bsssdr_load_diag_f32 (the same kernels on the
 *              state's head); leaves the norms and the records in the state.
 *   fsem_bsssdr_grad_f32  : reads the state fsem_bsssdr_state_f32 left for the same ref, deg, batch, length,
 *              ld and lengths (it writes nothing there and may be called again) and writes every element of
 *              grad[b, 0 .. length) (row b at grad + b grad_ld), rounded to float32 once from double.
 *   g_sdr    : [batch] float32 device array.
 * FSEM_EINVAL before any launch for null pointers (lengths may be NULL), batch < 0, length < 1,
 * length > 2^29, ld < length, grad_ld < length or a load_diag that is not finite (fsem_bsssdr_state_floats
 * returns 0 for such batch and length).  batch == 0 is FSEM_OK with nothing launched.
 */
int64_t fsem_bsssdr_state_floats(int64_t batch, int64_t length);  /* 0 for arguments the entries refuse */
int fsem_bsssdr_state_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                          const int32_t *lengths, double load_diag, float *sdr, float *state, void *stream);
int fsem_bsssdr_grad_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                         const int32_t *lengths, const float *g_sdr, const float *state,
                         float *grad, int64_t grad_ld, void *stream);

/* ---------------------------------------------------------------- DNSMOS with gradients
 * The SIG, BAK and OVRL of fsem_dnsmos.h as functions to train against: the gradient of
 * L = sum_b sum_k g_scores[b][k] score_k(b) with respect to the 16 kHz rows.  (The forward entries live in
 * libfsem_dnsmos.so, whose entry set is pinned; these joined the core at ABI 11 without a bump, as above.)
 * It is the gradient of the forward the scores come from, f16 roundings included: every ReLU, pool and
 * maximum decision is the one the f16 forward took.  Notation of fsem_dnsmos.h.
 *
 * Nothing is kept between the forward call and this one.  The entry recomputes each pass of `pass`
 * segments (1 ... 16, the caller's choice) with the forward's own kernels, recording in the pass's scratch
 * re and im of the front end (float32), which of its 2 x 2 inputs each pooled element is, and where conv7's
 * maxima lie; then the adjoint of the pass runs; pass after pass on the stream.  Per segment:
 *  - Seed: g_scores[b][k] (c1_k + 2 c2_k r_k) / S_b at raw output k, in double, rounded to float32.
 *  - Dense layers transposed, float32; a ReLU passes the gradient where its output is > 0.  The maximum
 *    over positions passes a channel's gradient to the first position (row-major) that attains the
 *    maximum, and nothing when the maximum is 0.
 *  - Scale: the 64 values at conv7's output are multiplied by the power of two that puts the largest
 *    magnitude into [8, 16), so that the f16 gradients below stay clear of f16's subnormal range whatever
 *    the seed's size; the inverse is multiplied back exactly where the image gradient is formed.  A
 *    segment whose 64 values are all zero (a zero seed) or not all finite is skipped: it adds nothing.
 *  - Data gradients of conv7 ... conv2 on v_mfma_f32_16x16x32_f16: the forward's implicit GEMM with C_in
 *    and C_out exchanged, weights rounded to f16 from the same float32 tensors, ordered
 *    [2 - ky, 2 - kx][C_in][C_out]; float32 accumulation; the gradient of each layer's input is stored as
 *    f16.  A pooled layer passes the gradient of a pooled element to its winner (the first of the 2 x 2
 *    in row-major order that attains the maximum, taken on the float32 values) where the pooled f16
 *    activation is > 0; the row and column that pooling's floor dropped get 0.  conv2 and conv3 pass the
 *    gradient where the stored f16 activation is > 0.
 *  - conv2's data gradient (128 channels) is not stored: conv1's pre-activation is recomputed from the
 *    image (the forward's nine FMAs) for the mask z > 0, and the pixel's 128 channels are contracted with
 *    conv1's float32 weights into the image gradient [900][161], float32.
 *  - Front end in double: g_p = g_img / (p ln 10) where the float32 power p > 1e-12, else 0;
 *    g_re = 2 re g_p, g_im = 2 im g_p; a frame sample is the sum over the bins in ascending order (re's
 *    term, then im's); the two frames that cover a segment sample are added, the earlier first.
 *  - Rows: segment s, sample t belongs to row sample (16000 s + t) mod n; a sample of a short row collects
 *    every wrap, in ascending t, in double; the segments are added in ascending order onto the float32
 *    gradient, one rounding per segment.
 * A row flagged non-finite by the forward's rule (its scores are NaN), a row of no samples and a row whose
 * g_scores are zero get a gradient row of exact zeros; no other row is touched by them.  grad[b, n_b ..
 * length) is zero; samples at or past n_b are never read; columns of grad at or past `length` are not written.
 * No float atomics; every sum has one order.  A row's gradient is bitwise the same whatever `pass`, the
 * batch size, the row's position, `length`, `ld`, `ld_grad`, the alignment and the stream.
 *
 *   weights  : the blob of fsem_dnsmos_grad_pack_weights_f32 (fsem_dnsmos_grad_weights_floats() floats,
 *              256-byte aligned): the forward's blob, the two STFT matrices in the checkpoint's layout and
 *              the flipped f16 convolution weights, from the same 22 tensors (a HOST array of 22 device
 *              pointers in state-dict order, as fsem_dnsmos_pack_weights_f32 takes them).
 *   scratch  : [fsem_dnsmos_grad_scratch_floats(batch, length, pass)] float32, 256-byte aligned, owned by
 *              the caller; about 92 MB per segment of a pass and 4 bytes per row.
 *   g_scores : [batch][3] float32 device array.
 *   grad     : [batch, length] float32 (row stride ld_grad), every element of [b, 0 .. length) written.
 *   raw      : NULL or [S_total][3]: the raw outputs the entry recomputed, bitwise fsem_dnsmos_raw_f32's.
 *   fsem_dnsmos_grad_image_f32 : the stage entry, the counterpart of fsem_dnsmos_features_f32: g_image
 *              [S_total][900][161] float32, the gradient with respect to each segment's log-power image
 *              (zeros for a skipped segment), and nothing after it.
 * FSEM_EINVAL before any launch for null pointers (lengths and raw may be NULL), batch < 1, length < 1,
 * ld < length, ld_grad < length, length > 2^29 or pass outside 1 ... 16 (the scratch query returns 0 for
 * those); FSEM_EWORKSPACE from the pack entry for a blob that is too small.
 */
int64_t fsem_dnsmos_grad_scratch_floats(int64_t batch, int64_t length, int64_t pass);
int64_t fsem_dnsmos_grad_weights_floats(void);
int fsem_dnsmos_grad_pack_weights_f32(const float *const *tensors, float *blob, int64_t blob_floats, void *stream);
int fsem_dnsmos_grad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                         const float *weights, const float *g_scores, float *grad, int64_t ld_grad,
                         float *raw /* or NULL */, float *scratch, int64_t pass, void *stream);
int fsem_dnsmos_grad_image_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                               const float *weights, const float *g_scores, float *g_image, float *scratch,
                               int64_t pass, void *stream);

/* ---------------------------------------------------------------- SRMR with gradients
 * SRMR ("SRMR" above, its notation) as a function to train against: the gradient of L = sum_b gout[b] SRMR_b
 * with respect to the rows.  (Joined the core at ABI 11 without a bump, as above.  The entries are named
 * fsem_srmrgrad_*: the set of names that begin with fsem_srmr_ is the forward's and is pinned.)  K* is a decision and is
 * taken as a constant.  Per row, with G = gout[b], N and D the ratio's numerator and denominator, per channel
 * i with pole p and gain g (v, the four stages s_j with y = s_4, e = |y|, m_k as in the forward):
 *  1. c_k = G / D for k < 4; -G N / D^2 for 4 <= k < K*; 0 for k >= K*.  The same c_k for every channel.
 *  2. q_ik[t] = (2 c_k / F) m_ik[t] V[t] for t < nend = (F - 1) wi + wl, and 0 from nend on.
 *  3. The adjoint biquad runs backwards in time: r_ik[t] = q_ik[t] - a1_k r_ik[t + 1] - a2_k r_ik[t + 2], r = 0
 *     from nend on; de_i[t] = sum_k b0_k (r_ik[t] - r_ik[t + 2]).
 *  4. a0_i[t] = de_i[t] y_i[t] / |y_i[t]|, exactly 0 where |y_i[t]| = 0 (the subgradient 0).
 *  5. Four adjoint stages backwards in time with the conjugate pole: a^j[t] = conj(p) a^j[t + 1] + a^(j-1)[t].
 *  6. dx[t] = sum_i Re(conj(p) a4_i[t + 1] + 4 conj(p)^2 a4_i[t + 2] + conj(p)^3 a4_i[t + 3]) / g_i.
 * dx[t] is exactly 0 for t >= nend - 1.  SRMR does not depend on the row's scale: sum_t dx[t] x[t] = 0 up to
 * rounding, and the gradient scales with 1 / gain.
 *
 * Row conventions.  A row with F = 0, a row with a non-finite sample among its first n, a row whose score is
 * not finite (a digitally silent row) and a row whose gout is 0 get a gradient row of exact zeros; no other row
 * is touched by them.  grad[b, t] is written as zero for t >= nend - 1 and for t >= n_b; samples at or past
 * n_b are never read; columns of grad at or past `length` are not written.
 *
 * Precision and order.  Nothing of the forward is kept but `energies`.  The entry walks a row's 4096-sample
 * tiles twice per channel: first to last, storing the filter state that enters each tile (184 bytes per row,
 * channel and tile); then last to first, recomputing the tile's y and envelope from that state with the
 * forward's own code and running steps 2 - 6 on it, with the adjoint states carried to the tile before.  The
 * modulation recurrences, their adjoints and de are double; the gammatone, y / |y| and the adjoint stages are
 * float32 complex, with the forward's constants.  The sum over k is ((0 + 1) + (2 + 3) + (4 + 5)) + (6 + 7);
 * each channel's dx goes to a float32 plane in scratch and the 23 planes are added in channel order in double,
 * rounded once.  Rows are processed in passes of fsem_srmrgrad_pass_rows(length) rows (at most 2 GiB of planes
 * and checkpoints).  No float atomics; a row's gradient is bitwise the same whatever the pass it falls in, the
 * batch size, the row's position, `length`, `ld` and the stream.
 *   deg, lengths, sample_rate : as fsem_srmr_f32 took them
 *   energies : [batch][23][8] float64, as fsem_srmr_f32 wrote them for these rows
 *   gout     : [batch] float32 device array, the incoming gradients
 *   scratch  : fsem_srmrgrad_scratch_bytes(batch, length) bytes, 256-byte aligned, owned by the caller
 *   grad     : [batch, length] float32 with the rows' own stride ld; every element of [b, 0 .. length) written
 * FSEM_EINVAL before any launch for null pointers (lengths may be NULL), batch < 1, length < 1, ld < length or
 * length > 2^29 (the queries return 0 for those); FSEM_ERATE for another sample rate.
 */
int64_t fsem_srmrgrad_pass_rows(int64_t length);                    /* rows per pass, from length alone */
int64_t fsem_srmrgrad_scratch_bytes(int64_t batch, int64_t length); /* 0 for arguments the entry refuses */
int fsem_srmrgrad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                      int32_t sample_rate, const double *energies, const float *gout, void *scratch, float *grad,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FSEM_H */
