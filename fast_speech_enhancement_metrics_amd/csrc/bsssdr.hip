// BSS-eval SDR with a 512-tap distortion filter of (clean, denoised) rows (include/fsem_bsssdr.h),
// the reference's fast_se_metrics.SDR (SDR.py:7-97): the entries of libfsem_bsssdr.so.  The kernels
// (sdr_norm_partial, sdr_norms, sdr_corr, sdr_solve), the workspace layout and the launch sequence
// are fsem_bsssdr_kernels.h's, shared with bsssdr_grad.hip (libfsem.so), which runs them with the
// records its backward reads; here sdr_solve gets no record and writes the scores alone.
#include "../../include/fsem_bsssdr.h"
#include "fsem_build_marker.h"
#include "fsem_bsssdr_kernels.h"

using namespace fsem;

extern "C" int64_t fsem_bsssdr_filter_length(void) { return bsssdr::K; }

extern "C" int64_t fsem_bsssdr_chunk(void) { return bsssdr::C; }

extern "C" int64_t fsem_bsssdr_norm_chunk(void) { return bsssdr::NC; }

extern "C" size_t fsem_bsssdr_workspace_bytes(int64_t batch, int64_t length) {
  if (batch < 1 || length < 1 || length > kMaxLength) return 0;
  return layout_bytes(bsssdr::layout, batch, length);
}

extern "C" int fsem_bsssdr_load_diag_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                         const int32_t *lengths, double load_diag, float *sdr, void *ws,
                                         size_t ws_bytes, void *stream) {
  if (!ref || !deg || !sdr || batch < 1 || length < 1 || ld < length || length > kMaxLength || !isfinite(load_diag))
    return FSEM_EINVAL;
  Arena a(ws);
  const bsssdr::Ws w = bsssdr::layout(a, batch, length);
  if (!a.fits(ws_bytes)) return FSEM_EWORKSPACE;
  return bsssdr::launch_scores(ref, deg, batch, length, ld, lengths, load_diag, sdr, w, nullptr, (hipStream_t)stream);
}

extern "C" int fsem_bsssdr_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                               const int32_t *lengths, float *sdr, void *ws, size_t ws_bytes, void *stream) {
  return fsem_bsssdr_load_diag_f32(ref, deg, batch, length, ld, lengths, 0.0, sdr, ws, ws_bytes, stream);
}
