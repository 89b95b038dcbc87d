// DNSMOS (SIG, BAK, OVRL) of 16 kHz rows (include/fsem_dnsmos.h), the reference's fast_se_metrics.DNSMOS:
// the entries of libfsem_dnsmos.so.  The kernels, the layouts and the launch sequence of a pass are
// fsem_dnsmos_kernels.h's (described there), shared with the backward in libfsem.so (dnsmos_grad.hip).
#include "fsem_build_marker.h"
#include "fsem_dnsmos_kernels.h"

namespace fsem {
namespace dnsmos {

inline int pass_size(size_t ws_bytes) {
  for (int P = MAXP; P >= 1; --P)
    if (layout_bytes(layout, P) <= ws_bytes) return P;
  return 0;
}

// The three entries: scores (sig_bak_ovr), the image (features) or the raw outputs (raw).
inline int run(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
               const void *weights, float *scores, float *features, float *raw, void *ws, size_t ws_bytes,
               void *stream) {
  if (!deg || !weights || !(scores || features || raw) || batch < 1 || length < 1 || ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  const int P = ws ? pass_size(ws_bytes) : 0;
  if (P < 1) return FSEM_EWORKSPACE;
  Arena a(ws);
  const Ws w = layout(a, P);
  Arena ba(const_cast<void *>(weights));
  const Blob b = blob_layout(ba);
  hipStream_t st = (hipStream_t)stream;
  if (scores) {
    const int64_t n = batch * 3;
    hipLaunchKernelGGL(fill_nan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scores, n);
    FSEM_CHECK_LAUNCH();
  }
  // with `lengths` the rows' counts are on the device: the passes cover the largest possible total,
  // and the blocks of a pass past the last segment return at once
  const int64_t total = batch * max_segs(length, lengths != nullptr);
  int parity = 0;
  for (int64_t g0 = 0; g0 < total; g0 += P, parity ^= 1) {
    float *img = features ? features + (size_t)g0 * NF * NB : w.img;
    const int rc = forward_pass<false>(st, deg, batch, length, ld, lengths, b, w, P, g0, img, features != nullptr, raw,
                                       Rec{});
    if (rc != FSEM_OK) return rc;
    if (features) continue;
    if (scores) {
      hipLaunchKernelGGL(dn_finish, dim3(1), dim3(64), 0, st, w.map, w.poly, w.segflag, w.carry, P, parity, scores);
      FSEM_CHECK_LAUNCH();
    }
  }
  return FSEM_OK;
}

}  // namespace dnsmos
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_dnsmos_segments(int64_t length) { return dnsmos::segs_of(length); }

extern "C" size_t fsem_dnsmos_weights_bytes(void) { return layout_bytes(dnsmos::blob_layout); }

extern "C" int fsem_dnsmos_pack_weights_f32(const float *const *t, void *blob, size_t blob_bytes, void *stream) {
  if (!t || !blob) return FSEM_EINVAL;
  for (int i = 0; i < FSEM_DNSMOS_NUM_TENSORS; ++i)
    if (!t[i]) return FSEM_EINVAL;
  Arena a(blob);
  const dnsmos::Blob b = dnsmos::blob_layout(a);
  if (!a.fits(blob_bytes)) return FSEM_EWORKSPACE;
  return dnsmos::pack_blob(t, b, (hipStream_t)stream);
}

extern "C" size_t fsem_dnsmos_min_workspace_bytes(void) { return layout_bytes(dnsmos::layout, 1); }

extern "C" size_t fsem_dnsmos_workspace_bytes(int64_t batch, int64_t length) {
  if (batch < 1 || length < 1 || length > kMaxLength) return 0;
  const int64_t most = batch * dnsmos::max_segs(length, true);
  return layout_bytes(dnsmos::layout, (int)(most < dnsmos::MAXP ? most : dnsmos::MAXP));
}

extern "C" int fsem_dnsmos_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                               const void *weights, float *sig_bak_ovr, void *ws, size_t ws_bytes, void *stream) {
  if (!sig_bak_ovr) return FSEM_EINVAL;
  return dnsmos::run(deg, batch, length, ld, lengths, weights, sig_bak_ovr, nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int fsem_dnsmos_features_f32(const float *deg, int64_t batch, int64_t length, int64_t ld,
                                        const int32_t *lengths, const void *weights, float *features, void *ws,
                                        size_t ws_bytes, void *stream) {
  if (!features) return FSEM_EINVAL;
  return dnsmos::run(deg, batch, length, ld, lengths, weights, nullptr, features, nullptr, ws, ws_bytes, stream);
}

extern "C" int fsem_dnsmos_raw_f32(const float *deg, int64_t batch, int64_t length, int64_t ld,
                                   const int32_t *lengths, const void *weights, float *raw, void *ws, size_t ws_bytes,
                                   void *stream) {
  if (!raw) return FSEM_EINVAL;
  return dnsmos::run(deg, batch, length, ld, lengths, weights, nullptr, nullptr, raw, ws, ws_bytes, stream);
}
