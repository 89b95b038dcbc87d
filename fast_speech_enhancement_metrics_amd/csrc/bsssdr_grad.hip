// BSS-eval SDR with gradients (include/fsem.h, "BSS-eval SDR with gradients"): the scores of
// fsem_bsssdr_load_diag_f32 with a record per row, and the closed-form gradient with respect to the
// denoised rows.  In libfsem.so: libfsem_bsssdr.so's entry set is pinned, and these entries take no
// workspace.  The forward's kernels, workspace layout and launch sequence are fsem_bsssdr_kernels.h's
// (this library compiles its own copy); here sdr_solve leaves x, coh and the row's flags in the state.
//
//   sdr_grad_fir   grid (tile of UB = 4096 outputs, row), 4 waves.  With x the solution of R x = b,
//                  y[u] = sum_{k < 512} x[k] s'[u - k] (s' = 0 outside [0, n)) and
//                    grad[u] = g D (2 / nh) (y[u] - coh h'[u])      (D: the score's slope in coh)
//                  for u < n, zeros for n <= u < length.  The inner loop is fsem_corr512.h's
//                  corr_quarter, the forward's: the taps reversed (xr[k'] = x[511 - k']) are its
//                  broadcast signal, and a window of s' that starts at u0 - 511 turns its "lag
//                  8 lane + j" into "output u0 + 8 lane + j".  One wave makes 512 outputs per pass
//                  over the taps; its two accumulators serve two such output tiles, so a block makes
//                  8 x 512 outputs from s'[U0 - 511 .. U0 + 4096) in LDS (4608 doubles, groups of 8
//                  stored 80 bytes apart as in the forward) and the 512 reversed taps: 51200 bytes, the
//                  forward's 3 blocks per CU.  All in double on the vector FMA pipe; y - coh h' cancels
//                  to 1 - coh, which reaches 1e-4 and below on good estimates.  One rounding, at the
//                  float32 store.  No atomics: every output has one owner and one order of its 512 terms.
#include "fsem_bsssdr_kernels.h"

namespace fsem {
namespace bsssdr {

constexpr int TILES = 2 * NWAVE;             // output tiles of a block: two per wave
constexpr int UB = TILES * K;                // outputs of a block
constexpr int NGS = (UB + K) / G;            // groups of the block's extent of s'
constexpr int NGX = K / G;                   // groups of the reversed taps
static_assert((NGS + NGX) * GP * sizeof(double) == 51200, "the forward's LDS: 3 blocks per CU");
static_assert((TILES - 1) * (K / G) + (QT / G - 1) + 63 + 1 < NGS, "the last tile's last window group lies in LDS");

__global__ __launch_bounds__(T) void sdr_grad_fir(const float *__restrict__ ref, const float *__restrict__ deg,
                                                  int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                  int64_t r0, const float2 *__restrict__ nrm,
                                                  const Rec *__restrict__ rec, const float *__restrict__ g_sdr,
                                                  float *__restrict__ grad, int64_t grad_ld) {
  __shared__ __attribute__((aligned(16))) double lds[(NGS + NGX) * GP];
  double *__restrict__ S = lds;
  double *__restrict__ XR = lds + NGS * GP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = r0 + blockIdx.y;
  const int n = row_length(lengths, row, length);
  const int U0 = blockIdx.x * UB;  // < length <= 2^29
  const Rec *__restrict__ rc = rec + row;
  float *__restrict__ grow = grad + row * grad_ld;
  const int32_t flags = rc->flags;
  const double coh = rc->coh;
  // the score's slope in coh, by the clamps of the forward: 10 log10(max(coh / max(1 - coh, 1e-8), 1e-8))
  double D = 0.0;
  if (!(flags & kRowBad)) {
    const double den = 1.0 - coh;
    const double ratio = coh / (den < 1e-8 ? 1e-8 : den);
    constexpr double k10 = 4.342944819032518;  // 10 / ln 10
    if (!(ratio < 1e-8)) D = den < 1e-8 ? k10 / coh : k10 / (coh * den);
  }
  if (D == 0.0 || U0 >= n) {  // (block-uniform) a NaN row, a score at its floor, or the row's padding: zeros
    for (int i = tid; i < UB && U0 + i < length; i += T) grow[U0 + i] = 0.f;
    return;
  }
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  const float2 nm = nrm[row];
  for (int i = tid; i < UB + K; i += T) {
    const int t = U0 - (K - 1) + i;
    const bool in = t >= 0 && t < n;
    // the float32 quotient, as sdr_corr forms it
    const float sq = in ? srow[t] / nm.x : 0.f;
    S[gpad(i)] = (double)sq;
  }
  for (int i = tid; i < K; i += T) XR[gpad(i)] = rc->x[K - 1 - i];
  __syncthreads();
  double acc0[G], acc1[G];
#pragma unroll
  for (int j = 0; j < G; ++j) acc0[j] = acc1[j] = 0.0;
  const int t0 = 2 * wave, u0 = U0 + t0 * K;  // this wave's tiles t0, t0 + 1: outputs from u0 and from u0 + 512
  if (u0 < n)  // (wave-uniform; the second tile may lie past n: its sums are not stored)
    corr_quarter(XR, S + t0 * (K / G) * GP, S + (t0 + 1) * (K / G) * GP, 0, lane, 0, K, acc0, acc1);
  // with the norm at its clamp nh is the constant 1e-6 and h' has no term through it
  const double c = (flags & kRowClamped) ? 0.0 : coh;
  const double scale = (double)g_sdr[row] * D * (2.0 / (double)nm.y);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int u = u0 + half * K + G * lane + j;
      if (u < n) {
        const float hq = hrow[u] / nm.y;
        grow[u] = (float)(scale * fma(-c, (double)hq, half ? acc1[j] : acc0[j]));
      } else if (u < length) {
        grow[u] = 0.f;
      }
    }
  }
}

// The state: the forward's workspace (its head), then one record per row.
struct GradWs {
  Ws w;
  Rec *rec;
};
inline GradWs grad_layout(Arena &a, int64_t batch, int64_t length) {
  GradWs g;
  g.w = layout(a, batch, length);
  g.rec = a.take<Rec>((size_t)batch);
  return g;
}

}  // namespace bsssdr
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_bsssdr_state_floats(int64_t batch, int64_t length) {
  if (batch < 0 || length < 1 || length > kMaxLength) return 0;
  return (int64_t)(layout_bytes(bsssdr::grad_layout, batch, length) / sizeof(float));
}

extern "C" int fsem_bsssdr_state_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                     const int32_t *lengths, double load_diag, float *sdr, float *state,
                                     void *stream) {
  if (!ref || !deg || !sdr || !state || batch < 0 || length < 1 || ld < length || length > kMaxLength ||
      !isfinite(load_diag))
    return FSEM_EINVAL;
  if (batch == 0) return FSEM_OK;
  Arena a(state);
  const bsssdr::GradWs g = bsssdr::grad_layout(a, batch, length);
  return bsssdr::launch_scores(ref, deg, batch, length, ld, lengths, load_diag, sdr, g.w, g.rec, (hipStream_t)stream);
}

extern "C" int fsem_bsssdr_grad_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                    const int32_t *lengths, const float *g_sdr, const float *state, float *grad,
                                    int64_t grad_ld, void *stream) {
  if (!ref || !deg || !g_sdr || !state || !grad || batch < 0 || length < 1 || ld < length || grad_ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  if (batch == 0) return FSEM_OK;
  Arena a(const_cast<float *>(state));
  const bsssdr::GradWs g = bsssdr::grad_layout(a, batch, length);
  hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((length + bsssdr::UB - 1) / bsssdr::UB);
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    hipLaunchKernelGGL(bsssdr::sdr_grad_fir, grid_slice(tiles, batch, r0), dim3(bsssdr::T), 0, st, ref, deg, ld,
                       lengths, (int)length, r0, g.w.nrm, g.rec, g_sdr, grad, grad_ld);
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}
