// Multi-source SI-SDR and SNR with the assignment and the gradient with respect to the estimates
// (include/fsem.h, "PITSDR").  Replaces nothing in the reference.  One read of each input forward,
// one read of each input and one write of the gradient backward.
//
//   pit_partial<S, E>  grid (chunk, mixture); a chunk is C = 8192 samples.  A block reads the chunk of
//                      the mixture's S + E rows once: thread t takes the float4s t, t + 256, ... of the
//                      chunk from every row (one 16-byte load each where the rows are aligned and the
//                      float4 lies inside the mixture's n samples, 4-byte loads otherwise: the same
//                      samples to the same thread either way) and adds, in double, the products of the
//                      float32 samples (exact in double): ss[S], hh[E], s1[S], h1[E], sh[S E], dd[S E].
//                      The 2 S + 2 E + 2 S E sums stay in registers (templated on S and E), are added
//                      over the wave by wave_sums_d and over the four waves as ((w0 + w1) + w2) + w3.
//                      One record per (mixture, chunk); no atomics.
//   pit_finish         one thread per mixture: the chunk records in ascending order into the totals at
//                      the head of the mixture's block (left there for the backward), sdr.hip's
//                      sdr_finish rules per pair, both matrices, the <= 24 assignments.
//   pit_grad<S>        grid (chunk, mixture).  The first S E threads form the pairs' coefficients from
//                      the totals in double, E threads add them over the sources in ascending order and
//                      round A, C and K to float32 (LDS); then the block streams the chunk: the S source
//                      float4s once, each estimate float4 once, S + 1 float32 FMAs per sample, one
//                      store.  Every element of the row capacity is written (zeros from n on).
//
// Every sum has one order, fixed by n alone: a mixture's outputs do not depend on the batch size,
// the mixture's position, the row capacity, the loads' width or the stream.
#include <math.h>

#include "fsem_sdr_rules.h"

namespace fsem {
namespace pitsdr {

constexpr int MAXS = 4;   // sources (and estimates) per mixture, at most
constexpr int T = 256;    // threads of a chunk block
constexpr int C = 8192;   // samples per chunk: 8 float4s per thread and row
constexpr int FT = 64;    // threads of a finish block

// A record (and the totals): ss[S], hh[E], s1[S], h1[E], sh[S E], dd[S E]; pair (i, e) at i E + e.
__host__ __device__ constexpr int fields(int S, int E) { return 2 * S + 2 * E + 2 * S * E; }
struct Off {
  int ss, hh, s1, h1, sh, dd;
};
__host__ __device__ constexpr Off offsets(int S, int E) {
  return Off{0, S, S + E, 2 * S + E, 2 * S + 2 * E, 2 * S + 2 * E + S * E};
}

inline bool rate_ok(int32_t sr) { return sr >= 4000 && sr <= 192000; }
inline int64_t chunks(int64_t length) { return (length + C - 1) / C; }
inline int64_t sums_doubles(int S, int E, int64_t length) { return (int64_t)fields(S, E) * (1 + chunks(length)); }

template <int S, int E, bool VEC>
__global__ __launch_bounds__(T) void pit_partial(const float *__restrict__ src, const float *__restrict__ est,
                                                 int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                 int64_t b0, double *__restrict__ sums, int64_t stride) {
  constexpr int NT = fields(S, E);
  constexpr Off o = offsets(S, E);
  __shared__ double red[4][NT];
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int c = blockIdx.x;
  const int n = row_length(lengths, b, length);
  const int base = c * C;  // < length + C <= 2^29 + 2^13
  if (base >= n) return;   // (the finish pass reads ceil(n / C) records of this mixture)
  const int hi = min(base + C, n);
  const float *__restrict__ srow = src + b * S * ld;
  const float *__restrict__ hrow = est + b * E * ld;
  double acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = 0.0;
  for (int a = base + 4 * tid; a < hi; a += 4 * T) {
    float sv[S][4], hv[E][4];
#pragma unroll
    for (int i = 0; i < S; ++i) load4<VEC>(srow + i * ld, a, hi, sv[i]);
#pragma unroll
    for (int e = 0; e < E; ++e) load4<VEC>(hrow + e * ld, a, hi, hv[e]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double sd[S], hd[E];
#pragma unroll
      for (int i = 0; i < S; ++i) {
        sd[i] = sv[i][j];
        acc[o.ss + i] = fma(sd[i], sd[i], acc[o.ss + i]);
        acc[o.s1 + i] += sd[i];
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        hd[e] = hv[e][j];
        acc[o.hh + e] = fma(hd[e], hd[e], acc[o.hh + e]);
        acc[o.h1 + e] += hd[e];
      }
#pragma unroll
      for (int i = 0; i < S; ++i) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double d = hd[e] - sd[i];
          acc[o.sh + i * E + e] = fma(sd[i], hd[e], acc[o.sh + i * E + e]);
          acc[o.dd + i * E + e] = fma(d, d, acc[o.dd + i * E + e]);
        }
      }
    }
  }
  wave_sums_d<NT>(acc);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NT; ++k) red[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < NT) sums[b * stride + NT * (1 + c) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// A mixture without a sample, or with a non-finite one (it reaches a sum of squares): NaN everywhere.
__device__ __forceinline__ bool mixture_bad(const double *__restrict__ tot, int S, int E, int n) {
  const Off o = offsets(S, E);
  bool bad = n == 0;
  for (int i = 0; i < S; ++i) bad = bad || !isfinite(tot[o.ss + i]);
  for (int e = 0; e < E; ++e) bad = bad || !isfinite(tot[o.hh + e]);
  for (int k = 0; k < S * E; ++k) bad = bad || !isfinite(tot[o.sh + k]) || !isfinite(tot[o.dd + k]);
  return bad;
}

__global__ __launch_bounds__(FT) void pit_finish(double *__restrict__ sums, int64_t stride,
                                                 const int32_t *__restrict__ lengths, int length, int64_t B, int S,
                                                 int E, int zero_mean, int criterion, float *__restrict__ si_mat,
                                                 float *__restrict__ snr_mat, int32_t *__restrict__ perm) {
  const int64_t b = (int64_t)blockIdx.x * FT + threadIdx.x;
  if (b >= B) return;
  const int n = row_length(lengths, b, length);
  const int NT = fields(S, E);
  const Off o = offsets(S, E);
  double *__restrict__ tot = sums + b * stride;
  const int nc = (n + C - 1) / C;
  for (int k = 0; k < NT; ++k) {
    double v = 0.0;
    for (int c = 0; c < nc; ++c) v += tot[NT * (1 + c) + k];
    tot[k] = v;
  }
  const bool bad = mixture_bad(tot, S, E, n);
  double si[MAXS][MAXS], sn[MAXS][MAXS];
  bool nan = bad;
  for (int i = 0; i < S; ++i) {
    for (int e = 0; e < E; ++e) {
      const int k = i * E + e;
      const PairScores p = pair_scores(tot[o.ss + i], tot[o.hh + e], tot[o.sh + k], tot[o.dd + k], tot[o.s1 + i],
                                 tot[o.h1 + e], n, zero_mean);
      si[i][e] = p.si;
      sn[i][e] = p.snr;
      nan = nan || (criterion == 1 ? p.si != p.si : p.snr != p.snr);
    }
  }
  int p[MAXS] = {0, 1, 2, 3};
  if (criterion != 0 && S == E && !nan) {
    // the assignments in lexicographic order (itertools.permutations'); the first of equal means stays
    int total = 1;
    for (int e = 0; e < S; ++e) total *= S;
    double best = 0;
    bool have = false;
    for (int code = 0; code < total; ++code) {
      int cand[MAXS], used = 0, rest = code;
      for (int e = S - 1; e >= 0; --e) {
        cand[e] = rest % S;
        rest /= S;
      }
      bool isperm = true;
      for (int e = 0; e < S; ++e) {
        isperm = isperm && !(used >> cand[e] & 1);
        used |= 1 << cand[e];
      }
      if (!isperm) continue;
      double m = 0;
      for (int e = 0; e < S; ++e) m += criterion == 1 ? si[cand[e]][e] : sn[cand[e]][e];
      m /= S;
      if (!have || m > best) {
        have = true;
        best = m;
        for (int e = 0; e < S; ++e) p[e] = cand[e];
      }
    }
  }
  const float fnan = __builtin_nanf("");
  for (int e = 0; e < E; ++e) {
    perm[b * E + e] = p[e];
    for (int i = 0; i < S; ++i) {
      si_mat[(b * S + i) * E + e] = bad ? fnan : (float)si[i][e];
      snr_mat[(b * S + i) * E + e] = bad ? fnan : (float)sn[i][e];
    }
  }
}

template <int S, bool VEC>
__global__ __launch_bounds__(T) void pit_grad(const float *__restrict__ src, const float *__restrict__ est, int64_t ld,
                                              const int32_t *__restrict__ lengths, int length, int64_t b0, int E,
                                              int zero_mean, const double *__restrict__ sums, int64_t stride,
                                              const float *__restrict__ g_si, const float *__restrict__ g_snr,
                                              float *__restrict__ grad, int64_t grad_ld) {
  __shared__ double pa_si[MAXS * MAXS], pa_snr[MAXS * MAXS], pc_si[MAXS * MAXS], pc_snr[MAXS * MAXS];
  __shared__ float cA[MAXS * MAXS], cC[MAXS], cK[MAXS];
  __shared__ int live;
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int n = row_length(lengths, b, length);
  const double *__restrict__ tot = sums + b * stride;
  const Off o = offsets(S, E);
  if (tid < S * E) {
    const int i = tid / E, e = tid % E;
    const double kk = 20.0 / 2.302585092994045684;  // 20 / ln 10
    double a_si = 0, a_snr = 0, c_si = 0, c_snr = 0;
    const bool bad = mixture_bad(tot, S, E, n);
    if (!bad) {
      const double dd = tot[o.dd + tid];
      const PairScores p = pair_scores(tot[o.ss + i], tot[o.hh + e], tot[o.sh + tid], dd, tot[o.s1 + i], tot[o.h1 + e], n,
                                 zero_mean);
      const int64_t at = (b * S + i) * E + e;
      if (isfinite(p.si)) {  // (then ss, sh and nn are all non-zero)
        const double g = kk * (double)g_si[at];
        a_si = g * (1.0 / p.sh + p.sh / (p.ss * p.nn));
        c_si = -g / p.nn;
      }
      if (isfinite(p.snr)) {
        const double g = kk * (double)g_snr[at];
        a_snr = g / dd;
        c_snr = -g / dd;
      }
    }
    pa_si[tid] = a_si, pa_snr[tid] = a_snr, pc_si[tid] = c_si, pc_snr[tid] = c_snr;
    cA[tid] = (float)(a_si + a_snr);
    if (tid == 0) live = !bad;
  }
  __syncthreads();
  if (tid < E) {
    double cc = 0, kc = 0, ka = 0;
    for (int i = 0; i < S; ++i) {
      cc += pc_si[i * E + tid] + pc_snr[i * E + tid];
      kc += pc_si[i * E + tid];
      ka += pa_si[i * E + tid] * (tot[o.s1 + i] / n);
    }
    cC[tid] = (float)cc;
    cK[tid] = zero_mean && live ? (float)(-ka - kc * (tot[o.h1 + tid] / n)) : 0.f;
  }
  __syncthreads();
  const int nl = live ? n : 0;  // samples with a gradient; zeros from there to the capacity
  const int base = blockIdx.x * C;
  const int hi = min(base + C, length);
  const float *__restrict__ srow = src + b * S * ld;
  const float *__restrict__ hrow = est + b * E * ld;
  float *__restrict__ grow = grad + b * E * grad_ld;
  for (int a = base + 4 * tid; a < hi; a += 4 * T) {
    float sv[S][4];
#pragma unroll
    for (int i = 0; i < S; ++i) load4<VEC>(srow + i * ld, a, nl, sv[i]);
    for (int e = 0; e < E; ++e) {
      float hv[4], g[4];
      load4<VEC>(hrow + e * ld, a, nl, hv);
      const float kc = cK[e], cc = cC[e];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = kc;
#pragma unroll
        for (int i = 0; i < S; ++i) v = fmaf(cA[i * E + e], sv[i][j], v);
        v = fmaf(cc, hv[j], v);
        g[j] = a + j < nl ? v : 0.f;
      }
      float *__restrict__ out = grow + e * grad_ld + a;
      if (VEC && a + 4 <= hi) {
        *reinterpret_cast<float4 *>(out) = make_float4(g[0], g[1], g[2], g[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (a + j < hi) out[j] = g[j];
        }
      }
    }
  }
}

template <int S, int E>
inline void launch_partial(hipStream_t st, dim3 grid, bool vec, const float *src, const float *est, int64_t ld,
                           const int32_t *lengths, int length, int64_t b0, double *sums, int64_t stride) {
  if (vec)
    hipLaunchKernelGGL((pit_partial<S, E, true>), grid, dim3(T), 0, st, src, est, ld, lengths, length, b0, sums, stride);
  else
    hipLaunchKernelGGL((pit_partial<S, E, false>), grid, dim3(T), 0, st, src, est, ld, lengths, length, b0, sums,
                       stride);
}

template <int S>
inline void launch_partial_e(int E, hipStream_t st, dim3 grid, bool vec, const float *src, const float *est, int64_t ld,
                             const int32_t *lengths, int length, int64_t b0, double *sums, int64_t stride) {
  // (E <= S: the ten instantiations)
  if constexpr (S >= 4)
    if (E == 4) return launch_partial<S, 4>(st, grid, vec, src, est, ld, lengths, length, b0, sums, stride);
  if constexpr (S >= 3)
    if (E == 3) return launch_partial<S, 3>(st, grid, vec, src, est, ld, lengths, length, b0, sums, stride);
  if constexpr (S >= 2)
    if (E == 2) return launch_partial<S, 2>(st, grid, vec, src, est, ld, lengths, length, b0, sums, stride);
  launch_partial<S, 1>(st, grid, vec, src, est, ld, lengths, length, b0, sums, stride);
}

template <int S>
inline void launch_grad(hipStream_t st, dim3 grid, bool vec, const float *src, const float *est, int64_t ld,
                        const int32_t *lengths, int length, int64_t b0, int E, int zero_mean, const double *sums,
                        int64_t stride, const float *g_si, const float *g_snr, float *grad, int64_t grad_ld) {
  if (vec)
    hipLaunchKernelGGL((pit_grad<S, true>), grid, dim3(T), 0, st, src, est, ld, lengths, length, b0, E, zero_mean, sums,
                       stride, g_si, g_snr, grad, grad_ld);
  else
    hipLaunchKernelGGL((pit_grad<S, false>), grid, dim3(T), 0, st, src, est, ld, lengths, length, b0, E, zero_mean,
                       sums, stride, g_si, g_snr, grad, grad_ld);
}

inline bool shape_ok(int64_t batch, int32_t S, int32_t E, int64_t length, int64_t ld) {
  return batch >= 0 && S >= 1 && S <= MAXS && E >= 1 && E <= S && length >= 1 && length <= kMaxLength && ld >= length;
}

}  // namespace pitsdr
}  // namespace fsem

using namespace fsem;

extern "C" int fsem_pitsdr_max_sources(void) { return pitsdr::MAXS; }

extern "C" int64_t fsem_pitsdr_chunk(int32_t sample_rate) { return pitsdr::rate_ok(sample_rate) ? pitsdr::C : 0; }

extern "C" int64_t fsem_pitsdr_sums_doubles(int32_t n_src, int32_t n_est, int64_t length, int32_t sample_rate) {
  if (!pitsdr::shape_ok(0, n_src, n_est, length, length) || !pitsdr::rate_ok(sample_rate)) return 0;
  return pitsdr::sums_doubles(n_src, n_est, length);
}

extern "C" int fsem_pitsdr_f32(const float *src, const float *est, int64_t batch, int32_t n_src, int32_t n_est,
                               int64_t length, int64_t ld, const int32_t *lengths, int32_t sample_rate,
                               int32_t zero_mean, int32_t criterion, double *sums, float *si_mat, float *snr_mat,
                               int32_t *perm, void *stream) {
  using namespace pitsdr;
  if (!src || !est || !sums || !si_mat || !snr_mat || !perm || !shape_ok(batch, n_src, n_est, length, ld) ||
      criterion < 0 || criterion > 2)
    return FSEM_EINVAL;
  if (!rate_ok(sample_rate)) return FSEM_ERATE;
  if (batch == 0) return FSEM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = n_src, E = n_est;
  const int nchunk = (int)chunks(length);
  const int64_t stride = sums_doubles(S, E, length);
  // 16-byte loads where every row of both operands starts on a 16-byte boundary
  const bool vec = (((uintptr_t)src | (uintptr_t)est) & 15) == 0 && ld % 4 == 0;
  for (int64_t b0 = 0; b0 < batch; b0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)nchunk, batch, b0);
    switch (S) {
      case 1: launch_partial_e<1>(E, st, grid, vec, src, est, ld, lengths, (int)length, b0, sums, stride); break;
      case 2: launch_partial_e<2>(E, st, grid, vec, src, est, ld, lengths, (int)length, b0, sums, stride); break;
      case 3: launch_partial_e<3>(E, st, grid, vec, src, est, ld, lengths, (int)length, b0, sums, stride); break;
      default: launch_partial_e<4>(E, st, grid, vec, src, est, ld, lengths, (int)length, b0, sums, stride); break;
    }
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(pit_finish, dim3((unsigned)((batch + FT - 1) / FT)), dim3(FT), 0, st, sums, stride, lengths,
                     (int)length, batch, S, E, zero_mean, criterion, si_mat, snr_mat, perm);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}

extern "C" int fsem_pitsdr_grad_f32(const float *src, const float *est, int64_t batch, int32_t n_src, int32_t n_est,
                                    int64_t length, int64_t ld, const int32_t *lengths, int32_t zero_mean,
                                    const double *sums, const float *g_si, const float *g_snr, float *grad,
                                    int64_t grad_ld, void *stream) {
  using namespace pitsdr;
  if (!src || !est || !sums || !g_si || !g_snr || !grad || !shape_ok(batch, n_src, n_est, length, ld) ||
      grad_ld < length)
    return FSEM_EINVAL;
  if (batch == 0) return FSEM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = n_src, E = n_est;
  const int nchunk = (int)chunks(length);
  const int64_t stride = sums_doubles(S, E, length);
  const bool vec = (((uintptr_t)src | (uintptr_t)est | (uintptr_t)grad) & 15) == 0 && ld % 4 == 0 && grad_ld % 4 == 0;
  for (int64_t b0 = 0; b0 < batch; b0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)nchunk, batch, b0);
    switch (S) {
      case 1:
        launch_grad<1>(st, grid, vec, src, est, ld, lengths, (int)length, b0, E, zero_mean, sums, stride, g_si, g_snr,
                       grad, grad_ld);
        break;
      case 2:
        launch_grad<2>(st, grid, vec, src, est, ld, lengths, (int)length, b0, E, zero_mean, sums, stride, g_si, g_snr,
                       grad, grad_ld);
        break;
      case 3:
        launch_grad<3>(st, grid, vec, src, est, ld, lengths, (int)length, b0, E, zero_mean, sums, stride, g_si, g_snr,
                       grad, grad_ld);
        break;
      default:
        launch_grad<4>(st, grid, vec, src, est, ld, lengths, (int)length, b0, E, zero_mean, sums, stride, g_si, g_snr,
                       grad, grad_ld);
        break;
    }
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}
