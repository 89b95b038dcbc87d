// The kernels of the BSS-eval SDR with a 512-tap distortion filter (include/fsem_bsssdr.h), shared by
// bsssdr.hip (libfsem_bsssdr.so: the scores) and bsssdr_grad.hip (libfsem.so: the scores with the
// records the backward reads).  Each library compiles its own copy.  Two reads of each input.
//
//   sdr_norm_partial  grid (chunk, row).  A chunk is NC = 8192 samples: thread t takes the samples
//                     t, t + 256, ... of the chunk, in that order, and adds s s and h h in double
//                     (products of float32 samples, exact in double); the block's 256 sums are added
//                     in a fixed tree.  One 16-byte record per (row, chunk); no atomics.
//   sdr_norms         one thread per row: the records in ascending order, the two norms
//                     max((float)sqrt(sum), 1e-6f); NaN / inf for a row with a non-finite sample.
//   sdr_corr          grid (chunk, row), 4 waves (the step loop and the reduction are fsem_corr512.h's,
//                     shared with bsseval.hip): the direct form of r[k] = sum_t s'[t] s'[t + k] and
//                     b[k] = sum_t s'[t] h'[t + k], k = 0 ... 511, in double on the vector FMA
//                     pipe, exact up to the rounding of the double sums.  A chunk is C = 32768 samples,
//                     taken in pieces of SC = 2048: the block puts s'[t], h'[t] for
//                     t in [p, p + SC + 512) into LDS as doubles (the float32 quotients s / |s|;
//                     zero at and past n), wave w takes the piece's t in [512 w, 512 w + 512), 8 at
//                     a time in ascending order, and lane l owns the lags 8 l ... 8 l + 7.  Per step
//                     of 8 samples a lane reads the 8 s'[t] (one address for the wave) and ONE new
//                     group of 8 values of each signal -- its window t + 8 l ... t + 8 l + 15 slides
//                     by 8, the upper half becomes the lower half -- and issues 128 FMAs: 12 LDS
//                     reads of 16 bytes per lane against 128 FMAs.  Groups of 8 doubles are 80 bytes
//                     apart in LDS, so the lanes' 16-byte reads (64 bytes apart without the gap: 4
//                     lanes per bank) fall on distinct banks.  After the chunk the four waves' sums
//                     are added as ((w0 + w1) + w2) + w3 and written as one record of 1024 doubles
//                     per (row, chunk).
//   sdr_solve         one wave per row: the chunk records in ascending order, then the
//                     Levinson-Durbin recursion for R x = b in double, lane l holding the elements
//                     l, l + 64, ... of the predictor and of the solution; the reversed predictor
//                     goes through LDS, the two inner products of an order through one xor
//                     exchange each.  Then coh = b . x and the score.  Given a record (Rec) it
//                     also leaves there what the backward reads: x, coh and the row's flags.
//
// Every sum has one order that depends on n alone: a row's score does not depend on the batch
// size, the row's position, the row capacity, the alignment or the stream.
#pragma once
#include <math.h>

#include "fsem_corr512.h"

namespace fsem {
namespace bsssdr {

using namespace corr512;          // T, NWAVE, K, NC, C, SC, QT, G, GP, chunks, norm_chunks
constexpr int NG = (SC + K) / G;  // groups of a piece's extent
static_assert(2 * NG * GP >= NWAVE * 2 * K, "the four waves' sums fit the piece's LDS");

struct Part {
  double ss, hh;  // sum s s, sum h h over the chunk's samples
};
static_assert(sizeof(Part) == 16, "one record is 16 bytes");

// What sdr_solve leaves for the backward (bsssdr_grad.hip), one per row.
constexpr int32_t kRowBad = 1;      // the score is NaN: a singular system or a non-finite sample
constexpr int32_t kRowClamped = 2;  // the estimate's float32 norm was below 1e-6: nh is the constant 1e-6
struct Rec {
  double x[K];  // the solution of R x = b
  double coh;   // b . x
  int32_t flags;
  int32_t pad;
};
static_assert(sizeof(Rec) == 8 * K + 16, "one record is 4112 bytes");

__global__ __launch_bounds__(T) void sdr_norm_partial(const float *__restrict__ ref, const float *__restrict__ deg,
                                                      int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                      int64_t r0, Part *__restrict__ part, int nchunk) {
  __shared__ double red[NWAVE][2];
  const int tid = threadIdx.x;
  const int64_t row = r0 + blockIdx.y;
  const int c = blockIdx.x;
  const int n = row_length(lengths, row, length);
  const int base = c * NC;  // < length + NC <= 2^29 + 2^13
  if (base >= n) return;    // (sdr_norms reads ceil(n / NC) records of this row)
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  double ss = 0, hh = 0;
#pragma unroll 8
  for (int j = 0; j < NC / T; ++j) {
    const int a = base + tid + T * j;
    const bool in = a < n;
    const double sd = in ? srow[a] : 0.f, hd = in ? hrow[a] : 0.f;
    ss = fma(sd, sd, ss);
    hh = fma(hd, hd, hh);
  }
  ss = wave_sum_d(ss);
  hh = wave_sum_d(hh);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = ss;
    red[tid >> 6][1] = hh;
  }
  __syncthreads();
  if (tid < 2) {
    const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    Part *__restrict__ p = part + (row * nchunk + c);
    if (tid == 0) p->ss = v;
    else p->hh = v;
  }
}

__global__ __launch_bounds__(64) void sdr_norms(const Part *__restrict__ part, int nchunk,
                                                const int32_t *__restrict__ lengths, int length, int64_t B,
                                                float2 *__restrict__ nrm) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int n = row_length(lengths, b, length);
  const int nc = (n + NC - 1) / NC;
  const Part *__restrict__ p = part + b * nchunk;
  double ss = 0, hh = 0;
  for (int c = 0; c < nc; ++c) {
    ss += p[c].ss;
    hh += p[c].hh;
  }
  // a non-finite sample makes its sum non-finite (NaN < x is false: the norm stays NaN)
  float ns = (float)sqrt(ss), nh = (float)sqrt(hh);
  ns = ns < 1e-6f ? 1e-6f : ns;
  nh = nh < 1e-6f ? 1e-6f : nh;
  nrm[b] = make_float2(ns, nh);
}

__global__ __launch_bounds__(T) void sdr_corr(const float *__restrict__ ref, const float *__restrict__ deg, int64_t ld,
                                              const int32_t *__restrict__ lengths, int length, int64_t r0,
                                              const float2 *__restrict__ nrm, double *__restrict__ part, int nchunk) {
  __shared__ __attribute__((aligned(16))) double lds[2 * NG * GP];  // 51200 bytes: 3 blocks per CU
  double *__restrict__ S = lds;
  double *__restrict__ H = lds + NG * GP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = r0 + blockIdx.y;
  const int c = blockIdx.x;
  const int n = row_length(lengths, row, length);
  const int base = c * C;  // < length + C <= 2^29 + 2^15
  if (base >= n) return;   // (sdr_solve reads ceil(n / C) records of this row)
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  const float2 nm = nrm[row];
  double accR[G], accB[G];
#pragma unroll
  for (int j = 0; j < G; ++j) accR[j] = accB[j] = 0.0;
  for (int p0 = base; p0 < base + C && p0 < n; p0 += SC) {  // (block-uniform)
    __syncthreads();  // the previous piece has been read
    for (int i = tid; i < SC + K; i += T) {
      const int t = p0 + i;
      const bool in = t < n;
      // the float32 quotient, correctly rounded, as the reference's preprocess_speech takes it
      const float sq = in ? srow[t] / nm.x : 0.f;
      const float hq = in ? hrow[t] / nm.y : 0.f;
      S[gpad(i)] = (double)sq;
      H[gpad(i)] = (double)hq;
    }
    __syncthreads();
    corr_quarter(S, S, H, wave, lane, p0, n, accR, accB);  // s' is the broadcast signal and the first window
  }
  corr_gather(lds, wave, lane, accR, accB);
  double *__restrict__ out = part + (row * nchunk + c) * (2 * K);
#pragma unroll
  for (int o = tid; o < 2 * K; o += T) out[o] = corr_total(lds, o);
}

// rec: NULL, or [rows] records (with npart, nnc: the rows' sums of squares, as sdr_norms reads them).
__global__ __launch_bounds__(64) void sdr_solve(const double *__restrict__ part, int nchunk,
                                                const float2 *__restrict__ nrm,
                                                const int32_t *__restrict__ lengths, int length, double load_diag,
                                                float *__restrict__ out, Rec *__restrict__ rec,
                                                const Part *__restrict__ npart, int nnc) {
  __shared__ double R[K], Bv[K], A[K];
  constexpr int J = K / 64;
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int n = row_length(lengths, row, length);
  const int nc = (n + C - 1) / C;
  const double *__restrict__ p = part + row * nchunk * (2 * K);
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int i = lane + 64 * j;
    double r = 0, b = 0;
    for (int c = 0; c < nc; ++c) {
      r += p[(int64_t)c * (2 * K) + i];
      b += p[(int64_t)c * (2 * K) + K + i];
    }
    R[i] = i == 0 ? r + load_diag : r;
    Bv[i] = b;
  }
  wave_lds_fence();
  const float2 nm = nrm[row];
  const double r00 = R[0];
  // singular: r[0] == 0 (a silent clean row, n == 0); non-finite: a NaN or inf sample
  bool bad = !(r00 > 0.0) || !isfinite(nm.x) || !isfinite(nm.y);
  double E = r00;
  double av[J], xv[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int i = lane + 64 * j;
    av[j] = i == 0 ? 1.0 : 0.0;  // the predictor [1, a1, ..., am], zero past m
    xv[j] = i == 0 ? Bv[0] / r00 : 0.0;
    A[i] = av[j];
  }
  for (int m = 1; m < K && !bad; ++m) {
    wave_lds_fence();
    double acc = 0, q = 0;
    double ar[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int d = m - (lane + 64 * j);  // in (-512, 512)
      const double rr = R[d < 0 ? -d : d];
      acc = fma(av[j], rr, acc);  // sum_{i < m} a[i] r[m - i] (a[i] = 0 for i >= m)
      q = fma(xv[j], rr, q);      // sum_{i < m} x[i] r[m - i] (x[i] = 0 for i >= m)
      const double ad = A[d < 0 ? 0 : d];
      ar[j] = d >= 0 ? ad : 0.0;  // the reversed predictor a[m - i], i <= m
    }
    acc = wave_sum_d(acc);
    q = wave_sum_d(q);
    const double k = -acc / E;
    wave_lds_fence();  // (A has been read)
#pragma unroll
    for (int j = 0; j < J; ++j) {
      av[j] = fma(k, ar[j], av[j]);
      A[lane + 64 * j] = av[j];
    }
    E *= 1.0 - k * k;
    bad = !(E > 0.0);  // also a NaN
    wave_lds_fence();
    const double lam = (Bv[m] - q) / E;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int d = m - (lane + 64 * j);
      const double ad = A[d < 0 ? 0 : d];
      xv[j] = fma(lam, d >= 0 ? ad : 0.0, xv[j]);
    }
  }
  double coh = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) coh = fma(Bv[lane + 64 * j], xv[j], coh);
  coh = wave_sum_d(coh);
  const bool nan_row = bad || !isfinite(coh);
  if (lane == 0) {
    double den = 1.0 - coh;
    den = den < 1e-8 ? 1e-8 : den;
    double ratio = coh / den;
    ratio = ratio < 1e-8 ? 1e-8 : ratio;
    out[row] = nan_row ? __builtin_nanf("") : (float)(10.0 * log10(ratio));
  }
  if (rec) {
    Rec *__restrict__ rc = rec + row;
#pragma unroll
    for (int j = 0; j < J; ++j) rc->x[lane + 64 * j] = xv[j];
    if (lane == 0) {
      // the estimate's norm before its clamp, as sdr_norms takes it: the same records, order and comparison
      const Part *__restrict__ q = npart + row * nnc;
      double hh = 0;
      for (int c = 0; c < (n + NC - 1) / NC; ++c) hh += q[c].hh;
      const bool clamped = (float)sqrt(hh) < 1e-6f;
      rc->coh = coh;
      rc->flags = (nan_row ? kRowBad : 0) | (clamped ? kRowClamped : 0);
      rc->pad = 0;
    }
  }
}

// Workspace: the rows' norms, one record of sums of squares per (row, norm chunk), one record of
// partial correlations per (row, chunk).
struct Ws {
  float2 *nrm;
  Part *npart;
  double *part;
};
inline Ws layout(Arena &a, int64_t batch, int64_t length) {
  Ws w;
  w.nrm = a.take<float2>((size_t)batch);
  w.npart = a.take<Part>((size_t)batch * (size_t)norm_chunks(length));
  w.part = a.take<double>((size_t)batch * (size_t)chunks(length) * (size_t)(2 * K));
  return w;
}

// The four launches of a scoring call on the workspace w (batch >= 1); rec as sdr_solve takes it.
inline int launch_scores(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                         const int32_t *lengths, double load_diag, float *sdr, const Ws &w, Rec *rec, hipStream_t st) {
  const int nnc = (int)norm_chunks(length);
  const int nchunk = (int)chunks(length);
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    hipLaunchKernelGGL(sdr_norm_partial, grid_slice((unsigned)nnc, batch, r0), dim3(T), 0, st, ref, deg, ld, lengths,
                       (int)length, r0, w.npart, nnc);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(sdr_norms, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st, w.npart, nnc, lengths,
                     (int)length, batch, w.nrm);
  FSEM_CHECK_LAUNCH();
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    hipLaunchKernelGGL(sdr_corr, grid_slice((unsigned)nchunk, batch, r0), dim3(T), 0, st, ref, deg, ld, lengths,
                       (int)length, r0, w.nrm, w.part, nchunk);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(sdr_solve, dim3((unsigned)batch), dim3(64), 0, st, w.part, nchunk, w.nrm, lengths, (int)length,
                     load_diag, sdr, rec, w.npart, nnc);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}

}  // namespace bsssdr
}  // namespace fsem
