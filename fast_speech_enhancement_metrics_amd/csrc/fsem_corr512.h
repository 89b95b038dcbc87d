// The 512-lag direct correlation of bsssdr.hip (sdr_corr) and bsseval.hip (bse_corr), in double on
// the vector FMA pipe: a block of 4 waves takes a chunk of C samples in pieces of SC; a piece's
// signals lie in LDS as doubles, groups of G = 8 stored GP = 10 doubles apart (80 bytes: the lanes'
// 16-byte reads fall on distinct banks); wave w takes the piece's samples [512 w, 512 w + 512), 8
// at a time in ascending order, lane l owns the lags 8 l ... 8 l + 7 of two correlations.  Each
// kernel fills its own pieces and writes its own records.
#pragma once
#include "fsem_common.h"

namespace fsem {
namespace corr512 {

constexpr int T = 256;          // threads of a block (4 waves)
constexpr int NWAVE = T / 64;
constexpr int K = 512;          // filter length: lags 0 ... 511
constexpr int NC = 8192;        // samples per record of a sum of squares
constexpr int C = 32768;        // samples per record of partial correlations
constexpr int SC = 2048;        // samples per piece in LDS
constexpr int QT = SC / NWAVE;  // a wave's samples of a piece
constexpr int G = 8;            // a group: 8 doubles, stored GP doubles apart
constexpr int GP = 10;
static_assert(QT == K && K == 8 * 64, "a lane owns 8 lags; a wave's quarter of a piece is 512 samples");
static_assert(C % SC == 0 && SC % (G * NWAVE) == 0, "pieces tile a chunk, steps tile a quarter");

inline int64_t chunks(int64_t length) { return (length + C - 1) / C; }
inline int64_t norm_chunks(int64_t length) { return (length + NC - 1) / NC; }

// Element i of a piece's extent lies at gpad(i) doubles.
__device__ __forceinline__ int gpad(int i) { return (i >> 3) * GP + (i & 7); }

__device__ __forceinline__ void load_group(const double *g, double v[G]) {
#pragma unroll
  for (int e = 0; e < G; e += 2) {
    const double2 d = *reinterpret_cast<const double2 *>(g + e);
    v[e] = d.x;
    v[e + 1] = d.y;
  }
}

// This wave's quarter of the piece at sample p0 of a row of n: acc0[j] += sum_t A[t] W0[t + 8 lane + j]
// and acc1 likewise with W1, t over the quarter.  A is the broadcast signal's piece (SC elements
// read), W0 and W1 the window signals' (SC + K); A may be W0.  Per step of 8 samples a lane reads
// the 8 A[t] (one address for the wave) and ONE new group of each window -- its window
// t + 8 lane ... t + 8 lane + 15 slides by 8, the upper half becomes the lower half -- and issues
// 128 FMAs.
__device__ __forceinline__ void corr_quarter(const double *A, const double *W0, const double *W1, int wave, int lane,
                                             int p0, int n, double acc0[G], double acc1[G]) {
  const int g0 = wave * (QT / G);
  double lo0[G], lo1[G];
  load_group(W0 + (g0 + lane) * GP, lo0);
  load_group(W1 + (g0 + lane) * GP, lo1);
#pragma unroll 2  // (two steps swap the roles of the window's halves: 19 register moves per 256 FMAs, not 64)
  for (int st = 0; st < QT / G; ++st) {
    if (p0 + G * (g0 + st) >= n) break;  // (wave-uniform: every A[t] of the step is zero)
    double a[G], hi0[G], hi1[G];
    load_group(A + (g0 + st) * GP, a);                // group < SC / G
    load_group(W0 + (g0 + st + lane + 1) * GP, hi0);  // group <= 192 + 63 + 63 + 1 < (SC + K) / G
    load_group(W1 + (g0 + st + lane + 1) * GP, hi1);
#pragma unroll
    for (int i = 0; i < G; ++i) {
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int w = i + j;  // lag 8 lane + j at sample t + i: element t + i + 8 lane + j
        acc0[j] = fma(a[i], w < G ? lo0[w] : hi0[w - G], acc0[j]);
        acc1[j] = fma(a[i], w < G ? lo1[w] : hi1[w - G], acc1[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      lo0[j] = hi0[j];
      lo1[j] = hi1[j];
    }
  }
}

// After the chunk: the four waves' sums into red ([NWAVE][2 K] doubles over the pieces' LDS, by
// the whole block), element o < K of acc0's correlation and K + o of acc1's; then corr_total(red, o).
__device__ __forceinline__ void corr_gather(double *__restrict__ red, int wave, int lane, const double acc0[G],
                                            const double acc1[G]) {
  __syncthreads();  // the last piece has been read
#pragma unroll
  for (int j = 0; j < G; ++j) {
    red[wave * 2 * K + G * lane + j] = acc0[j];
    red[wave * 2 * K + K + G * lane + j] = acc1[j];
  }
  __syncthreads();
}
__device__ __forceinline__ double corr_total(const double *__restrict__ red, int o) {
  return ((red[o] + red[2 * K + o]) + red[4 * K + o]) + red[6 * K + o];
}

}  // namespace corr512
}  // namespace fsem
