// BSS-eval of mixtures: SDR, SIR and SAR of E estimates against S sources with a 512-tap
// distortion filter (include/fsem.h, "BSS-eval"), an extension beside the one-source BSSSDR
// (bsssdr.hip).  The two share the 512-lag direct correlation of fsem_corr512.h: its constants,
// the LDS group layout, a wave's step loop and the four-wave reduction; each fills its own LDS
// pieces, and the norm kernels and the solvers are each file's own.
//
//   bse_norm_partial  grid (norm chunk, signal).  As sdr_norm_partial, one sum of squares per
//                     (signal, chunk of NC = 8192 samples); launched for the sources and for the
//                     estimates.
//   bse_norms         one thread per signal: the records in ascending order, max((float)sqrt, 1e-6f).
//   bse_corr          grid (chunk, (mixture, source i, group)), 4 waves.  sdr_corr's direct form with
//                     the broadcast signal s'_i apart from the window signals: a group is two of the
//                     S + E signals (sources first), so a block forms two of the 512-lag correlations
//                     C_ij / b_ie per pass over s'_i -- 16 accumulators and 32 window doubles per
//                     lane, what sdr_corr holds.  LDS: the piece of s'_i (2048 doubles) and the
//                     pieces of the two windows (2560 each), groups of 8 doubles 80 bytes apart:
//                     71680 bytes, 2 blocks per CU.  A group of one signal (S + E odd) runs its
//                     second window on zeros and writes no second record.  One record of 512
//                     doubles per (mixture, chunk, correlation), the quarters added as
//                     ((w0 + w1) + w2) + w3.
//   bse_sum           one thread per (mixture, correlation, lag): the chunk records in ascending order
//                     into the head of the mixture's `corr` block.
//   bse_solve<S>      one block per mixture; a system is solved by one wave.  The quadratic forms
//                     q = d^T T^-1 d of the S scalar systems T_i = Toeplitz(C_ii) (wave 0, one after
//                     the other) and of the block system G (wave 1; S = 1 has none), each by a
//                     (block) Levinson recursion that carries no solution: with the backward
//                     predictors B^(n) and their error matrices Eb_n,
//                     T^-1 = sum_n B^(n) Eb_n^-1 B^(n)^T, so q = sum_n g_n^T Eb_n^-1 g_n,
//                     g_n = B^(n)^T d -- a sum of squares through the Cholesky factor of Eb_n.  The
//                     forward predictor F and the reversed backward predictor Br live in LDS
//                     (element-major: lanes on consecutive blocks); at order n the lane of block l
//                     updates the pair F[l], Br[n - l] from each other (F[l] -= Br[n - l] Kf,
//                     Br[n - l] -= F[l] Kb: no other lane reads or writes either), and adds its
//                     terms of g_n (Br[n - l]^T d_l) and of the next order's reflection sum
//                     (Gamma_{n + 1 - l} F[l]); Gamma and d come from global memory.  The S x S
//                     work (two Cholesky factors, two solves, the error updates) is done by every
//                     lane on wave-uniform values.  The waves meet at one barrier; thread 0 writes
//                     the mixture's energies, all NaN where any system broke down.
//   bse_scores        one thread per mixture: the clamped logs, the assignment, the outputs.
//
// Every sum has one order that depends on n alone; no atomics; a mixture's outputs do not depend
// on the batch size, its position, the row capacity or the stream.
#include <math.h>

#include "fsem_corr512.h"

namespace fsem {
namespace bsseval {

using namespace corr512;           // T, NWAVE, K, NC, C, SC, QT, G, GP, chunks, norm_chunks
constexpr int NGA = SC / G;        // groups of the broadcast signal's piece
constexpr int NGW = (SC + K) / G;  // groups of a window signal's extent
constexpr int MAXS = 4;            // sources, and estimates, of a mixture
static_assert(SC % T == 0 && K % T == 0, "the fill loop is block-uniform");
static_assert(NGA * GP + 2 * NGW * GP >= NWAVE * 2 * K, "the four waves' sums fit the pieces' LDS");

__host__ __device__ inline int pairs(int S, int E) { return S * S + S * E; }  // correlations of a mixture
// A mixture's block of `corr`: the summed correlations, the chunk records, the norm records.
inline int64_t corr_doubles(int S, int E, int64_t length) {
  return (int64_t)pairs(S, E) * K * (1 + chunks(length)) + (int64_t)(S + E) * norm_chunks(length);
}

__global__ __launch_bounds__(T) void bse_norm_partial(const float *__restrict__ x, int64_t ld,
                                                      const int32_t *__restrict__ lengths, int length, int64_t rows,
                                                      int nsig, int sig0, double *__restrict__ corr, int64_t stride,
                                                      int64_t npoff, int nnc) {
  __shared__ double red[NWAVE];
  const int tid = threadIdx.x;
  const int64_t row = grid_row_yz();
  if (row >= rows) return;
  const int64_t b = row / nsig;
  const int sig = (int)(row - b * nsig);
  const int c = blockIdx.x;
  const int n = row_length(lengths, b, length);
  const int base = c * NC;  // < length + NC <= 2^29 + 2^13
  if (base >= n) return;    // (bse_norms reads ceil(n / NC) records of this signal)
  const float *__restrict__ xr = x + row * ld;
  double ss = 0;
#pragma unroll 8
  for (int j = 0; j < NC / T; ++j) {
    const int a = base + tid + T * j;
    const double v = a < n ? xr[a] : 0.f;
    ss = fma(v, v, ss);
  }
  ss = wave_sum_d(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  if (tid == 0) corr[b * stride + npoff + (int64_t)(sig0 + sig) * nnc + c] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void bse_norms(const double *__restrict__ corr, int64_t stride, int64_t npoff, int nnc,
                                                const int32_t *__restrict__ lengths, int length, int64_t rows, int nsig,
                                                float *__restrict__ norms) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= rows) return;
  const int64_t b = row / nsig;
  const int sig = (int)(row - b * nsig);
  const int n = row_length(lengths, b, length);
  const int nc = (n + NC - 1) / NC;
  const double *__restrict__ p = corr + b * stride + npoff + (int64_t)sig * nnc;
  double ss = 0;
  for (int c = 0; c < nc; ++c) ss += p[c];
  // a non-finite sample makes the sum non-finite (NaN < x is false: the norm stays NaN)
  float nm = (float)sqrt(ss);
  norms[row] = nm < 1e-6f ? 1e-6f : nm;
}

// Record of correlation (source i, window signal w) within a set of pairs(S, E) records: C_ij
// (i-major) first, then b_ie.
__device__ __forceinline__ int pair_index(int i, int w, int S, int E) {
  return w < S ? i * S + w : S * S + i * E + (w - S);
}

__global__ __launch_bounds__(T) void bse_corr(const float *__restrict__ src, const float *__restrict__ est, int64_t ld,
                                              const int32_t *__restrict__ lengths, int length, int64_t rows, int S,
                                              int E, const float *__restrict__ norms, double *__restrict__ corr,
                                              int64_t stride, int nchunk) {
  __shared__ __attribute__((aligned(16))) double lds[NGA * GP + 2 * NGW * GP];  // 71680 bytes: 2 blocks per CU
  double *__restrict__ A = lds;
  double *__restrict__ W0 = lds + NGA * GP;
  double *__restrict__ W1 = W0 + NGW * GP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = grid_row_yz();
  if (row >= rows) return;  // (block-uniform)
  const int nsig = S + E, ngrp = (nsig + 1) >> 1;
  const int64_t b = row / (S * ngrp);
  const int rem = (int)(row - b * (S * ngrp));
  const int i = rem / ngrp, w0 = 2 * (rem - i * ngrp), w1 = w0 + 1;
  const bool two = w1 < nsig;
  const int c = blockIdx.x;
  const int n = row_length(lengths, b, length);
  const int base = c * C;  // < length + C <= 2^29 + 2^15
  if (base >= n) return;   // (bse_sum reads ceil(n / C) records of this mixture)
  const float *__restrict__ arow = src + (b * S + i) * ld;
  const float *__restrict__ row0 = w0 < S ? src + (b * S + w0) * ld : est + (b * E + (w0 - S)) * ld;
  const float *__restrict__ row1 = !two ? row0 : w1 < S ? src + (b * S + w1) * ld : est + (b * E + (w1 - S)) * ld;
  const float na = norms[b * nsig + i], n0 = norms[b * nsig + w0], n1 = norms[b * nsig + (two ? w1 : w0)];
  double acc0[G], acc1[G];
#pragma unroll
  for (int j = 0; j < G; ++j) acc0[j] = acc1[j] = 0.0;
  for (int p0 = base; p0 < base + C && p0 < n; p0 += SC) {  // (block-uniform)
    __syncthreads();  // the previous piece has been read
    for (int x = tid; x < SC + K; x += T) {
      const int t = p0 + x;
      const bool in = t < n;
      // the float32 quotients, correctly rounded
      if (x < SC) A[gpad(x)] = (double)(in ? arow[t] / na : 0.f);
      W0[gpad(x)] = (double)(in ? row0[t] / n0 : 0.f);
      W1[gpad(x)] = (double)(in && two ? row1[t] / n1 : 0.f);
    }
    __syncthreads();
    corr_quarter(A, W0, W1, wave, lane, p0, n, acc0, acc1);
  }
  corr_gather(lds, wave, lane, acc0, acc1);
  double *__restrict__ rec = corr + b * stride + (int64_t)pairs(S, E) * K * (1 + c);
  double *__restrict__ out0 = rec + pair_index(i, w0, S, E) * K;
  double *__restrict__ out1 = rec + pair_index(i, two ? w1 : w0, S, E) * K;
#pragma unroll
  for (int o = tid; o < 2 * K; o += T) {
    const double v = corr_total(lds, o);
    if (o < K) out0[o] = v;
    else if (two) out1[o - K] = v;
  }
}

__global__ __launch_bounds__(T) void bse_sum(double *__restrict__ corr, int64_t stride, int npk,
                                             const int32_t *__restrict__ lengths, int length, int64_t batch) {
  const int64_t b = grid_row_yz();
  if (b >= batch) return;
  const int el = blockIdx.x * T + threadIdx.x;  // < npk (a multiple of T)
  const int n = row_length(lengths, b, length);
  const int nc = (n + C - 1) / C;
  double *__restrict__ p = corr + b * stride;
  double v = 0;
  for (int c = 0; c < nc; ++c) v += p[(int64_t)npk * (1 + c) + el];
  p[el] = v;
}

// L L^T = M (the lower triangle of M is read), Li[j] = 1 / L[j][j]; false where a pivot is not > 0.
template <int S>
__device__ __forceinline__ bool chol(const double (&M)[S][S], double (&L)[S][S], double (&Li)[S]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    double s = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = fma(-L[j][k], L[j][k], s);
    ok = ok && s > 0.0;  // (also false for a NaN)
    const double dj = sqrt(s);
    L[j][j] = dj;
    Li[j] = 1.0 / dj;
#pragma unroll
    for (int i = j + 1; i < S; ++i) {
      double t = M[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t = fma(-L[i][k], L[j][k], t);
      L[i][j] = t * Li[j];
    }
  }
  return ok;
}

// y = L^-1 r.
template <int S>
__device__ __forceinline__ void forward(const double (&L)[S][S], const double (&Li)[S], const double (&r)[S],
                                        double (&y)[S]) {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    double t = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t = fma(-L[i][k], y[k], t);
    y[i] = t * Li[i];
  }
}

// X = (L L^T)^-1 R, or with `transposed` (L L^T)^-1 R^T.
template <int S>
__device__ __forceinline__ void solve_spd(const double (&L)[S][S], const double (&Li)[S], const double (&R)[S][S],
                                          bool transposed, double (&X)[S][S]) {
#pragma unroll
  for (int c = 0; c < S; ++c) {
    double r[S], y[S];
#pragma unroll
    for (int i = 0; i < S; ++i) r[i] = transposed ? R[c][i] : R[i][c];
    forward<S>(L, Li, r, y);
#pragma unroll
    for (int i = S - 1; i >= 0; --i) {
      double t = y[i];
#pragma unroll
      for (int k = i + 1; k < S; ++k) t = fma(-L[k][i], X[k][c], t);
      X[i][c] = t * Li[i];
    }
  }
}

// q[e] = d_e^T T^-1 d_e, e < E, of the symmetric block-Toeplitz T with the S x S blocks
// Gamma_k[a][c] = Gm[a gi + c gj + k] (Gamma_-k = Gamma_k^T) and d_k[e][a] = D[a di + e de + k].
// F, Br: S S K doubles of LDS each.  False where an error matrix is not positive definite.
template <int S>
__device__ bool levinson(const double *__restrict__ Gm, int gi, int gj, const double *__restrict__ D, int di, int de,
                         int E, double *__restrict__ F, double *__restrict__ Br, double (&q)[MAXS]) {
  const int lane = threadIdx.x & 63;
  wave_lds_fence();  // (a previous system's reads of F, Br are done)
  for (int x = lane; x < S * S * K; x += 64) {
    const int k = x & (K - 1), ac = x / K;
    const double v = (k == 0 && ac / S == ac % S) ? 1.0 : 0.0;  // F[0] = Br[0] = I
    F[x] = v;
    Br[x] = v;
  }
  double Ef[S][S], Eb[S][S], Lf[S][S], Lb[S][S], Lfi[S], Lbi[S], eps[S][S];
#pragma unroll
  for (int a = 0; a < S; ++a) {
#pragma unroll
    for (int c = 0; c < S; ++c) {
      Ef[a][c] = Eb[a][c] = Gm[a * gi + c * gj];
      eps[a][c] = Gm[a * gi + c * gj + 1];  // Gamma_1 F[0]
    }
  }
  bool ok = chol<S>(Eb, Lb, Lbi);
  chol<S>(Ef, Lf, Lfi);
#pragma unroll
  for (int e = 0; e < MAXS; ++e) {
    q[e] = 0.0;
    if (e < E) {
      double r[S], y[S];
#pragma unroll
      for (int a = 0; a < S; ++a) r[a] = D[a * di + e * de];
      forward<S>(Lb, Lbi, r, y);
#pragma unroll
      for (int a = 0; a < S; ++a) q[e] = fma(y[a], y[a], q[e]);
    }
  }
  for (int n = 1; n < K && ok; ++n) {
    double Kf[S][S], Kb[S][S];
    solve_spd<S>(Lb, Lbi, eps, false, Kf);  // Eb^-1 eps
    solve_spd<S>(Lf, Lfi, eps, true, Kb);   // Ef^-1 eps^T
#pragma unroll
    for (int a = 0; a < S; ++a) {
#pragma unroll
      for (int c = 0; c < S; ++c) {
        double f = Ef[a][c], bk = Eb[a][c];
#pragma unroll
        for (int r = 0; r < S; ++r) {
          f = fma(-eps[r][a], Kf[r][c], f);   // Ef - eps^T Kf
          bk = fma(-eps[a][r], Kb[r][c], bk);  // Eb - eps Kb
        }
        Ef[a][c] = f;
        Eb[a][c] = bk;
      }
    }
    double g[S][MAXS], en[S][S];
#pragma unroll
    for (int a = 0; a < S; ++a) {
#pragma unroll
      for (int e = 0; e < MAXS; ++e) g[a][e] = 0.0;
#pragma unroll
      for (int c = 0; c < S; ++c) en[a][c] = 0.0;
    }
    wave_lds_fence();  // the previous order's F, Br are written
    // Block l of the pass, l <= n.
    auto trip = [&](int l) {
      double f[S][S], bk[S][S], nf[S][S], nb[S][S], dv[S][MAXS], gv[S][S];
#pragma unroll
      for (int a = 0; a < S; ++a) {
#pragma unroll
        for (int c = 0; c < S; ++c) {
          f[a][c] = F[(a * S + c) * K + l];
          bk[a][c] = Br[(a * S + c) * K + (n - l)];
          // Gamma_{n + 1 - l}, n + 1 - l in [1, K) (the last order has no next: any block, unused)
          gv[a][c] = Gm[a * gi + c * gj + (n + 1 < K ? n + 1 - l : 0)];
        }
#pragma unroll
        for (int e = 0; e < MAXS; ++e) dv[a][e] = e < E ? D[a * di + e * de + l] : 0.0;
      }
#pragma unroll
      for (int a = 0; a < S; ++a) {
#pragma unroll
        for (int c = 0; c < S; ++c) {
          double x = f[a][c], y = bk[a][c];
#pragma unroll
          for (int r = 0; r < S; ++r) {
            x = fma(-bk[a][r], Kf[r][c], x);
            y = fma(-f[a][r], Kb[r][c], y);
          }
          F[(a * S + c) * K + l] = x;
          Br[(a * S + c) * K + (n - l)] = y;
          nf[a][c] = x;
          nb[a][c] = y;
        }
      }
#pragma unroll
      for (int a = 0; a < S; ++a) {
#pragma unroll
        for (int c = 0; c < S; ++c) {
#pragma unroll
          for (int e = 0; e < MAXS; ++e)
            if (e < E) g[a][e] = fma(nb[c][a], dv[c][e], g[a][e]);  // g_n += Br[n - l]^T d_l
#pragma unroll
          for (int r = 0; r < S; ++r) en[a][c] = fma(gv[a][r], nf[r][c], en[a][c]);  // += Gamma_{n + 1 - l} F[l]
        }
      }
    };
#pragma unroll 1
    for (int l = lane; l <= n; l += 64) trip(l);
#pragma unroll
    for (int a = 0; a < S; ++a) {
#pragma unroll
      for (int c = 0; c < S; ++c) eps[a][c] = wave_sum_d(en[a][c]);
#pragma unroll
      for (int e = 0; e < MAXS; ++e)
        if (e < E) g[a][e] = wave_sum_d(g[a][e]);
    }
    ok = chol<S>(Eb, Lb, Lbi);
    ok = chol<S>(Ef, Lf, Lfi) && ok;
#pragma unroll
    for (int e = 0; e < MAXS; ++e) {
      if (e < E) {
        double r[S], y[S];
#pragma unroll
        for (int a = 0; a < S; ++a) r[a] = g[a][e];
        forward<S>(Lb, Lbi, r, y);
#pragma unroll
        for (int a = 0; a < S; ++a) q[e] = fma(y[a], y[a], q[e]);
      }
    }
  }
  return ok;
}

// Waves of a bse_solve block: at S > 1 the scalar systems (wave 0, one after the other) and the block
// system (wave 1) are independent and run side by side.
template <int S>
constexpr int solve_threads() { return S > 1 ? 128 : 64; }

template <int S>
__global__ __launch_bounds__(solve_threads<S>()) void bse_solve(const double *__restrict__ corr, int64_t stride,
                                                                const float *__restrict__ norms,
                                                                const int32_t *__restrict__ lengths, int length,
                                                                int64_t batch, int E, double *__restrict__ coh,
                                                                double *__restrict__ coh_all) {
  // F, Br of the block system (8 KB per element pair; 128 KB at S = 4), then those of the scalar systems
  __shared__ double lds[2 * S * S * K + (S > 1 ? 2 * K : 0)];
  __shared__ double res[(S + 1) * MAXS];  // coh[i][e] at i MAXS + e, coh_all[e] at S MAXS + e
  __shared__ int okw[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = grid_row_xy();
  if (b >= batch) return;  // (block-uniform)
  const int n = row_length(lengths, b, length);
  const double *__restrict__ cm = corr + b * stride;
  const double *__restrict__ dm = cm + S * S * K;  // b_ie at (i E + e) K
  // the rule of n, a non-finite sample (its norm is not finite), a silent source
  bool bad = (int64_t)n + K - 1 < (int64_t)S * K;
  for (int s = 0; s < S + E; ++s) bad = bad || !isfinite(norms[b * (S + E) + s]);
  for (int i = 0; i < S && !bad; ++i) bad = bad || !(cm[(i * S + i) * K] > 0.0);
  if (!bad) {  // (block-uniform)
    bool ok = true;
    if (wave == 0) {
      double *__restrict__ F1 = lds + (S > 1 ? 2 * S * S * K : 0);
#pragma unroll 1
      for (int i = 0; i < S; ++i) {
        double q[MAXS];
        ok = levinson<1>(cm + (i * S + i) * K, 0, 0, dm + i * E * K, 0, K, E, F1, F1 + K, q) && ok;
        if (lane == 0) {
#pragma unroll
          for (int e = 0; e < MAXS; ++e) {
            res[i * MAXS + e] = q[e];
            if (S == 1) res[MAXS + e] = q[e];  // coh_all is coh[0] itself
          }
        }
      }
    } else {
      double q[MAXS];
      ok = levinson<S>(cm, S * K, K, dm, E * K, K, E, lds, lds + S * S * K, q);
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < MAXS; ++e) res[S * MAXS + e] = q[e];
      }
    }
    if (lane == 0) okw[wave] = ok;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (!bad) {
      bad = !okw[0] || (S > 1 && !okw[1]);
      for (int x = 0; x < (S + 1) * MAXS; ++x)
        if (x % MAXS < E) bad = bad || !isfinite(res[x]);
    }
    const double nan = __builtin_nan("");
    for (int e = 0; e < E; ++e) {
      coh_all[b * E + e] = bad ? nan : res[S * MAXS + e];
      for (int i = 0; i < S; ++i) coh[(b * S + i) * E + e] = bad ? nan : res[i * MAXS + e];
    }
  }
}

__device__ __forceinline__ double ratio_db(double num, double den) {
  den = den < 1e-8 ? 1e-8 : den;
  double r = num / den;
  r = r < 1e-8 ? 1e-8 : r;
  return 10.0 * log10(r);
}

__global__ __launch_bounds__(64) void bse_scores(const double *__restrict__ coh, const double *__restrict__ coh_all,
                                                 int64_t batch, int S, int E, int criterion, float *__restrict__ sdr,
                                                 float *__restrict__ sir, float *__restrict__ sar,
                                                 int32_t *__restrict__ perm, float *__restrict__ sdr_mat,
                                                 float *__restrict__ sir_mat) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  double sd[MAXS][MAXS], si[MAXS][MAXS], sa[MAXS];
  bool nan = false;
  for (int e = 0; e < E; ++e) {
    const double ca = coh_all[b * E + e];
    nan = nan || !isfinite(ca);
    sa[e] = ratio_db(ca, 1.0 - ca);
    for (int i = 0; i < S; ++i) {
      const double c = coh[(b * S + i) * E + e];
      nan = nan || !isfinite(c);
      sd[i][e] = ratio_db(c, 1.0 - c);
      si[i][e] = ratio_db(c, ca - c);
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
      for (int e = 0; e < S; ++e) m += criterion == 1 ? si[cand[e]][e] : sd[cand[e]][e];
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
    sdr[b * E + e] = nan ? fnan : (float)sd[p[e]][e];
    sir[b * E + e] = nan ? fnan : (float)si[p[e]][e];
    sar[b * E + e] = nan ? fnan : (float)sa[e];
    perm[b * E + e] = p[e];
    for (int i = 0; i < S; ++i) {
      if (sdr_mat) sdr_mat[(b * S + i) * E + e] = nan ? fnan : (float)sd[i][e];
      if (sir_mat) sir_mat[(b * S + i) * E + e] = nan ? fnan : (float)si[i][e];
    }
  }
}

template <int S>
inline void launch_solve(hipStream_t st, const double *corr, int64_t stride, const float *norms, const int32_t *lengths,
                         int length, int64_t batch, int E, double *coh, double *coh_all) {
  hipLaunchKernelGGL(bse_solve<S>, grid_xy(batch), dim3(solve_threads<S>()), 0, st, corr, stride, norms, lengths, length, batch, E, coh,
                     coh_all);
}

}  // namespace bsseval
}  // namespace fsem

using namespace fsem;

extern "C" int fsem_bsseval_max_sources(void) { return bsseval::MAXS; }

extern "C" int64_t fsem_bsseval_corr_doubles(int32_t n_src, int32_t n_est, int64_t length) {
  if (n_src < 1 || n_src > bsseval::MAXS || n_est < 1 || n_est > bsseval::MAXS || length < 1 || length > kMaxLength)
    return 0;
  return bsseval::corr_doubles(n_src, n_est, length);
}

extern "C" int fsem_bsseval_f32(const float *src, const float *est, int64_t batch, int32_t n_src, int32_t n_est,
                                int64_t length, int64_t ld, const int32_t *lengths, float *norms, double *corr,
                                double *coh, double *coh_all, void *stream) {
  using namespace bsseval;
  if (!src || !est || !norms || !corr || !coh || !coh_all || batch < 0 || n_src < 1 || n_src > MAXS || n_est < 1 ||
      n_est > MAXS || length < 1 || ld < length || length > kMaxLength)
    return FSEM_EINVAL;
  if (batch == 0) return FSEM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = n_src, E = n_est, nsig = S + E, npk = pairs(S, E) * K;
  const int nnc = (int)norm_chunks(length), nchunk = (int)chunks(length);
  const int64_t stride = corr_doubles(S, E, length);
  const int64_t npoff = (int64_t)npk * (1 + nchunk);
  hipLaunchKernelGGL(bse_norm_partial, grid_yz((unsigned)nnc, batch * S), dim3(T), 0, st, src, ld, lengths, (int)length,
                     batch * S, S, 0, corr, stride, npoff, nnc);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(bse_norm_partial, grid_yz((unsigned)nnc, batch * E), dim3(T), 0, st, est, ld, lengths, (int)length,
                     batch * E, E, S, corr, stride, npoff, nnc);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(bse_norms, dim3((unsigned)((batch * nsig + 63) / 64)), dim3(64), 0, st, corr, stride, npoff, nnc,
                     lengths, (int)length, batch * nsig, nsig, norms);
  FSEM_CHECK_LAUNCH();
  const int64_t rows = batch * S * ((nsig + 1) / 2);
  hipLaunchKernelGGL(bse_corr, grid_yz((unsigned)nchunk, rows), dim3(T), 0, st, src, est, ld, lengths, (int)length, rows,
                     S, E, norms, corr, stride, nchunk);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(bse_sum, grid_yz((unsigned)(npk / T), batch), dim3(T), 0, st, corr, stride, npk, lengths,
                     (int)length, batch);
  FSEM_CHECK_LAUNCH();
  switch (S) {
    case 1: launch_solve<1>(st, corr, stride, norms, lengths, (int)length, batch, E, coh, coh_all); break;
    case 2: launch_solve<2>(st, corr, stride, norms, lengths, (int)length, batch, E, coh, coh_all); break;
    case 3: launch_solve<3>(st, corr, stride, norms, lengths, (int)length, batch, E, coh, coh_all); break;
    default: launch_solve<4>(st, corr, stride, norms, lengths, (int)length, batch, E, coh, coh_all); break;
  }
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}

extern "C" int fsem_bsseval_scores_f32(const double *coh, const double *coh_all, int64_t batch, int32_t n_src,
                                       int32_t n_est, int32_t criterion, float *sdr, float *sir, float *sar,
                                       int32_t *perm, float *sdr_mat, float *sir_mat, void *stream) {
  using namespace bsseval;
  if (!coh || !coh_all || !sdr || !sir || !sar || !perm || batch < 0 || n_src < 1 || n_src > MAXS || n_est < 1 ||
      n_est > n_src || criterion < 0 || criterion > 2)
    return FSEM_EINVAL;
  if (batch == 0) return FSEM_OK;
  hipLaunchKernelGGL(bse_scores, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, coh, coh_all,
                     batch, (int)n_src, (int)n_est, (int)criterion, sdr, sir, sar, perm, sdr_mat, sir_mat);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}
