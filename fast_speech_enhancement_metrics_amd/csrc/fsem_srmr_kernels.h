// What SRMR's forward (srmr.hip) and its gradient (srmr_grad.hip) share: the geometry of a tile, the
// filters' constants and how the host forms them, the float32 complex helpers and the two chunked
// scans that carry filter state through a tile of 4096 samples -- the analytic gammatone (one lane
// per 16 samples) and the modulation biquads (one lane per filter and 128-sample segment).  Each
// source compiles its own copy.
#pragma once
#include <algorithm>
#include <complex>
#include <math.h>

#include "fsem_common.h"

namespace fsem {
namespace srmr {

constexpr int NCH = 23;          // gammatone channels
constexpr int NMOD = 8;          // modulation filters
constexpr int T = 256;           // threads of an energy block
constexpr int C = 16;            // gammatone samples per lane and tile
constexpr int TILE = T * C;      // 4096 samples
constexpr int NSEG = 32;         // modulation segments per tile (half a wave)
constexpr int SEG = TILE / NSEG; // 128 samples
constexpr int SEGP = SEG + 1;    // a segment's LDS stride (bank spread)
constexpr int NLEV = 5;          // scan levels over NSEG segments
constexpr int RT = 256;          // threads of a score block
static_assert(T == NMOD * NSEG && C * 64 == 1024, "lane layouts");

struct Chan {
  double br, th, inv_g;  // p = exp(br + i th); 1 / g
};
struct Mod {
  double b0, na1, na2;  // B0 / a0, -a1 / a0, -a2 / a0
  double M[NLEV][4];    // A^(128 2^l), A = [[na1, na2], [1, 0]], row-major
};
constexpr int MODD = (int)(sizeof(Mod) / sizeof(double));
static_assert(sizeof(Mod) == (3 + 4 * NLEV) * sizeof(double) && 3 + 4 * NLEV <= NSEG, "a lane per constant");
struct Params {
  Chan ch[NCH];
  Mod mod[NMOD];
};
struct ScoreParams {
  double erb[NCH];  // ERB(cf_i), i = 1 .. 23
  double L[NMOD];   // lower band edges of the modulation filters
};

struct cf2 {
  float r, i;
};
__device__ __forceinline__ cf2 cfma(cf2 a, cf2 b, cf2 c) {  // a b + c
  return {fmaf(a.r, b.r, fmaf(-a.i, b.i, c.r)), fmaf(a.r, b.i, fmaf(a.i, b.r, c.i))};
}
__device__ __forceinline__ cf2 cshfl_up(cf2 v, int d) { return {__shfl_up(v.r, d, 64), __shfl_up(v.i, d, 64)}; }
__device__ __forceinline__ cf2 cshfl_down(cf2 v, int d) { return {__shfl_down(v.r, d, 64), __shfl_down(v.i, d, 64)}; }
__device__ __forceinline__ cf2 cconj(cf2 v) { return {v.r, -v.i}; }
// scale p^k, in double, rounded once
__device__ __forceinline__ cf2 cpow(const Chan &c, double k, double scale) {
  const double m = exp(k * c.br) * scale;
  double s, co;
  sincos(k * c.th, &s, &co);
  return {(float)(m * co), (float)(m * s)};
}

__device__ __forceinline__ int pad(int m) { return m + (m >> 7); }

// The gammatone constants of a channel (the same in every lane but PL).
struct Gamma {
  cf2 p, c1, c2, c3;  // the pole; the numerator's taps p / g, 4 p^2 / g, p^3 / g
  cf2 Q[6], Q6, PL;   // p^(16 2^l), p^1024, p^(16 lane) (lane 0: exactly 1)
  Chan chf;           // the float32 pole in polar form
};
__device__ __forceinline__ Gamma gamma_of(const Chan &ch, int lane) {
  Gamma G;
  G.p = cpow(ch, 1.0, 1.0);
  G.c1 = cpow(ch, 1.0, ch.inv_g), G.c2 = cpow(ch, 2.0, 4.0 * ch.inv_g), G.c3 = cpow(ch, 3.0, ch.inv_g);
  // the scans' p^k are powers of the float32 pole the recurrences multiply by, not of the exact one
  // (a pole's rounding moves a channel's gain by parts in 1e5: both halves of a scan must share it)
  G.chf = {0.5 * log((double)G.p.r * G.p.r + (double)G.p.i * G.p.i), atan2((double)G.p.i, (double)G.p.r), 0.0};
#pragma unroll
  for (int l = 0; l < 6; ++l) G.Q[l] = cpow(G.chf, (double)(C << l), 1.0);
  G.Q6 = cpow(G.chf, (double)(C * 64), 1.0);
  G.PL = cpow(G.chf, (double)(C * lane), 1.0);
  return G;
}

// The gammatone over a tile: x[j] = sample c0 + j - 3 of the lane's 16 (c0 = 16 tid); v[j] = y at
// sample c0 + j.  The three-tap numerator, then the four recurrences s[t] = p s[t - 1] + in[t], each a
// chunked scan: the lane's 16 steps from a zero state (the tile's first lane: from the carried state
// Tc), an inclusive scan of the lanes' end states, the four waves' totals through `wt`, the 16 steps
// again from the true state.  Tc becomes the state at the tile's end.  One barrier per stage.
__device__ __forceinline__ void gammatone_tile(const Gamma &G, const float (&x)[C + 3], cf2 (&v)[C], cf2 (&Tc)[4],
                                               cf2 (*wt)[4], int tid, int lane, int wave) {
  const cf2 p = G.p;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    v[j].r = fmaf(G.c1.r, x[j + 2], fmaf(G.c2.r, x[j + 1], G.c3.r * x[j]));
    v[j].i = fmaf(G.c1.i, x[j + 2], fmaf(G.c2.i, x[j + 1], G.c3.i * x[j]));
  }
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    const cf2 zero = {0.f, 0.f};
    cf2 c = tid == 0 ? Tc[st] : zero;  // (the tile's first lane starts from the carried state)
#pragma unroll
    for (int j = 0; j < C; ++j) c = cfma(p, c, v[j]);
#pragma unroll
    for (int l = 0; l < 6; ++l) {
      const cf2 u = cshfl_up(c, 1 << l);
      if (lane >= (1 << l)) c = cfma(G.Q[l], u, c);
    }
    if (lane == 63) wt[st][wave] = c;
    cf2 ex = cshfl_up(c, 1);
    if (lane == 0) ex = zero;
    __syncthreads();
    const cf2 t0 = wt[st][0], t1 = wt[st][1], t2 = wt[st][2], t3 = wt[st][3];
    const cf2 cw1 = t0, cw2 = cfma(G.Q6, cw1, t1), cw3 = cfma(G.Q6, cw2, t2);
    const cf2 cw = wave == 0 ? zero : wave == 1 ? cw1 : wave == 2 ? cw2 : cw3;
    cf2 cin = cfma(G.PL, cw, ex);
    if (tid == 0) cin = Tc[st];
    Tc[st] = cfma(G.Q6, cw3, t3);
    c = cin;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      c = cfma(p, c, v[j]);
      v[j] = c;
    }
  }
}

// Modulation filter of constants mc (a Mod as doubles) over segment s of the tile's envelope in `buf`
// (the segment at buf[sb ...]; eb2, eb1 = e[t - 2], e[t - 1] at its start): the lane runs its biquad from
// a zero state (segment 0: from the carried state (Z1, Z2) = (m[t - 1], m[t - 2]) at the tile's start),
// the end states are scanned over the 32 segments with the matrices A^(128 2^l).  (i1, i2): the true
// state at the segment's start; (Z1, Z2) becomes the state at the tile's end.
__device__ __forceinline__ void mod_scan(const float *buf, int sb, int s, const double *__restrict__ mc, double eb1,
                                         double eb2, double &Z1, double &Z2, double &i1, double &i2) {
  const double b0 = mc[0], na1 = mc[1], na2 = mc[2];
  double y1 = s ? 0.0 : Z1, y2 = s ? 0.0 : Z2, e1 = eb1, e2 = eb2;
#pragma unroll 8
  for (int j = 0; j < SEG; ++j) {
    const double e0 = (double)buf[sb + j];
    const double y = fma(na1, y1, fma(na2, y2, b0 * (e0 - e2)));
    y2 = y1, y1 = y, e2 = e1, e1 = e0;
  }
#pragma unroll
  for (int l = 0; l < NLEV; ++l) {
    const double u1 = __shfl_up(y1, 1 << l, 32), u2 = __shfl_up(y2, 1 << l, 32);
    if (s >= (1 << l)) {
      const double *__restrict__ M = mc + 3 + 4 * l;
      y1 += fma(M[0], u1, M[1] * u2);
      y2 += fma(M[2], u1, M[3] * u2);
    }
  }
  i1 = __shfl_up(y1, 1, 32), i2 = __shfl_up(y2, 1, 32);
  if (s == 0) i1 = Z1, i2 = Z2;
  Z1 = __shfl(y1, 31, 32), Z2 = __shfl(y2, 31, 32);  // the state at the tile's end
}

// The filters of one sample rate, in double on the host.
inline void make_params(int sr, Params *P, ScoreParams *S) {
  const double pi = 3.14159265358979323846, fs = (double)sr;
  const double EarQ = 9.26449, minBW = 24.7, c = EarQ * minBW;
  for (int i = 1; i <= NCH; ++i) {
    const double cf = -c + exp(i * (log(125.0 + c) - log(fs / 2 + c)) / NCH) * (fs / 2 + c);
    const double erb = cf / EarQ + minBW;
    Chan &ch = P->ch[i - 1];
    ch.br = -2.0 * pi * 1.019 * erb / fs;
    ch.th = 2.0 * pi * cf / fs;
    const std::complex<double> zi = std::polar(1.0, -ch.th);  // 1 / z0
    std::complex<double> G[2];
    for (int q = 0; q < 2; ++q) {
      const std::complex<double> u = std::polar(exp(ch.br), q ? -ch.th : ch.th) * zi;  // p / z0
      const std::complex<double> d = (1.0 - u) * (1.0 - u);
      G[q] = u * (1.0 + 4.0 * u + u * u) / (d * d);
    }
    ch.inv_g = 2.0 / std::abs(G[0] + G[1]);
    S->erb[i - 1] = erb;
  }
  for (int k = 0; k < NMOD; ++k) {
    const double mcf = 4.0 * pow(32.0, k / 7.0);
    const double W0 = tan(pi * mcf / fs), B0 = W0 / 2.0;
    const double a0 = 1.0 + B0 + W0 * W0;
    Mod &m = P->mod[k];
    m.b0 = B0 / a0;
    m.na1 = -(2.0 * W0 * W0 - 2.0) / a0;
    m.na2 = -(1.0 - B0 + W0 * W0) / a0;
    long double a[4] = {m.na1, m.na2, 1.0L, 0.0L};
    auto square = [&]() {
      const long double r[4] = {a[0] * a[0] + a[1] * a[2], a[0] * a[1] + a[1] * a[3], a[2] * a[0] + a[3] * a[2],
                                a[2] * a[1] + a[3] * a[3]};
      for (int q = 0; q < 4; ++q) a[q] = r[q];
    };
    for (int q = 1; q < SEG; q <<= 1) square();  // A^128
    for (int l = 0; l < NLEV; ++l) {
      for (int q = 0; q < 4; ++q) m.M[l][q] = (double)a[q];
      square();
    }
    S->L[k] = mcf - B0 * fs / (2.0 * pi);
  }
}

// K* of a row's energies A [23][8]: the 90 % bandwidth rule (include/fsem.h "SRMR", Score).
__device__ __forceinline__ int bandwidth_mods(const double *__restrict__ A, const ScoreParams &S) {
  double ac[NCH], total = 0.0;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    double a = A[i * NMOD];
#pragma unroll
    for (int k = 1; k < NMOD; ++k) a += A[i * NMOD + k];
    ac[i] = a;
    total += a;
  }
  // upward in frequency (i = 23 first) to the first channel at which the share exceeds 90 %
  double cum = 0.0, bw = S.erb[0];
  bool found = false;
#pragma unroll
  for (int i = NCH - 1; i >= 0; --i) {
    cum += 100.0 * ac[i] / total;
    if (!found && cum > 90.0) {
      found = true;
      bw = S.erb[i];
    }
  }
  return bw > S.L[7] ? 8 : bw > S.L[6] ? 7 : bw > S.L[5] ? 6 : 5;
}

// K*, and the ratio's numerator N and denominator D: SRMR = N / D.
__device__ __forceinline__ int score_terms(const double *__restrict__ A, const ScoreParams &S, double &num,
                                           double &den) {
  const int K = bandwidth_mods(A, S);
  num = 0.0, den = 0.0;
  for (int i = 0; i < NCH; ++i) {
    for (int k = 0; k < 4; ++k) num += A[i * NMOD + k];
    for (int k = 4; k < K; ++k) den += A[i * NMOD + k];
  }
  return K;
}

}  // namespace srmr
}  // namespace fsem
