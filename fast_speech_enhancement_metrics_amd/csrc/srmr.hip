// SRMR, the speech-to-reverberation modulation energy ratio of a row (include/fsem.h "SRMR").
// Replaces nothing in the reference.  Two kernels, no workspace: the caller's `energies` is the
// only intermediate.
//
//   srmr_energies  grid (channel, row), 4 waves.  The block walks its row in tiles of TILE = 4096
//                  samples staged in LDS, carrying every filter's state from tile to tile.
//                    - Analytic gammatone, float32 complex, ONE LANE PER 16 SAMPLES: the three-tap
//                      numerator, then four first-order recurrences s[t] = p s[t - 1] + in[t], each
//                      a chunked scan -- the lane's 16 steps from a zero state, an inclusive scan of
//                      the lanes' end states (shuffles with p^(16 2^l), the four waves' totals
//                      through LDS with p^1024), the 16 steps again from the true state.  The
//                      envelope |y| goes back to LDS as float32.
//                    - Modulation filters, double, ONE LANE PER (filter, 128-sample segment): a
//                      wave holds two filters x 32 segments, so a filter's scan never leaves its
//                      half wave.  The lane runs its biquad from a zero state (lane 0: from the
//                      previous tile's end state), the end states (y[t], y[t - 1]) are scanned with
//                      the 2 x 2 matrices A^(128 2^l), and the lane runs the segment again from the
//                      true state, adding m^2 V[t] in sample order in double.
//                    - V[t] = sum_f w^2[t - f wi] from the squared window in LDS; where all four
//                      frames cover a segment, from their sum W4[t mod wi].  Frame bounds are
//                      multiples of 128, so a segment has one frame set.
//                    - At the end the 32 lanes of a filter add their sums in a fixed butterfly.
//   srmr_scores    one block per row: scans the row's n samples for a non-finite one, then one
//                  thread applies the 90 % bandwidth rule and the ratio to energies[row].
//
// Every sum has one order, fixed by the sample rate and the row's own length alone.
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
// scale p^k, in double, rounded once
__device__ __forceinline__ cf2 cpow(const Chan &c, double k, double scale) {
  const double m = exp(k * c.br) * scale;
  double s, co;
  sincos(k * c.th, &s, &co);
  return {(float)(m * co), (float)(m * s)};
}

__device__ __forceinline__ int pad(int m) { return m + (m >> 7); }

template <bool WIDE>
__global__ __launch_bounds__(T) void srmr_energies(const float *__restrict__ deg, int64_t ld,
                                                   const int32_t *__restrict__ lengths, int length, int64_t r0,
                                                   const Params P, double *__restrict__ energies) {
  constexpr int wl = WIDE ? 4096 : 2048, wi = wl / 4, HW = wl / 2;
  static_assert(wi % SEG == 0 && TILE % wi == 0, "a segment has one frame set");
  __shared__ float buf[NSEG * SEGP];                // the tile's samples, then its envelope (padded)
  __shared__ double w2[HW + (HW >> 7) + 1];         // w^2[m], m <= wl / 2 (w[m] = w[wl - m]), padded
  __shared__ double w4[wi + (wi >> 7)];             // sum of the four frames' w^2 at t mod wi, padded
  __shared__ float xh[2][3], eh[2][2];              // the previous tile's last samples, by tile parity
  __shared__ cf2 wt[4][4];                          // [stage][wave] end states
  __shared__ double modc[NMOD][sizeof(Mod) / sizeof(double)];  // the modulation filters' constants
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chn = blockIdx.x;
  const int64_t row = r0 + blockIdx.y;
  const int n = row_length(lengths, row, length);
  const int F = n >= wl ? (n - wl) / wi + 1 : 0;
  double *__restrict__ out = energies + (row * NCH + chn) * NMOD;
  if (F == 0) {  // (block-uniform, before any barrier)
    if (tid < NMOD) out[tid] = __builtin_nan("");
    return;
  }
  const int nend = (F - 1) * wi + wl;  // the frames cover [0, nend), nend <= n
  const int ntile = (nend + TILE - 1) / TILE;
  const float *__restrict__ xrow = deg + row * ld;

  for (int m = tid; m <= HW; m += T) {
    const double w = 0.54 - 0.46 * cospi((double)m / (double)HW);
    w2[pad(m)] = w * w;
  }
  if (tid < 3) xh[0][tid] = 0.f;
  if (tid < 2) eh[0][tid] = 0.f;
  __syncthreads();
  auto W2 = [&](int m) -> double { return w2[pad(m <= HW ? m : wl - m)]; };
  for (int r = tid; r < wi; r += T) w4[pad(r)] = ((W2(r + 3 * wi) + W2(r + 2 * wi)) + W2(r + wi)) + W2(r);

  // gammatone constants (the same in every lane but PL)
  const Chan ch = P.ch[chn];
  const cf2 p = cpow(ch, 1.0, 1.0);
  const cf2 c1 = cpow(ch, 1.0, ch.inv_g), c2 = cpow(ch, 2.0, 4.0 * ch.inv_g), c3 = cpow(ch, 3.0, ch.inv_g);
  // the scans' p^k are powers of the float32 pole the recurrences multiply by, not of the exact one
  // (a pole's rounding moves a channel's gain by parts in 1e5: both halves of a scan must share it)
  const Chan chf = {0.5 * log((double)p.r * p.r + (double)p.i * p.i), atan2((double)p.i, (double)p.r), 0.0};
  cf2 Q[6];
#pragma unroll
  for (int l = 0; l < 6; ++l) Q[l] = cpow(chf, (double)(C << l), 1.0);
  const cf2 Q6 = cpow(chf, (double)(C * 64), 1.0);
  const cf2 PL = cpow(chf, (double)(C * lane), 1.0);  // (lane 0: exactly 1)
  cf2 Tc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};  // the stages' states at the tile's start

  // modulation filter of this lane; its constants wait in LDS while the gammatone has the registers
  const int k = tid >> 5, s = tid & 31;
  if (s < (int)(sizeof(Mod) / sizeof(double))) modc[k][s] = reinterpret_cast<const double *>(&P.mod[k])[s];
  double Z1 = 0.0, Z2 = 0.0;  // (y[t], y[t - 1]) at the tile's start
  double acc = 0.0;
  const int sb = s * SEGP;

  for (int tile = 0; tile < ntile; ++tile) {
    const int base = tile * TILE, par = tile & 1;
    for (int i = tid; i < TILE; i += T) {
      const int g = base + i;
      buf[i] = g < n ? xrow[g] : 0.f;
    }
    __syncthreads();
    // ---- gammatone: samples c0 .. c0 + 15 of the tile
    const int c0 = tid * C;
    float x[C + 3];  // x[j] = sample c0 + j - 3
#pragma unroll
    for (int j = 0; j < C + 3; ++j) x[j] = (c0 + j >= 3) ? buf[c0 + j - 3] : xh[par][j];
    if (tid == T - 1) {
      xh[par ^ 1][0] = x[C];
      xh[par ^ 1][1] = x[C + 1];
      xh[par ^ 1][2] = x[C + 2];
    }
    __syncthreads();  // (the envelope overwrites the samples)
    cf2 v[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      v[j].r = fmaf(c1.r, x[j + 2], fmaf(c2.r, x[j + 1], c3.r * x[j]));
      v[j].i = fmaf(c1.i, x[j + 2], fmaf(c2.i, x[j + 1], c3.i * x[j]));
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
        if (lane >= (1 << l)) c = cfma(Q[l], u, c);
      }
      if (lane == 63) wt[st][wave] = c;
      cf2 ex = cshfl_up(c, 1);
      if (lane == 0) ex = zero;
      __syncthreads();
      const cf2 t0 = wt[st][0], t1 = wt[st][1], t2 = wt[st][2], t3 = wt[st][3];
      const cf2 cw1 = t0, cw2 = cfma(Q6, cw1, t1), cw3 = cfma(Q6, cw2, t2);
      const cf2 cw = wave == 0 ? zero : wave == 1 ? cw1 : wave == 2 ? cw2 : cw3;
      cf2 cin = cfma(PL, cw, ex);
      if (tid == 0) cin = Tc[st];
      Tc[st] = cfma(Q6, cw3, t3);
      c = cin;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        c = cfma(p, c, v[j]);
        v[j] = c;
      }
    }
    float e14 = 0.f, e15 = 0.f;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const float e = sqrtf(fmaf(v[j].r, v[j].r, v[j].i * v[j].i));
      buf[pad(c0 + j)] = e;
      if (j == C - 2) e14 = e;
      if (j == C - 1) e15 = e;
    }
    if (tid == T - 1) {
      eh[par ^ 1][0] = e14;
      eh[par ^ 1][1] = e15;
    }
    __syncthreads();
    // ---- modulation filter k over segment s
    int kk = k;
    asm volatile("" : "+v"(kk));  // (read the constants here, in every tile: not kept across the gammatone)
    const double *__restrict__ mc = modc[kk];
    const double b0 = mc[0], na1 = mc[1], na2 = mc[2];
    const double eb2 = s ? (double)buf[sb - 3] : (double)eh[par][0];  // e[t - 2], e[t - 1] at the segment's start
    const double eb1 = s ? (double)buf[sb - 2] : (double)eh[par][1];
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
    double i1 = __shfl_up(y1, 1, 32), i2 = __shfl_up(y2, 1, 32);
    if (s == 0) i1 = Z1, i2 = Z2;
    Z1 = __shfl(y1, 31, 32), Z2 = __shfl(y2, 31, 32);  // the state at the tile's end
    y1 = i1, y2 = i2, e1 = eb1, e2 = eb2;
    const int ts = base + s * SEG;
    const int f_lo = ts < wl ? 0 : (ts - wl) / wi + 1, f_hi = min(F - 1, ts / wi);
    if (f_hi - f_lo == 3) {
      const double *__restrict__ wv = w4 + pad(ts % wi);
#pragma unroll 8
      for (int j = 0; j < SEG; ++j) {
        const double e0 = (double)buf[sb + j];
        const double y = fma(na1, y1, fma(na2, y2, b0 * (e0 - e2)));
        y2 = y1, y1 = y, e2 = e1, e1 = e0;
        acc = fma(y * y, wv[j], acc);
      }
    } else if (f_hi >= f_lo) {
      for (int j = 0; j < SEG; ++j) {
        const double e0 = (double)buf[sb + j];
        const double y = fma(na1, y1, fma(na2, y2, b0 * (e0 - e2)));
        y2 = y1, y1 = y, e2 = e1, e1 = e0;
        double V = 0.0;
        for (int f = f_lo; f <= f_hi; ++f) V += W2(ts + j - f * wi);
        acc = fma(y * y, V, acc);
      }
    }
    __syncthreads();  // (the next tile overwrites the envelope)
  }
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 32);
  if (s == 0) out[k] = acc / (double)F;
}

__global__ __launch_bounds__(RT) void srmr_scores(const float *__restrict__ deg, int64_t ld,
                                                  const int32_t *__restrict__ lengths, int length, int64_t batch,
                                                  int wl, int wi, const ScoreParams S,
                                                  const double *__restrict__ energies, float *__restrict__ srmr) {
  const int tid = threadIdx.x;
  const int64_t row = grid_row_xy();
  if (row >= batch) return;
  const int n = row_length(lengths, row, length);
  const int F = n >= wl ? (n - wl) / wi + 1 : 0;
  const float *__restrict__ xrow = deg + row * ld;
  int bad = 0;
  if (F > 0)  // (a row without a frame is NaN whatever it holds)
    for (int i = tid; i < n; i += RT) bad |= !isfinite(xrow[i]);
  bad = __syncthreads_or(bad);
  if (tid != 0) return;
  if (F == 0 || bad) {
    srmr[row] = __builtin_nanf("");
    return;
  }
  const double *__restrict__ A = energies + row * NCH * NMOD;
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
  const int K = bw > S.L[7] ? 8 : bw > S.L[6] ? 7 : bw > S.L[5] ? 6 : 5;
  double num = 0.0, den = 0.0;
  for (int i = 0; i < NCH; ++i) {
    for (int k = 0; k < 4; ++k) num += A[i * NMOD + k];
    for (int k = 4; k < K; ++k) den += A[i * NMOD + k];
  }
  srmr[row] = (float)(num / den);  // (a digitally silent row: 0 / 0)
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

}  // namespace srmr
}  // namespace fsem

using namespace fsem;

extern "C" int fsem_srmr_channels(int32_t sample_rate) {
  return sample_rate == 8000 || sample_rate == 16000 ? srmr::NCH : 0;
}

extern "C" int fsem_srmr_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                             int32_t sample_rate, double *energies, float *srmr_out, void *stream) {
  if (!deg || !energies || !srmr_out || batch < 0 || length < 0 || ld < length || length > kMaxLength)
    return FSEM_EINVAL;
  if (!fsem_srmr_channels(sample_rate)) return FSEM_ERATE;
  if (batch == 0) return FSEM_OK;  // (nothing to score)
  srmr::Params P;
  srmr::ScoreParams S;
  srmr::make_params(sample_rate, &P, &S);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = sample_rate == 16000;
  // (rows without a frame, length == 0 included: the block writes NaN energies and reads no sample)
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice(srmr::NCH, batch, r0);
    if (wide)
      hipLaunchKernelGGL(srmr::srmr_energies<true>, grid, dim3(srmr::T), 0, st, deg, ld, lengths, (int)length, r0, P,
                         energies);
    else
      hipLaunchKernelGGL(srmr::srmr_energies<false>, grid, dim3(srmr::T), 0, st, deg, ld, lengths, (int)length, r0, P,
                         energies);
    FSEM_CHECK_LAUNCH();
  }
  const int wl = wide ? 4096 : 2048;
  hipLaunchKernelGGL(srmr::srmr_scores, grid_xy(batch), dim3(srmr::RT), 0, st, deg, ld, lengths, (int)length, batch, wl,
                     wl / 4, S, energies, srmr_out);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}
