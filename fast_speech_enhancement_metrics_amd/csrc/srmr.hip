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
#include "fsem_srmr_kernels.h"

namespace fsem {
namespace srmr {

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
  const Gamma G = gamma_of(P.ch[chn], lane);
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
    gammatone_tile(G, x, v, Tc, wt, tid, lane, wave);
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
    double y1, y2, e1 = eb1, e2 = eb2;
    mod_scan(buf, sb, s, mc, eb1, eb2, Z1, Z2, y1, y2);
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
  double num, den;
  score_terms(A, S, num, den);
  srmr[row] = (float)(num / den);  // (a digitally silent row: 0 / 0)
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
