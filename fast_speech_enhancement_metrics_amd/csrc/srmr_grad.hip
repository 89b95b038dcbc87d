// Gradient of SRMR with respect to the rows (include/fsem.h, "SRMR with gradients"; the forward:
// srmr.hip).  Time runs backwards: the forward recurrences are stable only forwards, so the adjoint
// cannot invert them; it recomputes them from checkpoints.  Three kernels; the last two run in passes
// of fsem_srmrgrad_pass_rows(length) rows so that the scratch stays bounded.
//
//   srmr_grad_rows    one block per row: scans the row's n samples for a non-finite one, then one thread
//                     takes K*, N and D from the forward's energies (the forward's own code,
//                     fsem_srmr_kernels.h) and writes the row's eight coefficients 2 c_k / F; a row
//                     without a frame, with a non-finite sample or score or with a zero incoming gradient
//                     is marked dead: nothing below reads it, its gradient row is written as zeros.
//   srmr_grad_planes  grid (channel, row of the pass), 4 waves, the forward's lane layouts.
//                     Sweep 1, tiles first to last: the forward's gammatone and the first half of its
//                     modulation scan (the shared bodies), storing at each tile's start the state that
//                     enters it (Ckpt: four complex gammatone states, the 3-sample and 2-envelope halos,
//                     8 x 2 biquad states; 184 bytes per (row, channel, tile)).  A thread reads back only
//                     what it wrote itself.
//                     Sweep 2, tiles last to first, from the tile's checkpoint:
//                       - the forward again: y in registers (16 complex per lane), |y| in LDS, each
//                         (filter, segment) lane's true state at its segment's start;
//                       - the lane runs its 128 samples forwards once more, keeping the state at every
//                         16th sample (8 sub-segments);
//                       - pass A, sub-segments last to first: 16 values of m recomputed into registers,
//                         then r[t] = q[t] - a1 r[t + 1] - a2 r[t + 2] over them, from a zero state (the
//                         tile's last segment: from the carried (r[t + 1], r[t + 2]));
//                       - the states (r[t], r[t + 1]) at the segments' starts are scanned from the last
//                         lane down.  Backwards in time that pair obeys the forward's own matrix
//                         A = [[-a1, -a2], [1, 0]], so the scan multiplies by the forward's A^(128 2^l);
//                       - pass B, a round per sub-segment, last first: m again, r from the true state,
//                         b0 (r[t] - r[t + 2]) of a wave's two filters added by one exchange and stored,
//                         then the four waves' values added in wave order and rounded to float32 over the
//                         envelope, which no later round reads.  The sum over k is ((0 + 1) + (2 + 3) +
//                         (4 + 5)) + (6 + 7), grouped as written;
//                       - a0 = de y / |y| (0 where |y| = 0), the four adjoint stages with conj(p) as the
//                         forward's chunked scan mirrored (the last lane takes the carried state, the
//                         lanes' states are scanned downwards with conj(p)^(16 2^l), the waves' totals
//                         with conj(p)^1024), the three taps on a4[t + 1 .. t + 3] with the next lane's
//                         first three values through LDS (the tile's last lane: the later tile's).
//                       - the channel's dx of the tile goes to its plane in scratch, float32.
//                     Carried to the tile before: 8 x (r[t + 1], r[t + 2]), the four stages, three a4.
//   srmr_grad_reduce  four samples per thread: the 23 planes added in channel order in double, rounded
//                     once; zeros from nend - 1 on, past the row's length and for a dead row.
//
// Every sum has one order, fixed by the sample rate and the row's own length; a row's blocks read and
// write only that row's scratch: its gradient does not depend on the pass size, the batch size, the
// row's position, `length`, `ld` or the stream.  No floating-point atomics.
#include "fsem_srmr_kernels.h"

namespace fsem {
namespace srmr {

constexpr int SUB = 16;          // samples of a sub-segment
constexpr int NSUB = SEG / SUB;  // 8 per segment
constexpr int SUBP = SUB + 1;    // its LDS stride in the rounds' exchange area
constexpr int64_t kPassBytes = int64_t(2) << 30;  // the planes and checkpoints of a pass stay below this

// The filters' state at a tile's start.
struct Ckpt {
  double Z[NMOD][2];  // (m[t - 1], m[t - 2])
  cf2 Tc[4];          // the gammatone stages
  float xh[3], eh[2], unused;
};
static_assert(sizeof(Ckpt) == 184, "the checkpoint's size (include/fsem.h)");

struct RowC {
  double c[NMOD];  // 2 c_k / F
  int32_t live, unused;
};

__global__ __launch_bounds__(RT) void srmr_grad_rows(const float *__restrict__ deg, int64_t ld,
                                                     const int32_t *__restrict__ lengths, int length, int64_t batch,
                                                     int wl, int wi, const ScoreParams S,
                                                     const double *__restrict__ energies,
                                                     const float *__restrict__ gout, RowC *__restrict__ rowc) {
  const int tid = threadIdx.x;
  const int64_t row = grid_row_xy();
  if (row >= batch) return;
  const int n = row_length(lengths, row, length);
  const int F = n >= wl ? (n - wl) / wi + 1 : 0;
  const float *__restrict__ xrow = deg + row * ld;
  int bad = 0;
  if (F > 0)
    for (int i = tid; i < n; i += RT) bad |= !isfinite(xrow[i]);
  bad = __syncthreads_or(bad);
  if (tid != 0) return;
  RowC rc;
  for (int k = 0; k < NMOD; ++k) rc.c[k] = 0.0;
  rc.live = 0, rc.unused = 0;
  const double G = (double)gout[row];
  if (F > 0 && !bad && G != 0.0) {
    double num, den;
    const int K = score_terms(energies + row * NCH * NMOD, S, num, den);
    if (isfinite((float)(num / den))) {
      const double lo = G / den, hi = -G * num / (den * den);
      for (int k = 0; k < NMOD; ++k) rc.c[k] = k < 4 ? 2.0 * lo / (double)F : k < K ? 2.0 * hi / (double)F : 0.0;
      rc.live = 1;
    }
  }
  rowc[row] = rc;
}

// Two waves per SIMD: what the block's LDS allows (two blocks per CU).  Uncapped the compiler takes 436 VGPRs
// and 180 AGPRs, one wave per SIMD, and the call is 6 % slower.
template <bool WIDE>
__global__ __launch_bounds__(T, 2) void srmr_grad_planes(const float *__restrict__ deg, int64_t ld,
                                                      const int32_t *__restrict__ lengths, int length, int64_t r0,
                                                      const Params P, const RowC *__restrict__ rowc, Ckpt *ckpt,
                                                      int ntmax, float *__restrict__ planes, int64_t pstride) {
  constexpr int wl = WIDE ? 4096 : 2048, wi = wl / 4, HW = wl / 2;
  static_assert(wi % SEG == 0 && TILE % wi == 0 && SEG % SUB == 0, "a segment has one frame set");
  __shared__ float buf[NSEG * SEGP];         // the tile's samples, then its envelope, then de (padded)
  __shared__ double w2[HW + (HW >> 7) + 1];  // w^2[m], m <= wl / 2 (w[m] = w[wl - m]), padded
  __shared__ double w4[wi + (wi >> 7)];      // sum of the four frames' w^2 at t mod wi, padded
  __shared__ float xh[2][3], eh[2][2];       // the previous tile's last samples, by tile parity
  __shared__ cf2 wt[4][4];                   // [stage][wave] end states
  __shared__ double modc[NMOD][MODD];        // the modulation filters' constants
  __shared__ double dsum[4][NSEG][SUBP];     // a round's b0 (r[t] - r[t + 2]) per wave; then the lanes' first a4
  __shared__ cf2 ahn[3];                     // a4 at the later tile's first three samples
  static_assert(sizeof(dsum) >= T * 3 * sizeof(cf2), "the a4 halos fit the exchange area");
  cf2(*ah)[3] = reinterpret_cast<cf2(*)[3]>(&dsum[0][0][0]);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chn = blockIdx.x;
  const int64_t lr = blockIdx.y, row = r0 + lr;
  const int n = row_length(lengths, row, length);
  const int F = n >= wl ? (n - wl) / wi + 1 : 0;
  if (F == 0 || !rowc[row].live) return;  // (block-uniform, before any barrier)
  const int nend = (F - 1) * wi + wl;     // the frames cover [0, nend), nend <= n
  const int ntile = (nend + TILE - 1) / TILE;  // <= ntmax
  const float *__restrict__ xrow = deg + row * ld;
  Ckpt *ck0 = ckpt + (lr * NCH + chn) * ntmax;
  float *__restrict__ plane = planes + (lr * NCH + chn) * pstride;

  for (int m = tid; m <= HW; m += T) {
    const double w = 0.54 - 0.46 * cospi((double)m / (double)HW);
    w2[pad(m)] = w * w;
  }
  if (tid < 3) {
    xh[0][tid] = 0.f;
    ahn[tid] = {0.f, 0.f};
  }
  if (tid < 2) eh[0][tid] = 0.f;
  __syncthreads();
  auto W2 = [&](int m) -> double { return w2[pad(m <= HW ? m : wl - m)]; };
  for (int r = tid; r < wi; r += T) w4[pad(r)] = ((W2(r + 3 * wi) + W2(r + 2 * wi)) + W2(r + wi)) + W2(r);

  const Gamma G = gamma_of(P.ch[chn], lane);
  cf2 Tc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};  // the stages' states at the tile's start

  const int k = tid >> 5, s = tid & 31;
  if (s < MODD) modc[k][s] = reinterpret_cast<const double *>(&P.mod[k])[s];
  double Z1 = 0.0, Z2 = 0.0;  // (m[t - 1], m[t - 2]) at the tile's start
  const int sb = s * SEGP;
  const int c0 = tid * C;

  // The forward over the tile at `base` from the state in Tc, xh[par], eh[par] and (Z1, Z2): v = y of the
  // lane's 16 samples, the envelope in buf, (eb1, eb2) = e[t - 1], e[t - 2] and (i1, i2) = m[t - 1], m[t - 2]
  // at the start of the lane's segment; the state becomes that at the tile's end (halos: parity par ^ 1).
  auto tile_forward = [&](int base, int par, cf2(&v)[C], const double *__restrict__ &mc, double &eb1, double &eb2,
                          double &i1, double &i2) {
    for (int i = tid; i < TILE; i += T) {
      const int g = base + i;
      buf[i] = g < n ? xrow[g] : 0.f;
    }
    __syncthreads();
    float x[C + 3];  // x[j] = sample c0 + j - 3
#pragma unroll
    for (int j = 0; j < C + 3; ++j) x[j] = (c0 + j >= 3) ? buf[c0 + j - 3] : xh[par][j];
    if (tid == T - 1) {
      xh[par ^ 1][0] = x[C];
      xh[par ^ 1][1] = x[C + 1];
      xh[par ^ 1][2] = x[C + 2];
    }
    __syncthreads();  // (the envelope overwrites the samples)
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
    int kk = k;
    asm volatile("" : "+v"(kk));  // (read the constants here, in every tile: not kept across the gammatone)
    mc = modc[kk];
    eb2 = s ? (double)buf[sb - 3] : (double)eh[par][0];
    eb1 = s ? (double)buf[sb - 2] : (double)eh[par][1];
    mod_scan(buf, sb, s, mc, eb1, eb2, Z1, Z2, i1, i2);
  };

  // ---- sweep 1: the state that enters every tile
  for (int tile = 0; tile < ntile; ++tile) {
    const int par = tile & 1;
    Ckpt *ck = ck0 + tile;
    if (tid == 0) {
#pragma unroll
      for (int st = 0; st < 4; ++st) ck->Tc[st] = Tc[st];
      ck->xh[0] = xh[par][0], ck->xh[1] = xh[par][1], ck->xh[2] = xh[par][2];
      ck->eh[0] = eh[par][0], ck->eh[1] = eh[par][1];
    }
    if (s == 0) ck->Z[k][0] = Z1, ck->Z[k][1] = Z2;
    if (tile == ntile - 1) break;  // (block-uniform)
    cf2 v[C];
    const double *__restrict__ mc;
    double eb1, eb2, i1, i2;
    tile_forward(tile * TILE, par, v, mc, eb1, eb2, i1, i2);
    __syncthreads();  // (the next tile overwrites the envelope)
  }

  // ---- sweep 2: the adjoint, tiles last to first
  const double coef = rowc[row].c[k];
  const cf2 pc = cconj(G.p);
  cf2 Qc[6];
#pragma unroll
  for (int l = 0; l < 6; ++l) Qc[l] = cconj(G.Q[l]);
  const cf2 Q6c = cconj(G.Q6);
  const cf2 PLr = cconj(cpow(G.chf, (double)(C * (63 - lane)), 1.0));  // (lane 63: exactly 1)
  const cf2 zero = {0.f, 0.f};
  cf2 Ta[4] = {zero, zero, zero, zero};  // the adjoint stages at the later tile's first sample
  double Rc1 = 0.0, Rc2 = 0.0;           // (r[t], r[t + 1]) at the later tile's first sample

  for (int tile = ntile - 1; tile >= 0; --tile) {
    const int base = tile * TILE;
    const Ckpt *ck = ck0 + tile;
    __syncthreads();  // (the tile before this one in the sweep has left buf, xh and eh)
    if (tid == 0) {
#pragma unroll
      for (int st = 0; st < 4; ++st) Tc[st] = ck->Tc[st];
      xh[0][0] = ck->xh[0], xh[0][1] = ck->xh[1], xh[0][2] = ck->xh[2];
      eh[0][0] = ck->eh[0], eh[0][1] = ck->eh[1];
    }
    if (s == 0) Z1 = ck->Z[k][0], Z2 = ck->Z[k][1];
    __syncthreads();
    cf2 v[C];
    const double *__restrict__ mc;
    double eb1, eb2, i1, i2;
    tile_forward(base, 0, v, mc, eb1, eb2, i1, i2);

    // ---- modulation filter k over segment s, and its adjoint
    const double b0 = mc[0], na1 = mc[1], na2 = mc[2];
    const int ts = base + s * SEG;
    const int f_lo = ts < wl ? 0 : (ts - wl) / wi + 1, f_hi = min(F - 1, ts / wi);
    const bool full = f_hi - f_lo == 3;
    const double *__restrict__ wv = w4 + pad(ts % wi);
    auto Vat = [&](int j) -> double {  // V[ts + j]; 0 from nend on
      if (full) return wv[j];
      double V = 0.0;
      for (int f = f_lo; f <= f_hi; ++f) V += W2(ts + j - f * wi);
      return V;
    };
    // (m[t - 1], m[t - 2]) at the sub-segments' starts.  The loops over sub-segments stay rolled: unrolled,
    // the kernel wants more than 512 registers and spills 800 of them
    double sy1[NSUB], sy2[NSUB];
    {
      double y1 = i1, y2 = i2, e1 = eb1, e2 = eb2;
#pragma unroll 1
      for (int u = 0; u < NSUB; ++u) {
        sy1[u] = y1, sy2[u] = y2;
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
          const double e0 = (double)buf[sb + u * SUB + j];
          const double y = fma(na1, y1, fma(na2, y2, b0 * (e0 - e2)));
          y2 = y1, y1 = y, e2 = e1, e1 = e0;
        }
      }
    }
    // q of sub-segment u: (2 c_k / F) m[t] V[t]
    auto sub_q = [&](int u, double y1, double y2, double(&q)[SUB]) {
      double e1 = u ? (double)buf[sb + u * SUB - 1] : eb1, e2 = u ? (double)buf[sb + u * SUB - 2] : eb2;
#pragma unroll
      for (int j = 0; j < SUB; ++j) {
        const double e0 = (double)buf[sb + u * SUB + j];
        const double y = fma(na1, y1, fma(na2, y2, b0 * (e0 - e2)));
        y2 = y1, y1 = y, e2 = e1, e1 = e0;
        q[j] = (coef * y) * Vat(u * SUB + j);
      }
    };
    // pass A: (r[ts], r[ts + 1]) from a zero state after the segment (the tile's last: the carried one)
    double r1 = s == NSEG - 1 ? Rc1 : 0.0, r2 = s == NSEG - 1 ? Rc2 : 0.0;  // r[t + 1], r[t + 2]
#pragma unroll 1
    for (int u = NSUB - 1; u >= 0; --u) {
      double q[SUB];
      sub_q(u, sy1[u], sy2[u], q);
#pragma unroll
      for (int j = SUB - 1; j >= 0; --j) {
        const double r = fma(na1, r1, fma(na2, r2, q[j]));
        r2 = r1, r1 = r;
      }
    }
#pragma unroll
    for (int l = 0; l < NLEV; ++l) {
      const double u1 = __shfl_down(r1, 1 << l, 32), u2 = __shfl_down(r2, 1 << l, 32);
      if (s + (1 << l) < NSEG) {
        const double *__restrict__ M = mc + 3 + 4 * l;
        r1 += fma(M[0], u1, M[1] * u2);
        r2 += fma(M[2], u1, M[3] * u2);
      }
    }
    {
      double n1 = __shfl_down(r1, 1, 32), n2 = __shfl_down(r2, 1, 32);
      if (s == NSEG - 1) n1 = Rc1, n2 = Rc2;
      Rc1 = __shfl(r1, 0, 32), Rc2 = __shfl(r2, 0, 32);  // the state at the tile's first sample
      r1 = n1, r2 = n2;
    }
    // pass B: r from the true state; de over the envelope, a round per sub-segment
#pragma unroll 1
    for (int u = NSUB - 1; u >= 0; --u) {
      double q[SUB];
      sub_q(u, sy1[u], sy2[u], q);
#pragma unroll
      for (int j = SUB - 1; j >= 0; --j) {
        const double r = fma(na1, r1, fma(na2, r2, q[j]));
        const double d = b0 * (r - r2);
        const double o = __shfl_xor(d, 32, 64);  // the wave's other filter, same segment
        if (lane < 32) dsum[wave][s][j] = d + o;
        r2 = r1, r1 = r;
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int idx = 2 * tid + h, ss = idx / SUB, jj = idx % SUB;
        const double de = ((dsum[0][ss][jj] + dsum[1][ss][jj]) + dsum[2][ss][jj]) + dsum[3][ss][jj];
        buf[ss * SEGP + u * SUB + jj] = (float)de;  // (sub-segment u's envelope: read by no later round)
      }
      __syncthreads();
    }

    // ---- the envelope's and the gammatone's adjoint: samples c0 .. c0 + 15, last first
    cf2 a[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const float e = sqrtf(fmaf(v[j].r, v[j].r, v[j].i * v[j].i));
      const float g = e > 0.f ? buf[pad(c0 + j)] / e : 0.f;
      a[j] = {g * v[j].r, g * v[j].i};
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      cf2 c = tid == T - 1 ? Ta[st] : zero;  // (the tile's last lane starts from the carried state)
#pragma unroll
      for (int j = C - 1; j >= 0; --j) c = cfma(pc, c, a[j]);
#pragma unroll
      for (int l = 0; l < 6; ++l) {
        const cf2 u = cshfl_down(c, 1 << l);
        if (lane + (1 << l) < 64) c = cfma(Qc[l], u, c);
      }
      if (lane == 0) wt[st][wave] = c;
      cf2 ex = cshfl_down(c, 1);
      if (lane == 63) ex = zero;
      __syncthreads();
      const cf2 t0 = wt[st][0], t1 = wt[st][1], t2 = wt[st][2], t3 = wt[st][3];
      const cf2 cw2 = t3, cw1 = cfma(Q6c, cw2, t2), cw0 = cfma(Q6c, cw1, t1);
      const cf2 cw = wave == 3 ? zero : wave == 2 ? cw2 : wave == 1 ? cw1 : cw0;
      cf2 cin = cfma(PLr, cw, ex);
      if (tid == T - 1) cin = Ta[st];
      Ta[st] = cfma(Q6c, cw0, t0);
      c = cin;
#pragma unroll
      for (int j = C - 1; j >= 0; --j) {
        c = cfma(pc, c, a[j]);
        a[j] = c;
      }
    }
    // the three taps read a4[t + 1 .. t + 3]: the next lane's first three values
    ah[tid][0] = a[0], ah[tid][1] = a[1], ah[tid][2] = a[2];
    __syncthreads();
    cf2 ae[C + 3];
#pragma unroll
    for (int j = 0; j < C; ++j) ae[j] = a[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) ae[C + j] = tid == T - 1 ? ahn[j] : ah[tid + 1 - (tid == T - 1)][j];
    float dx[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const float t1 = fmaf(G.c1.r, ae[j + 1].r, G.c1.i * ae[j + 1].i);
      const float t2 = fmaf(G.c2.r, ae[j + 2].r, G.c2.i * ae[j + 2].i);
      const float t3 = fmaf(G.c3.r, ae[j + 3].r, G.c3.i * ae[j + 3].i);
      dx[j] = (t1 + t2) + t3;
    }
    float4 *__restrict__ o = reinterpret_cast<float4 *>(plane + base + c0);  // 64-byte aligned
#pragma unroll
    for (int j = 0; j < C; j += 4) o[j / 4] = make_float4(dx[j], dx[j + 1], dx[j + 2], dx[j + 3]);
    __syncthreads();  // (every lane has read ahn)
    if (tid == 0) ahn[0] = a[0], ahn[1] = a[1], ahn[2] = a[2];
  }
}

// grad[row, t] = sum_i plane_i[t], t < nend - 1; zeros elsewhere below `length`.
__global__ __launch_bounds__(T) void srmr_grad_reduce(const int32_t *__restrict__ lengths, int length, int64_t r0,
                                                      int wl, int wi, const RowC *__restrict__ rowc,
                                                      const float *__restrict__ planes, int64_t pstride,
                                                      float *__restrict__ grad, int64_t ld, int vec) {
  const int64_t lr = blockIdx.y, row = r0 + lr;
  const int t0 = 4 * (blockIdx.x * T + threadIdx.x);
  if (t0 >= length) return;
  const int n = row_length(lengths, row, length);
  const int F = n >= wl ? (n - wl) / wi + 1 : 0;
  const int stop = F > 0 && rowc[row].live ? (F - 1) * wi + wl - 1 : 0;  // nend - 1
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  if (t0 < stop) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const float *__restrict__ p = planes + lr * NCH * pstride + t0;  // (t0 + 3 < the row's tiles' end)
    for (int i = 0; i < NCH; ++i) {
      const float4 x = *reinterpret_cast<const float4 *>(p + i * pstride);
      acc[0] += (double)x.x, acc[1] += (double)x.y, acc[2] += (double)x.z, acc[3] += (double)x.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = t0 + j < stop ? (float)acc[j] : 0.f;
  }
  float *out = grad + row * ld + t0;
  if (vec && t0 + 4 <= length) {
    *reinterpret_cast<float4 *>(out) = make_float4(o[0], o[1], o[2], o[3]);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (t0 + j < length) out[j] = o[j];
}

// The scratch: the rows' coefficients, then one pass's checkpoints and planes.  Every region is
// written by the call that reads it.
struct GradWs {
  RowC *rowc;
  Ckpt *ckpt;
  float *planes;
};
inline int64_t tiles_of(int64_t length) { return (length + TILE - 1) / TILE; }
inline int64_t pass_rows(int64_t length) {
  const int64_t per_row = NCH * tiles_of(length) * (int64_t)(sizeof(Ckpt) + TILE * sizeof(float));
  return std::min<int64_t>(kMaxGridY, std::max<int64_t>(1, kPassBytes / per_row));
}
inline GradWs grad_layout(Arena &a, int64_t batch, int64_t length) {
  const int64_t rows = std::min(batch, pass_rows(length)), nt = tiles_of(length);
  GradWs w;
  w.rowc = a.take<RowC>((size_t)batch);
  w.ckpt = a.take<Ckpt>((size_t)(rows * NCH * nt));
  w.planes = a.take<float>((size_t)(rows * NCH * nt * TILE));
  return w;
}

}  // namespace srmr
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_srmrgrad_pass_rows(int64_t length) {
  if (length < 1 || length > kMaxLength) return 0;
  return srmr::pass_rows(length);
}

extern "C" int64_t fsem_srmrgrad_scratch_bytes(int64_t batch, int64_t length) {
  if (batch < 1 || length < 1 || length > kMaxLength) return 0;
  return (int64_t)layout_bytes(srmr::grad_layout, batch, length);
}

extern "C" int fsem_srmrgrad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                                 int32_t sample_rate, const double *energies, const float *gout, void *scratch,
                                 float *grad, void *stream) {
  if (!deg || !energies || !gout || !scratch || !grad || batch < 1 || length < 1 || ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  if (sample_rate != 8000 && sample_rate != 16000) return FSEM_ERATE;
  srmr::Params P;
  srmr::ScoreParams S;
  srmr::make_params(sample_rate, &P, &S);
  Arena a(scratch);
  const srmr::GradWs w = srmr::grad_layout(a, batch, length);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = sample_rate == 16000;
  const int wl = wide ? 4096 : 2048, wi = wl / 4;
  const int ntmax = (int)srmr::tiles_of(length);
  const int64_t pstride = (int64_t)ntmax * srmr::TILE;
  const int64_t pass = srmr::pass_rows(length);
  const int vec = ((uintptr_t)grad & 15) == 0 && ld % 4 == 0;
  hipLaunchKernelGGL(srmr::srmr_grad_rows, grid_xy(batch), dim3(srmr::RT), 0, st, deg, ld, lengths, (int)length, batch,
                     wl, wi, S, energies, gout, w.rowc);
  FSEM_CHECK_LAUNCH();
  const unsigned wblocks = (unsigned)((length + 4 * srmr::T - 1) / (4 * srmr::T));
  for (int64_t r0 = 0; r0 < batch; r0 += pass) {
    const unsigned rows = (unsigned)std::min(pass, batch - r0);
    if (length >= wl) {  // (no row has a frame otherwise)
      if (wide)
        hipLaunchKernelGGL(srmr::srmr_grad_planes<true>, dim3(srmr::NCH, rows), dim3(srmr::T), 0, st, deg, ld, lengths,
                           (int)length, r0, P, w.rowc, w.ckpt, ntmax, w.planes, pstride);
      else
        hipLaunchKernelGGL(srmr::srmr_grad_planes<false>, dim3(srmr::NCH, rows), dim3(srmr::T), 0, st, deg, ld,
                           lengths, (int)length, r0, P, w.rowc, w.ckpt, ntmax, w.planes, pstride);
      FSEM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(srmr::srmr_grad_reduce, dim3(wblocks, rows), dim3(srmr::T), 0, st, lengths, (int)length, r0, wl,
                       wi, w.rowc, w.planes, pstride, grad, ld, vec);
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}
