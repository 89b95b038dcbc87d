// Gradient of the log-spectral distance with respect to the denoised rows (include/fsem.h, "LSD with
// gradients"; the forward: lsd.hip in libfsem_lsd.so, definition include/fsem_lsd.h).  Nothing of the
// forward call is kept: the entry recomputes the rows' scales with the forward's own kernels
// (fsem_lsd_kernels.h), then
//
//   lsd_grad_frames  grid (16 frames, row), 4 waves, a wave takes four CONSECUTIVE frames as two pairs.
//                    Per frame the forward's transform of z = w s + i w a h in double, then for the 257
//                    bins root, ratio and logarithm in double (t of order 1e-6 on near-identical rows:
//                    a float32 logarithm has no digits left there, and the backward divides by the
//                    frame's value), the frame's value v and the cotangents
//                      G_k = t_k / (257 v F) * (-2 q_k / ((|H_k| + 1e-8)(q_k + 1e-8))) * H_k / |H_k|
//                    (0 where |H_k| = 0 or v = 0).  Per pair (A, B) ONE complex transform gives both
//                    frames' x_t = Re sum_k G_k e^{+2 pi i k t / 512}: the spectra are made Hermitian
//                    (X_k = G_k / 2, X_{512-k} = conj(G_k) / 2, X_0 and X_256 real), so their inverse
//                    transforms are real, and the inverse of X^A + i X^B is x^A + i x^B; the inverse is
//                    the conjugate of the forward transform of the conjugate.  Times the window.
//                    Overlap-add: hop j (samples 256 j ... 256 j + 255) gets frame j's second half and
//                    frame j + 1's first half, which sit in the same lanes and registers (t = lane +
//                    64 r): inside a wave's four frames the sums are formed in registers; between two
//                    waves of a block the later wave's first half goes through LDS; between two blocks
//                    it goes to the `edge` area of the state and lsd_grad_write adds it.  Two addends
//                    per sample: no atomics, no ordering rule.  ybar (double) goes to the state.
//                    Sum over the frame of (w x) h, the frame's share of D = sum_t ybar_t h_t, per lane in
//                    the order of the frames, over the wave by xor exchanges, over the block's four
//                    waves in a fixed tree: one double per (row, block).
//   lsd_grad_rows    one thread per row: sum h h from the chunk records and D from the block records, both
//                    in ascending order; e = D / (sum h h + 1e-8).
//   lsd_grad_write   four samples per thread: grad = g (a ybar + e (s - 2 a h)) in double, rounded once
//                    to float32; zeros from the row's length on and for a row with a non-finite sample.
//
// Every sum has one order that depends on n alone, and which of the three overlap-add paths a hop
// takes depends on the hop's index alone: a row's gradient does not depend on the batch size, the
// row's position, `length`, `ld`, `grad_ld`, the alignment or the stream.
#include <math.h>

#include "fsem_lsd_kernels.h"
#include "fsem_resample.h"

namespace fsem {
namespace lsd {

// What lsd_grad_write needs of a row: the scale (NaN: a row with a non-finite sample) and e.
struct RowC {
  double a, e;
};

// Frame f of the row: the cotangents G[r] of the bins lane + 64 r, r < 4 (G[4]: bin 256, lane 0 only;
// zero in the other lanes), and the frame's samples of h (hv[r] = h[256 f - 256 + lane + 64 r], zero
// outside [0, n)).
// S: the rows' sample type, float (the engine's 16 kHz rows) or double (rows resampled in double by
// fsem_lsd_grad_rate_f32: 8-byte loads in the transform's order, VEC unused).
template <class S, bool VEC>
__device__ __forceinline__ void frame_cotangent(const S *__restrict__ srow, const S *__restrict__ hrow, int f,
                                                int n, int F, double a, int lane, int plane, cd *buf, const cd *tw,
                                                cd G[5], S hv[8]) {
  const int p0 = f * HOP - HOP;  // the frame's first sample; -256 for frame 0
  S sv[8];
  if constexpr (sizeof(S) == sizeof(float)) {
    float *fb = reinterpret_cast<float *>(buf);
    FSEM_LSD_LOAD_FRAME(VEC, srow, hrow, p0, n, lane, fb, sv, hv)
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int t = p0 + lane + 64 * r;
      const bool in = t >= 0 && t < n;
      sv[r] = in ? srow[t] : 0.0;
      hv[r] = in ? hrow[t] : 0.0;
    }
  }
  // a frame of one signal that is all zero has an exactly zero spectrum, as in the forward
  bool snz = false, hnz = false;
  cd v[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    snz |= sv[r] != (S)0;
    hnz |= hv[r] != (S)0;
    const double w = 0.5 * (1.0 - tw[lane + 64 * r].r);  // periodic Hann
    v[r] = {w * (double)sv[r], w * (a * (double)hv[r])};
  }
  const bool s_zero = !__any(snz), h_zero = !__any(hnz) || a == 0.0;
  fft512_wave_d(v, buf, lane, tw);  // v[r] = Z[lane + 64 r]
  double acc = 0;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    const cd m = r < 4 ? mirror_bin(v, r, lane, plane) : v[4];
    // S = (Z + conj M) / 2, H = (Z - conj M) / (2 i) = (hr - i hi) / 2
    const double sr = v[r].r + m.r, si = v[r].i - m.i, hr = v[r].i + m.i, hi = v[r].r - m.r;
    const double S2 = s_zero ? 0.0 : 0.25 * fma(sr, sr, si * si);
    const double H2 = h_zero ? 0.0 : 0.25 * fma(hr, hr, hi * hi);
    const double Hm = sqrt(H2), He = Hm + 1e-8;
    const double q = S2 / (He * He), qe = q + 1e-8;
    const double t = log(qe);
    const bool own = r < 4 || lane == 0;
    acc = own ? fma(t, t, acc) : acc;
    // d lsd / d|H_k| without the frame's 1 / (257 v F); |H_k| = 0 takes the subgradient 0
    const double c = (own && Hm > 0.0) ? t * (-2.0 * q / (He * qe)) : 0.0;
    const double ur = Hm > 0.0 ? (0.5 * hr) / Hm : 0.0, ui = Hm > 0.0 ? (-0.5 * hi) / Hm : 0.0;
    G[r] = {c * ur, c * ui};
  }
  const double tot = wave_sum_d(acc);
  const double vf = sqrt(tot / (double)NBIN);
  const double fac = vf > 0.0 ? 1.0 / ((double)NBIN * vf * (double)F) : 0.0;  // a frame with v = 0 contributes 0
#pragma unroll
  for (int r = 0; r < 5; ++r) G[r] = {G[r].r * fac, G[r].i * fac};
}

template <class S, bool VEC>
__global__ __launch_bounds__(T) void lsd_grad_frames(const S *__restrict__ ref, const S *__restrict__ deg,
                                                     int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                     int64_t r0, const cd *__restrict__ twg,
                                                     const double *__restrict__ scale, double *__restrict__ ybar,
                                                     int64_t ycap, double *__restrict__ edge,
                                                     double *__restrict__ dpart, int nfb) {
  __shared__ __attribute__((aligned(16))) cd xbuf[NWAVE * NFFT];  // a wave's exchange area: 512 complex doubles
  __shared__ __attribute__((aligned(16))) cd tw[NFFT];
  __shared__ double red[NWAVE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = r0 + blockIdx.y;
  const int n = row_length(lengths, row, length);
  const int F = 1 + n / HOP;
  const int f0 = blockIdx.x * KF;
  if (f0 >= F) return;  // (the whole block)
  const double a = scale[row];
  if (isnan(a)) return;  // a row with a non-finite sample: lsd_grad_write writes its zeros (the whole block)
  for (int i = threadIdx.x; i < NFFT; i += T) tw[i] = twg[i];
  __syncthreads();
  const S *__restrict__ srow = ref + row * ld;
  const S *__restrict__ hrow = deg + row * ld;
  double *__restrict__ yrow = ybar + row * ycap;
  cd *buf = xbuf + wave * NFFT;
  const int plane = (64 - lane) & 63;
  const int fa = f0 + (KF / NWAVE) * wave;  // this wave's frames fa ... fa + 3 (wave-uniform)
  double head[4] = {0, 0, 0, 0};  // frame fa's first half, hop fa - 1's second addend
  double tail[4] = {0, 0, 0, 0};  // the last frame's second half where a later frame follows it
  int tail_hop = -1;
  double dacc = 0;
#pragma unroll 1
  for (int u = 0; u < KF / NWAVE / 2; ++u) {
    const int f = fa + 2 * u;
    if (f >= F) break;
    const bool hasB = f + 1 < F;
    cd GA[5], GB[5];
    S hA[8], hB[8];
    frame_cotangent<S, VEC>(srow, hrow, f, n, F, a, lane, plane, buf, tw, GA, hA);
    if (hasB) {
      frame_cotangent<S, VEC>(srow, hrow, f + 1, n, F, a, lane, plane, buf, tw, GB, hB);
    } else {
#pragma unroll
      for (int r = 0; r < 5; ++r) GB[r] = {0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 8; ++r) hB[r] = (S)0;
    }
    // U = conj(X^A + i X^B): U_k = (conj A_k - i conj B_k) / 2, U_{512-k} = (A_k - i B_k) / 2
    cd v[8], m[5];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = {0.5 * (GA[r].r - GB[r].i), -0.5 * (GA[r].i + GB[r].r)};
      m[r] = {0.5 * (GA[r].r + GB[r].i), 0.5 * (GA[r].i - GB[r].r)};
    }
    m[4] = {GA[4].r, -GB[4].r};  // bin 256 (read by lane 0 alone)
    if (lane == 0) v[0] = {GA[0].r, -GB[0].r};
#pragma unroll
    for (int r = 4; r < 8; ++r) v[r] = mirror_bin(m, r, lane, plane);  // bin lane + 64 r = 512 - k
    fft512_wave_d(v, buf, lane, tw);  // x^A_t = Re, x^B_t = -Im at t = lane + 64 r
    double cA[8], cB[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const double w = 0.5 * (1.0 - tw[lane + 64 * r].r);
      cA[r] = w * v[r].r;
      cB[r] = -(w * v[r].i);
      dacc = fma(cA[r], (double)hA[r], dacc);
      dacc = fma(cB[r], (double)hB[r], dacc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = lane + 64 * q;
      if (u == 0) {
        head[q] = cA[q];
      } else {  // hop f - 1: the first pair's frame B and this frame A
        const int i = (f - 1) * HOP + t;
        if (i < n) yrow[i] = tail[q] + cA[q];
      }
      const int i = f * HOP + t;  // hop f: both addends in this pair, or the row's last hop
      if (i < n) yrow[i] = hasB ? cA[4 + q] + cB[q] : cA[4 + q];
      tail[q] = cB[4 + q];
    }
    tail_hop = hasB ? f + 1 : -1;
  }
  // the first half of this wave's first frame: to the wave before it, or to the block before it
  if (fa < F) {
    if (wave > 0) {
      double *hb = reinterpret_cast<double *>(buf);
#pragma unroll
      for (int q = 0; q < 4; ++q) hb[lane + 64 * q] = head[q];
    } else if (blockIdx.x > 0) {
      double *__restrict__ e = edge + (row * nfb + blockIdx.x) * HOP;
#pragma unroll
      for (int q = 0; q < 4; ++q) e[lane + 64 * q] = head[q];
    }
  }
  dacc = wave_sum_d(dacc);
  if (lane == 0) red[wave] = dacc;  // (0 for a wave without a frame)
  __syncthreads();
  if (tail_hop >= 0) {
    // a later frame follows: in this wave's range it was consumed above, so tail_hop == fa + 3 or
    // the row's last hop
    const bool next = tail_hop + 1 < F;
    const double *hn = reinterpret_cast<const double *>(xbuf + (wave + 1 < NWAVE ? wave + 1 : wave) * NFFT);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = tail_hop * HOP + lane + 64 * q;
      if (i < n) yrow[i] = (next && wave + 1 < NWAVE) ? tail[q] + hn[lane + 64 * q] : tail[q];
    }
  }
  if (threadIdx.x == 0) dpart[row * nfb + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(ST) void lsd_grad_rows(const Part *__restrict__ part, int nchunk,
                                                    const double *__restrict__ dpart, int nfb,
                                                    const double *__restrict__ scale,
                                                    const int32_t *__restrict__ lengths, int length, int64_t B,
                                                    RowC *__restrict__ rowc) {
  const int64_t b = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (b >= B) return;
  const double a = scale[b];
  if (isnan(a)) {
    rowc[b] = {a, 0.0};
    return;
  }
  const int n = row_length(lengths, b, length);
  const int nc = (n + C - 1) / C, nb = (1 + n / HOP + KF - 1) / KF;
  const Part *__restrict__ p = part + b * nchunk;
  double hh = 0, D = 0;
  for (int c = 0; c < nc; ++c) hh += p[c].hh;
  const double *__restrict__ d = dpart + b * nfb;
  for (int i = 0; i < nb; ++i) D += d[i];
  rowc[b] = {a, D / (hh + 1e-8)};
}

// One element: g (a ybar + e (s - 2 a h)), rounded once.
template <class S>
__device__ __forceinline__ S grad_elem(double g, double a, double e, double y, S s, S h) {
  return (S)(g * fma(a, y, e * fma(-2.0 * a, (double)h, (double)s)));
}

// S = double (fsem_lsd_grad_rate_f32): rows in double, and the gradient with respect to them in double:
// `grad` may be ybar itself (each thread reads and writes its own four elements).
template <class S, bool VEC, bool VECOUT>
__global__ __launch_bounds__(T) void lsd_grad_write(const S *__restrict__ ref, const S *__restrict__ deg,
                                                    int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                    int64_t r0, const double *ybar, int64_t ycap,
                                                    const double *__restrict__ edge, int nfb,
                                                    const RowC *__restrict__ rowc, const float *__restrict__ g_lsd,
                                                    S *grad, int64_t grad_ld) {
  const int64_t row = r0 + blockIdx.y;
  const int t0 = 4 * (blockIdx.x * T + threadIdx.x);  // < length + 4 T
  if (t0 >= length) return;
  const int n = row_length(lengths, row, length);
  S o[4] = {(S)0, (S)0, (S)0, (S)0};
  const RowC rc = rowc[row];
  if (t0 < n && !isnan(rc.a)) {
    const int F = 1 + n / HOP;
    S sv[4], hv[4];
    if constexpr (sizeof(S) == sizeof(float)) {
      load4<VEC>(ref + row * ld, t0, n, sv);
      load4<VEC>(deg + row * ld, t0, n, hv);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sv[j] = t0 + j < n ? ref[row * ld + t0 + j] : 0.0;
        hv[j] = t0 + j < n ? deg[row * ld + t0 + j] : 0.0;
      }
    }
    const double *y = ybar + row * ycap + t0;  // 32-byte aligned
    const int hop = t0 >> 8;                                // (of all four: t0 % 4 == 0)
    const bool cross = (hop & (KF - 1)) == KF - 1 && hop + 1 < F;  // the next block's first frame reaches it
    const double *__restrict__ e = edge + (row * nfb + ((hop + 1) >> 4)) * HOP + (t0 & (HOP - 1));
    const double g = (double)g_lsd[row];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (t0 + j < n) {
        const double yv = cross ? y[j] + e[j] : y[j];
        o[j] = grad_elem(g, rc.a, rc.e, yv, sv[j], hv[j]);
      }
    }
  }
  S *out = grad + row * grad_ld + t0;
  if constexpr (VECOUT && sizeof(S) == sizeof(float)) {
    if (t0 + 4 <= length) {
      *reinterpret_cast<float4 *>(out) = make_float4(o[0], o[1], o[2], o[3]);
      return;
    }
  }
  {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < length) out[j] = o[j];
  }
}

// The state: the twiddles, the rows' scales, one record per (row, chunk), one share of D per (row,
// frame block), the rows' (a, e), the first half-frame of every frame block and ybar.  Scratch:
// every region is written by the call that reads it.
struct GradWs {
  cd *tw;
  double *scale;
  Part *part;
  double *dpart;
  RowC *rowc;
  double *edge;
  double *ybar;
};
inline int64_t frame_blocks(int64_t length) { return (frames_of(length) + KF - 1) / KF; }
inline int64_t ceil4(int64_t length) { return (length + 3) / 4 * 4; }
inline GradWs grad_layout(Arena &a, int64_t batch, int64_t length) {
  GradWs w;
  w.tw = a.take<cd>((size_t)NFFT);
  w.scale = a.take<double>((size_t)batch);
  w.part = a.take<Part>((size_t)batch * (size_t)chunks(length));
  w.dpart = a.take<double>((size_t)batch * (size_t)frame_blocks(length));
  w.rowc = a.take<RowC>((size_t)batch);
  w.edge = a.take<double>((size_t)batch * (size_t)frame_blocks(length) * HOP);
  w.ybar = a.take<double>((size_t)batch * (size_t)ceil4(length));
  return w;
}

// ---- rows at another rate (fsem_lsd_grad_rate_f32): the 16 kHz rows in double, never rounded to float32.
// The forward's resampler stores float32 rows; rows resampled from 8 kHz have an upper half-spectrum 100 dB
// below a frame's peak, where that rounding (1e-7 of the peak) is a tenth of a bin and moves the gradient
// by per cent.  So the backward resamples both rows itself, with the forward's float32 taps and the sums in
// double, differentiates at those rows (the kernels above on double rows) and pulls the double gradient back
// through the transposed resampler, rounding once at the float32 store.

// n16[b] = ceil(n_b nw / orig), the row's 16 kHz length.
__global__ void lsd_rate_lengths(const int32_t *__restrict__ lengths, int length, int64_t B, int orig, int nw,
                                 int32_t *__restrict__ n16) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int64_t n = row_length(lengths, b, length);
  n16[b] = (int32_t)((n * nw + orig - 1) / orig);
}

__device__ __forceinline__ double rate_coef(const ResampleKernel &rk, const float *ks, int j, int t) {
  return (double)(rk.big ? sinc_coef(j, t, rk.orig, rk.nw, rk.width) : ks[j * rk.taps + t]);
}

// out[b, o] = sum_t K[o mod nw][t] x[b, m orig - width + t] in double (x = 0 outside [0, n_b)), o < n16[b];
// grid (256 outputs, row, operand).
__global__ void __launch_bounds__(T) lsd_rate_resample(const float *__restrict__ ref, const float *__restrict__ deg,
                                                       int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                       int64_t r0, const int32_t *__restrict__ n16,
                                                       double *__restrict__ ref16, double *__restrict__ deg16,
                                                       int64_t ycap, ResampleKernel rk) {
  __shared__ float ks[FSEM_RS_MAX_COEF];
  if (!rk.big)
    for (int i = threadIdx.x; i < rk.nw * rk.taps; i += T) ks[i] = rk.k[i];
  __syncthreads();
  const int64_t row = r0 + blockIdx.y;
  const int64_t o = (int64_t)blockIdx.x * T + threadIdx.x;
  if (o >= n16[row]) return;  // (the kernels above read nothing at or past n16)
  const int64_t n = row_length(lengths, row, length);
  const float *__restrict__ x = (blockIdx.z ? deg : ref) + row * ld;
  const int64_t m = o / rk.nw;
  const int j = (int)(o - m * rk.nw);
  const int64_t base = m * rk.orig - rk.width;
  double acc = 0.0;
  for (int t = 0; t < rk.taps; ++t) {
    const int64_t i = base + t;
    if (i >= 0 && i < n) acc = fma(rate_coef(rk, ks, j, t), (double)x[i], acc);
  }
  (blockIdx.z ? deg16 : ref16)[row * ycap + o] = acc;
}

// The state of the rate entry: the 16 kHz entry's at the resampled length, the rows' 16 kHz lengths and both
// rows in double [ceil4(length16)].  The gradient with respect to the 16 kHz rows overwrites ybar.
struct RateWs {
  GradWs g;
  int32_t *n16;
  double *ref16, *deg16;
};
inline RateWs rate_layout(Arena &a, int64_t batch, int64_t length16) {
  RateWs w;
  w.g = grad_layout(a, batch, length16);
  w.n16 = a.take<int32_t>((size_t)batch);
  w.ref16 = a.take<double>((size_t)batch * (size_t)ceil4(length16));
  w.deg16 = a.take<double>((size_t)batch * (size_t)ceil4(length16));
  return w;
}

}  // namespace lsd
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_lsd_grad_state_floats(int64_t batch, int64_t length) {
  if (batch < 1 || length < 1 || length > kMaxLength) return 0;
  return (int64_t)(layout_bytes(lsd::grad_layout, batch, length) / sizeof(float));
}

extern "C" int fsem_lsd_grad_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                 const int32_t *lengths, const float *g_lsd, float *state, float *grad,
                                 int64_t grad_ld, void *stream) {
  if (!ref || !deg || !g_lsd || !state || !grad || batch < 1 || length < 1 || ld < length || grad_ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  Arena a(state);
  const lsd::GradWs w = lsd::grad_layout(a, batch, length);
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = (int)lsd::chunks(length);
  const int nfb = (int)lsd::frame_blocks(length);
  const int64_t ycap = lsd::ceil4(length);
  // 16-byte loads where every row of both operands starts on a 16-byte boundary, as the forward
  const bool vec = (((uintptr_t)ref | (uintptr_t)deg) & 15) == 0 && ld % 4 == 0;
  const bool vecout = ((uintptr_t)grad & 15) == 0 && grad_ld % 4 == 0;
  const int rc = lsd::launch_scales(ref, deg, batch, length, ld, lengths, vec, w.tw, w.part, w.scale, st);
  if (rc != FSEM_OK) return rc;
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)nfb, batch, r0);
    if (vec)
      hipLaunchKernelGGL((lsd::lsd_grad_frames<float, true>), grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length, r0,
                         w.tw, w.scale, w.ybar, ycap, w.edge, w.dpart, nfb);
    else
      hipLaunchKernelGGL((lsd::lsd_grad_frames<float, false>), grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length,
                         r0, w.tw, w.scale, w.ybar, ycap, w.edge, w.dpart, nfb);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(lsd::lsd_grad_rows, dim3((unsigned)((batch + lsd::ST - 1) / lsd::ST)), dim3(lsd::ST), 0, st,
                     w.part, nchunk, w.dpart, nfb, w.scale, lengths, (int)length, batch, w.rowc);
  FSEM_CHECK_LAUNCH();
  const unsigned wblocks = (unsigned)((length + 4 * lsd::T - 1) / (4 * lsd::T));
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice(wblocks, batch, r0);
#define FSEM_LSD_WRITE(V, VO)                                                                                      \
  hipLaunchKernelGGL((lsd::lsd_grad_write<float, V, VO>), grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length, \
                     r0, w.ybar, ycap, w.edge, nfb, w.rowc, g_lsd, grad, grad_ld)
    if (vec && vecout) FSEM_LSD_WRITE(true, true);
    else if (vec) FSEM_LSD_WRITE(true, false);
    else if (vecout) FSEM_LSD_WRITE(false, true);
    else FSEM_LSD_WRITE(false, false);
#undef FSEM_LSD_WRITE
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}

extern "C" int64_t fsem_lsd_grad_rate_state_floats(int64_t batch, int64_t length, int32_t sample_rate) {
  if (batch < 1 || length < 1 || length > kMaxLength) return 0;
  if (sample_rate == 16000) return fsem_lsd_grad_state_floats(batch, length);
  ResampleKernel rk;
  if (make_resample_kernel(sample_rate, 16000, &rk) != FSEM_OK) return 0;
  const int64_t l16 = (rk.nw * length + rk.orig - 1) / rk.orig;
  if (l16 > kMaxLength) return 0;
  return (int64_t)(layout_bytes(lsd::rate_layout, batch, l16) / sizeof(float));
}

extern "C" int fsem_lsd_grad_rate_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                      const int32_t *lengths, int32_t sample_rate, const float *g_lsd, float *state,
                                      float *grad, int64_t grad_ld, void *stream) {
  if (!ref || !deg || !g_lsd || !state || !grad || batch < 1 || length < 1 || ld < length || grad_ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  if (sample_rate == 16000)
    return fsem_lsd_grad_f32(ref, deg, batch, length, ld, lengths, g_lsd, state, grad, grad_ld, stream);
  ResampleKernel rk;
  const int rc = make_resample_kernel(sample_rate, 16000, &rk);
  if (rc != FSEM_OK) return rc;
  const int64_t l16 = (rk.nw * length + rk.orig - 1) / rk.orig;
  if (l16 > kMaxLength) return FSEM_EINVAL;
  Arena a(state);
  const lsd::RateWs w = lsd::rate_layout(a, batch, l16);
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = (int)lsd::chunks(l16);
  const int nfb = (int)lsd::frame_blocks(l16);
  const int64_t ycap = lsd::ceil4(l16);
  hipLaunchKernelGGL(lsd::lsd_rate_lengths, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, lengths,
                     (int)length, batch, rk.orig, rk.nw, w.n16);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(lsd::lsd_tables, dim3(lsd::NFFT / 256), dim3(256), 0, st, w.g.tw);
  FSEM_CHECK_LAUNCH();
  const unsigned oblocks = (unsigned)((l16 + lsd::T - 1) / lsd::T);
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    dim3 grid = grid_slice(oblocks, batch, r0);
    grid.z = 2;
    hipLaunchKernelGGL(lsd::lsd_rate_resample, grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length, r0,
                       w.n16, w.ref16, w.deg16, ycap, rk);
    FSEM_CHECK_LAUNCH();
    hipLaunchKernelGGL((lsd::lsd_partial<double, false>), grid_slice((unsigned)nchunk, batch, r0), dim3(lsd::T), 0, st,
                       w.ref16, w.deg16, ycap, w.n16, (int)l16, r0, w.g.part, nchunk);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(lsd::lsd_scale, dim3((unsigned)((batch + lsd::ST - 1) / lsd::ST)), dim3(lsd::ST), 0, st,
                     w.g.part, nchunk, w.n16, (int)l16, batch, w.g.scale);
  FSEM_CHECK_LAUNCH();
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    hipLaunchKernelGGL((lsd::lsd_grad_frames<double, false>), grid_slice((unsigned)nfb, batch, r0), dim3(lsd::T), 0,
                       st, w.ref16, w.deg16, ycap, w.n16, (int)l16, r0, w.g.tw, w.g.scale, w.g.ybar, ycap, w.g.edge,
                       w.g.dpart, nfb);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(lsd::lsd_grad_rows, dim3((unsigned)((batch + lsd::ST - 1) / lsd::ST)), dim3(lsd::ST), 0, st,
                     w.g.part, nchunk, w.g.dpart, nfb, w.g.scale, w.n16, (int)l16, batch, w.g.rowc);
  FSEM_CHECK_LAUNCH();
  const unsigned wblocks = (unsigned)((l16 + 4 * lsd::T - 1) / (4 * lsd::T));
  const unsigned iblocks = (unsigned)((length + RS_GRAD_T - 1) / RS_GRAD_T);
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    // the gradient with respect to the 16 kHz rows, in double, over ybar (zeros from n16 on)
    hipLaunchKernelGGL((lsd::lsd_grad_write<double, false, false>), grid_slice(wblocks, batch, r0), dim3(lsd::T), 0,
                       st, w.ref16, w.deg16, ycap, w.n16, (int)l16, r0, w.g.ybar, ycap, w.g.edge, nfb, w.g.rowc,
                       g_lsd, w.g.ybar, ycap);
    FSEM_CHECK_LAUNCH();
    // (the transpose's own per-row output length ceil(n nw / orig) is n16)
    hipLaunchKernelGGL(resample_rows_grad<double>, grid_slice(iblocks, batch, r0), dim3(RS_GRAD_T), 0, st, w.g.ybar,
                       length, ycap, lengths, grad, grad_ld, r0, rk);
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}
