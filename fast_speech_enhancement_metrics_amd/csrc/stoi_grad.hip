// STOI / ESTOI with gradients for gfx950 (MI355X): the backward of stoi.hip with respect to the
// denoised rows (include/fsem.h, "STOI with gradients").
//
// fsem_stoi_state_f32 runs the forward (stoi::run) on a caller-owned state whose head is the forward's
// workspace (stoi::Ws): the 10 kHz rows, the kept frame indices and counts and both envelope sets stay
// there.  fsem_stoi_grad_f32 walks the forward backwards in five kernels, every sum in a fixed order
// (gathers and store-then-sum, no atomics), through scratch in the state's tail:
//
//  stoi_grad_rows      per row: 1 when the row has a segment and every denoised sample is finite; the
//                      inverse of the kept frame indices (frame -> position among the kept, or -1).
//  stoi_seg_grad       per (row, 64 segments), one wave, one lane per segment as stoi_seg: the
//                      derivative of the segment's STOI and ESTOI terms with respect to the denoised
//                      envelopes Y[15, T].  STOI, band by band: the lanes leave six coefficients per
//                      (segment, band) in LDS, then turn into frames and gather their <= 30 segments
//                      in ascending frame offset.  ESTOI: each lane adds its segment's 15 x 30
//                      derivatives to the wave's LDS tile one frame offset at a time (all lanes hit
//                      different frames; the offsets in ascending order).  A wave writes the tile
//                      of the 93 frames its segments cover; a frame lies in at most two tiles.
//  stoi_tob_grad       per (row, 32 STFT frames) as stoi_tob: the overlap-added blocks of the denoised
//                      row rebuilt from the kept frames, two frames per complex 512-point FFT, the
//                      spectrum of each scaled per band by gY / Y (0 where Y = 0), both frames'
//                      one-sided spectra folded into one Hermitian-extended transform back, times
//                      the STFT window: the derivative with respect to each frame's 256 samples.
//  stoi_ola_grad       per 10 kHz sample: the adjoint of the overlap-add of the kept frames, a gather
//                      of at most two blocks of two frame halves each.
//  stoi_resample_grad  per input sample: the transposed polyphase resampler with the forward's taps,
//                      polyphase groups and phases in ascending order (the identity at 10 kHz, where
//                      stoi_ola_grad writes the gradient itself); at 16 kHz stoi_resample_grad16, eight
//                      input samples per lane with the compile-time taps kRs16k10k.
#include <algorithm>

#include "fsem_stoi.h"

namespace fsem {
namespace stoi {

constexpr int GW = 64;               // segments per stoi_seg_grad workgroup (one wave)
constexpr int GFR = GW + NSEG - 1;   // frames those segments cover (93)
constexpr int GLD = 96;              // frames per row of a wave's tile
static_assert(GFR <= GLD && GFR <= 2 * GW, "a frame lies in at most two tiles; two gather rounds");

inline int seg_waves(int64_t tmax) { return tmax > 29 ? (int)((tmax - 29 + GW - 1) / GW) : 1; }

// The state: the forward's workspace, then the backward's scratch.
struct GradWs {
  int *ok;      // [B] rows that get a gradient
  int *pos;     // [B, nv_ld] position of each VAD frame among the row's kept frames, or -1
  float *gyw;   // [B, seg_waves, 15, GLD] envelope derivatives per wave tile
  float *gf;    // [B, tmax, 256] derivatives of the STFT frames' samples
  float *g10;   // [B, y_ld] derivatives of the 10 kHz rows (not at 10 kHz input)
};
struct State {
  Ws fwd;
  GradWs bwd;
};
inline State state_layout(Arena &a, int64_t B, const Geometry &g) {
  State s;
  s.fwd = layout(a, B, g);
  s.bwd.ok = a.take<int>((size_t)B);
  s.bwd.pos = a.take<int>((size_t)B * (size_t)g.nv_ld);
  s.bwd.gyw = a.take<float>((size_t)B * (size_t)seg_waves(g.tmax) * NB * GLD);
  s.bwd.gf = a.take<float>((size_t)B * (size_t)g.tmax * 256);
  s.bwd.g10 = a.take<float>(g.direct ? 0 : (size_t)B * (size_t)g.y_ld);
  return s;
}

__global__ void __launch_bounds__(256)
    stoi_grad_rows(const float *__restrict__ deg, int64_t ld, Rows rows, const int *__restrict__ idx,
                   const int *__restrict__ kept, int nv_ld, int *__restrict__ ok, int *__restrict__ pos) {
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int nk = kept[b];
  const bool scored = nk - 31 > 0;
  // the inverse of the kept indices (ascending, all below the row's frame count <= nv_ld): every slot is
  // written once with -1, then the kept ones once more with their position
  for (int i = tid; i < nv_ld; i += 256) pos[b * nv_ld + i] = -1;
  __syncthreads();
  for (int q = tid; q < nk; q += 256) pos[b * nv_ld + idx[b * nv_ld + q]] = q;
  int bad = 0;
  if (scored) {
    const int64_t n = rows.n(b);
    const float *__restrict__ x = deg + b * ld;
    for (int64_t i = tid; i < n; i += 256) bad |= !__builtin_isfinite(x[i]);
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) ok[b] = (scored && !bad) ? 1 : 0;
}

// 30-frame segments per row (0: the row scores NaN)
__global__ void __launch_bounds__(256)
    stoi_segments(const int *__restrict__ kept, int64_t B, int32_t *__restrict__ segments) {
  const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (b < B) segments[b] = max(kept[b] - 31, 0);
}

// d(g_s STOI_b + g_e ESTOI_b) / dY[j, t] over the segments m0 .. m0 + 63 of row b (_cpu.stoi).
// Segment m, band j, x_t = X[j, m + t], y_t = Y[j, m + t]:
//  STOI   alpha = |x| / (|y| + 1e-9), c_t = min(alpha y_t, kClip x_t), u_t = [alpha y_t < kClip x_t],
//         rho = <xn, cn> with xn = (x - mx) rx, cn = (c - mc) rc (regularised norms).
//         d rho / d c_t = rc (xn_t - rho cn_t), so
//         d rho / d y_t = u_t (a1 (x_t - mx) - a2 (alpha y_t - mc)) + beta y_t
//         a1 = alpha rc rx, a2 = alpha rc^2 rho, beta = -(sum_t u_t y_t d rho / d c_t) alpha / ((|y| + 1e-9) |y|)
//         (0 for |y| = 0: the norm's subgradient).
//  ESTOI  a_y[j, t] = (y_t - my_j) ry_j, by[., t] = (a_y[., t] - mean_j) wy_t with
//         wy_t = (sum_j (.)^2 + (14/15) sum_j 1e-24 ry_j^2 + 15e-24)^-1/2, likewise bx; e_t = sum_j bx by.
//         d E / d a_y[j, t] = g[j, t] = wy_t (bx[j, t] - e_t by[j, t]) (its band mean is 0), and
//         d E / d y_t = ry_j (g[j, t] - mean_s g[j, s] - a_y[j, t] sum_s g[j, s] a_y[j, s]) + kappa_j a_y[j, t]
//         kappa_j = (14/15) 1e-24 ry_j^3 sum_t wy_t^2 e_t: the band normalisation's regulariser seen
//         through the row norms.
__global__ void __launch_bounds__(GW)
    stoi_seg_grad(const float *__restrict__ tob, int64_t B, int64_t tmax, const int *__restrict__ kept,
                  const int *__restrict__ ok, const float *__restrict__ g_stoi, const float *__restrict__ g_estoi,
                  float *__restrict__ gyw, int NW, int64_t b0) {
  __shared__ f2 XY[NB][GLD];
  __shared__ float G[NB][GLD];
  __shared__ float4 CFa[GW];  // (alpha, gs a1, gs a2, mx) per segment: one 16-byte read
  __shared__ float2 CFb[GW];  // (mc, gs beta)
  const int lane = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int wv = blockIdx.x;
  const int n = kept[b];
  const int S = n - 31;
  const int m0 = wv * GW;
  if (!ok[b] || m0 >= S) return;  // (uniform) no tile: stoi_tob_grad reads tiles wv < ceil(S / 64) of rows that are ok
  const int T = n - 2;
  const int nf = min(GFR, T - m0);
  const int nlive = min(GW, S - m0);
  const bool live = lane < nlive;
  const float *xc = tob + (b * NB) * tmax + m0;
  const float *xd = tob + ((b + B) * NB) * tmax + m0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    for (int f = lane; f < GLD; f += GW) {
      const int i = min(f, nf - 1);  // slots past nf: copies no live segment reads
      XY[j][f] = (f2){xc[j * tmax + i], xd[j * tmax + i]};
    }
  }
  wave_lds_fence();
  constexpr float kInvN = 1.f / NSEG;
  constexpr float kReg30 = 30e-24f;
  const float gs = g_stoi[b] / (15.f * (float)S), ge = g_estoi[b] / (30.f * (float)S);
  f2 rxy[NB], nmr[NB];
  f2 nvar = {0.f, 0.f};
#pragma unroll 1
  for (int j = 0; j < NB; ++j) {
    f2 v[NSEG];
    f2 s1 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NSEG; ++t) {
      v[t] = XY[j][lane + t];
      s1 += v[t];
    }
    const f2 mu = s1 * kInvN;
    f2 dd = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NSEG; ++t) {
      const f2 d = v[t] - mu;
      dd = __builtin_elementwise_fma(d, d, dd);
    }
    const f2 s2 = __builtin_elementwise_fma(mu * (float)NSEG, mu, dd);
    const float ny = __builtin_amdgcn_sqrtf(s2.y);
    const float alpha = __builtin_amdgcn_sqrtf(s2.x) * __builtin_amdgcn_rcpf(ny + 1e-9f);
    float c[NSEG];
    float sc = 0.f;
#pragma unroll
    for (int t = 0; t < NSEG; ++t) {
      c[t] = fminf(alpha * v[t].y, kClip * v[t].x);
      sc += c[t];
    }
    const float mc = sc * kInvN;
    float dcc = 0.f, dxc = 0.f;
#pragma unroll
    for (int t = 0; t < NSEG; ++t) {
      const float dc = c[t] - mc;
      dcc = fmaf(dc, dc, dcc);
      dxc = fmaf(v[t].x - mu.x, dc, dxc);
    }
    const float rx = __builtin_amdgcn_rsqf(dd.x + kReg30);
    const float ry = __builtin_amdgcn_rsqf(dd.y + kReg30);
    const float rc = __builtin_amdgcn_rsqf(dcc + kReg30);
    const float rho = dxc * rx * rc;
    const float a1 = alpha * rc * rx, a2 = alpha * rc * rc * rho;
    float ga = 0.f;  // sum_t u_t y_t (a1 (x_t - mx) - a2 (c_t - mc)) = alpha d rho / d alpha
#pragma unroll
    for (int t = 0; t < NSEG; ++t) {
      const bool u = alpha * v[t].y < kClip * v[t].x;
      const float q = a1 * (v[t].x - mu.x) - a2 * (c[t] - mc);
      ga += u ? q * v[t].y : 0.f;
    }
    const float beta = ny > 0.f ? -ga / ((ny + 1e-9f) * ny) : 0.f;
    CFa[lane] = make_float4(alpha, gs * a1, gs * a2, mu.x);
    CFb[lane] = make_float2(mc, gs * beta);
    rxy[j] = (f2){rx, ry};
    nvar = __builtin_elementwise_fma(rxy[j], rxy[j], nvar);
    nmr[j] = -mu * rxy[j];
    wave_lds_fence();
    // the lanes as frames lane and lane + 64 of the tile: their segments by ascending frame offset
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int f = lane + GW * h;
      if (f < GLD) {
        const f2 xy = XY[j][f];
        const float kx = kClip * xy.x;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < NSEG; ++t) {
          const int mm = f - t;
          const bool in = mm >= 0 && mm < nlive;
          const float4 ca = CFa[in ? mm : 0];  // (reads of a live slot, masked below: no branch per offset)
          const float2 cb = CFb[in ? mm : 0];
          const float ay = ca.x * xy.y;
          const float q = ca.y * (xy.x - ca.w) - ca.z * (ay - cb.x);
          const float term = (ay < kx ? q : 0.f) + cb.y * xy.y;
          acc += in ? term : 0.f;
        }
        G[j][f] = acc;
      }
    }
    wave_lds_fence();
  }
  // ESTOI: the columns twice, first for the sums over the segment's frames, then for the derivatives
  const f2 breg = __builtin_elementwise_fma(nvar, (f2){14e-24f / 15.f, 14e-24f / 15.f}, (f2){15e-24f, 15e-24f});
  float m1[NB], m2[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) m1[j] = m2[j] = 0.f;
  float greg = 0.f;
  auto column = [&](int t, f2 a[NB], float g[NB], float &wy2e) {
    f2 ma = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      a[j] = __builtin_elementwise_fma(XY[j][lane + t], rxy[j], nmr[j]);
      ma += a[j];
    }
    ma *= 1.f / NB;
    f2 q = {0.f, 0.f};
    float ac = 0.f;
    f2 d[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      d[j] = a[j] - ma;
      q = __builtin_elementwise_fma(d[j], d[j], q);
      ac = fmaf(d[j].x, d[j].y, ac);
    }
    const float wx = __builtin_amdgcn_rsqf(q.x + breg.x);
    const float wy = __builtin_amdgcn_rsqf(q.y + breg.y);
    const float e = ac * wx * wy;
#pragma unroll
    for (int j = 0; j < NB; ++j) g[j] = wy * (d[j].x * wx - e * (d[j].y * wy));
    wy2e = wy * wy * e;
  };
#pragma unroll 1
  for (int t = 0; t < NSEG; ++t) {
    f2 a[NB];
    float g[NB], w2e;
    column(t, a, g, w2e);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      m1[j] += g[j];
      m2[j] = fmaf(g[j], a[j].y, m2[j]);
    }
    greg += w2e;
  }
  // d E / d y_t = ry g - c2 + c3 a_y with c2 = ry mean g, c3 = kappa - ry sum g a_y  (x ge)
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const float ry = rxy[j].y;
    const float kappa = (14.f / 15.f) * (((1e-24f * ry) * ry) * ry) * greg;
    const float c2 = ge * ry * (m1[j] * kInvN);
    const float c3 = ge * (kappa - ry * m2[j]);
    m1[j] = c2;
    m2[j] = c3;
  }
#pragma unroll 1
  for (int t = 0; t < NSEG; ++t) {
    f2 a[NB];
    float g[NB], w2e;
    column(t, a, g, w2e);
    if (live) {
#pragma unroll
      for (int j = 0; j < NB; ++j) G[j][lane + t] += fmaf(ge * rxy[j].y, g[j], fmaf(m2[j], a[j].y, -m1[j]));
    }
    wave_lds_fence();  // the next offset's frames are other lanes' of this one
  }
  float *out = gyw + ((b * NW + wv) * NB) * GLD;
#pragma unroll
  for (int j = 0; j < NB; ++j)
    for (int f = lane; f < GLD; f += GW) out[j * GLD + f] = G[j][f];
}

constexpr int TGW = 4;  // waves per stoi_tob_grad workgroup
__global__ void __launch_bounds__(64 * TGW)
    stoi_tob_grad(const float *__restrict__ y10, int64_t y_ld, int64_t B, Rows rows, const int *__restrict__ idx,
                  const int *__restrict__ kept, int nv_ld, const float *__restrict__ tob, int64_t tmax,
                  const int *__restrict__ ok, const float *__restrict__ gyw, int NW, float *__restrict__ gf,
                  int64_t b0) {
  __shared__ __attribute__((aligned(16))) float blk[TF + 1][128];
  __shared__ __attribute__((aligned(16))) float xbuf[TGW * 2 * kFftBuf];
  __shared__ float qb[TF][16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t b = b0 + blockIdx.y;
  const int n = kept[b];
  const int T = n - 2, S = n - 31;
  const int k0 = blockIdx.x * TF;
  if (!ok[b] || k0 >= T) return;  // (uniform)
  const int64_t L10 = rows.l10(b);
  const int kend = min(k0 + TF, T);
  const int *kidx = idx + b * nv_ld;
  const float *__restrict__ yd = y10 + (b * 2 + 1) * y_ld;
  const __amdgpu_buffer_rsrc_t rd = row_rsrc(yd, (uint32_t)(L10 * 4));  // the row's [0, L10) (sample_at)
  float win[4];
  hann_quad(lane, win);
  // overlap-added blocks q = k0 + 1 .. kend + 1 of the denoised row
  const int nblk = kend - k0 + 1;
  for (int j = wave; j < nblk; j += TGW) {
    float g[4];
    ola_taps(rd, kidx, k0 + 1 + j, lane, g);
    blk[j][lane] = ola_block(win, g, 0);
    blk[j][64 + lane] = ola_block(win, g, 1);
  }
  // gY / Y per (frame, band): a frame's derivative is the sum of the at most two tiles it lies in
  const int nwb = (S + GW - 1) / GW;
  for (int e = tid; e < TF * 16; e += 64 * TGW) {
    const int fr = e >> 4, j = e & 15;
    const int t = k0 + fr;
    float val = 0.f;
    if (j < NB && t < kend) {
      const float Y = tob[((b + B) * NB + j) * tmax + t];
      const int w1 = t / GW, off = t % GW;
      float s = 0.f;
      if (w1 >= 1 && w1 - 1 < nwb && off + GW < GFR) s = gyw[((b * NW + w1 - 1) * NB + j) * GLD + off + GW];
      if (w1 < nwb) s += gyw[((b * NW + w1) * NB + j) * GLD + off];
      val = Y > 0.f ? s / Y : 0.f;  // sqrt's subgradient 0 at a zero envelope
    }
    qb[fr][j] = val;
  }
  lds_stores_done();
  lds_barrier();

  cf tw1[8], tw2[8];
  fft512_twiddles(lane, tw1, tw2);
  float2 *wbuf = reinterpret_cast<float2 *>(xbuf) + wave * kFftBuf;
  const int plane = (64 - lane) & 63;
  int band[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = lane + 64 * r;
    band[r] = 15;  // (qb[.][15] = 0: a bin in no band)
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if (k >= kObmEdge[j][0] && k < kObmEdge[j][1]) band[r] = j;
  }
  const int nfr = kend - k0;
  for (int p = wave; 2 * p < nfr; p += TGW) {
    const int ja = 2 * p;  // frames a = k0 + ja = [block_ja, block_ja+1] * w and b = a + 1 in one transform
    const bool has_b = ja + 1 < nfr;
    cf v[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = lane + 64 * (r & 1);
      const float a = blk[ja + (r >> 1)][t];
      const float bq = has_b ? blk[ja + 1 + (r >> 1)][t] : 0.f;
      v[r] = {a * win[r], bq * win[r]};
    }
#pragma unroll
    for (int r = 4; r < 8; ++r) v[r] = {0.f, 0.f};
    // frames far apart in level are equalised first, exactly as the forward does (pair_level_shift)
    int ea, eb;
    pair_peaks(v, ea, eb);
    const float b_scale = __builtin_amdgcn_ldexpf(0.25f, -pair_level_shift(v, ea, eb));
    fft512_wave<true>(v, wbuf, lane, tw1, tw2);
    // Za = (Z[k] + conj Z[N-k]) / 2, Zb = (Z[k] - conj Z[N-k]) / 2i; G = (gY / Y) Z per frame;
    // W[k] = conj(Ga + i Gb) / 2 and W[N-k] = conj(conj Ga + i conj Gb) / 2: the transform of W is the
    // conjugate of ga + i gb, the derivatives with respect to both frames' samples
    cf u[8];
    pair_grad_fold(
        v,
        [&](int r, float &ca, float &cb) {
          ca = 0.25f * qb[ja][band[r]];
          cb = has_b ? b_scale * qb[ja + 1][band[r]] : 0.f;
        },
        lane, plane, u);
    fft512_wave<false>(u, wbuf, lane, tw1, tw2);
    float *fa = gf + ((int64_t)b * tmax + k0 + ja) * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      fa[lane + 64 * r] = win[r] * u[r].r;
      if (has_b) fa[256 + lane + 64 * r] = -win[r] * u[r].i;
    }
    wave_lds_fence();
  }
}

// 10 kHz sample o = 128 c + s of row b: block q = w_lo F_iq[0:128] + w_hi F_iq-1[128:256] and STFT frame t
// = [block t+1, block t+2], so the sample collects w_lo[s] gblk_q[s] for the kept frame q that starts
// at c and w_hi[s] gblk_q'+1[s] for the kept frame q' that starts at c - 1, with gblk_q = gf[q-1][0:128] +
// gf[q-2][128:256].  256 samples (two frames' starts) per workgroup.
__global__ void __launch_bounds__(256)
    stoi_ola_grad(const float *__restrict__ gf, int64_t tmax, Rows rows, const int *__restrict__ kpos,
                  const int *__restrict__ kept, int nv_ld, const int *__restrict__ ok, float *__restrict__ out,
                  int64_t out_ld, int64_t ncols, int64_t b0) {
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int64_t o = (int64_t)blockIdx.x * 256 + tid;
  const int64_t L10 = rows.l10(b);
  float *__restrict__ row = out + b * out_ld;
  if (!ok[b] || (int64_t)blockIdx.x * 256 >= L10) {  // (uniform)
    if (o < ncols) row[o] = 0.f;
    return;
  }
  const int n = kept[b], T = n - 2;
  if (o >= ncols) return;
  float r = 0.f;
  if (o < L10) {
    const int s = tid & 127, h = tid >> 7;
    const float *g = gf + (int64_t)b * tmax * 256;
    auto gblk = [&](int q) {
      float a = 0.f;
      if (q - 1 >= 0 && q - 1 < T) a = g[(int64_t)(q - 1) * 256 + s];
      if (q - 2 >= 0 && q - 2 < T) a += g[(int64_t)(q - 2) * 256 + 128 + s];
      return a;
    };
    const int c = blockIdx.x * 2 + h;  // the VAD frame that starts at this sample's 128-sample chunk
    const int *__restrict__ pr = kpos + b * nv_ld;  // (stoi_grad_rows' table)
    const int q = c < nv_ld ? pr[c] : -1, qp = (c >= 1 && c - 1 < nv_ld) ? pr[c - 1] : -1;
    if (q >= 0) r = kHann256s[s] * gblk(q);
    if (qp >= 0) r += kHann256s[128 + s] * gblk(qp + 1);
  }
  row[o] = r;
}

// grad[b, i] = sum_o K[o mod nw][i - first(o)] g10[b, o] over the row's 10 kHz samples o = m nw + j whose
// taps reach input sample i (first(o) = m orig - width), m then j ascending; 0 from the row's end on.
__global__ void __launch_bounds__(256)
    stoi_resample_grad(const float *__restrict__ g10, int64_t y_ld, Rows rows, const int *__restrict__ ok,
                       float *__restrict__ grad, int64_t grad_ld, int64_t length, int64_t b0, ResampleKernel rk) {
  __shared__ float ks[FSEM_RS_MAX_COEF];
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int orig = rk.orig, nw = rk.nw, taps = rk.taps, width = rk.width;
  if (!rk.big)
    for (int i = tid; i < nw * taps; i += 256) ks[i] = rk.k[i];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  if (i >= length) return;
  const int64_t n = rows.n(b);
  float acc = 0.f;
  if (ok[b] && i < n) {
    const int64_t L10 = rows.l10(b);
    const float *__restrict__ g = g10 + b * y_ld;
    const int64_t num = i + width - taps + 1;
    const int64_t m_lo = num <= 0 ? 0 : (num + orig - 1) / orig;
    const int64_t m_hi = (i + width) / orig;
    for (int64_t m = m_lo; m <= m_hi; ++m) {
      const int t = (int)(i - (m * orig - width));
      for (int j = 0; j < nw; ++j) {
        const int64_t o = m * nw + j;
        if (o < L10) acc = fmaf(rk.big ? sinc_coef(j, t, orig, nw, width) : ks[j * taps + t], g[o], acc);
      }
    }
  }
  grad[b * grad_ld + i] = acc;
}

// 16 -> 10 kHz (the compile-time kernel kRs16k10k, 8 inputs per 5 outputs): one lane per polyphase group q
// = input samples 8 q .. 8 q + 7, which the taps of the output groups q - 2 .. q + 2 reach (t = r - 8 dm + 10 in
// 0 .. 27).  The workgroup's 1300 derivatives are staged in LDS (zeros outside the row's [0, L10)); the 25 of a
// lane sit 5 floats from its neighbour's (an odd stride: no bank conflicts).  Same terms in the same order as
// stoi_resample_grad (groups, then phases, ascending), so the same values.
template <bool VEC>
__global__ void __launch_bounds__(256)
    stoi_resample_grad16(const float *__restrict__ g10, int64_t y_ld, Rows rows, const int *__restrict__ ok,
                         float *__restrict__ grad, int64_t grad_ld, int64_t length, int64_t b0) {
  constexpr int NT = 5 * (256 + 4);
  __shared__ float gs[NT];
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int64_t q0 = (int64_t)blockIdx.x * 256;
  const int64_t n = rows.n(b);
  const bool live = ok[b] != 0 && 8 * q0 < n;  // (uniform)
  if (live) {
    const int64_t L10 = rows.l10(b);
    const float *__restrict__ g = g10 + b * y_ld;
    const int64_t o0 = 5 * (q0 - 2);
    for (int k = tid; k < NT; k += 256) {
      const int64_t o = o0 + k;
      gs[k] = (o >= 0 && o < L10) ? g[o] : 0.f;
    }
    __syncthreads();
  }
  const int64_t i0 = 8 * (q0 + tid);
  if (i0 >= length) return;
  float acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = 0.f;
  if (live) {
    float v[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) v[k] = gs[5 * tid + k];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
      for (int dm = -2; dm <= 2; ++dm) {
        const int t = r - 8 * dm + 10;
        if (t >= 0 && t < 28) {
#pragma unroll
          for (int j = 0; j < 5; ++j) acc[r] = fmaf(kRs16k10k[j][t], v[5 * (dm + 2) + j], acc[r]);
        }
      }
      if (i0 + r >= n) acc[r] = 0.f;
    }
  }
  float *__restrict__ out = grad + b * grad_ld + i0;
  if (VEC && i0 + 8 <= length) {
    reinterpret_cast<float4 *>(out)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    reinterpret_cast<float4 *>(out)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r)
      if (i0 + r < length) out[r] = acc[r];
  }
}

static int run_grad(const float *deg, int64_t B, int64_t length, int64_t ld, const int32_t *lengths, int32_t sr,
                    const Geometry &g, const ResampleKernel &rk, const State &s, const float *g_stoi,
                    const float *g_estoi, float *grad, int64_t grad_ld, hipStream_t st) {
  const Rows rows{lengths, length, rk.orig, rk.nw};
  const Ws &w = s.fwd;
  const GradWs &q = s.bwd;
  const int NW = seg_waves(g.tmax);
  hipLaunchKernelGGL(stoi_grad_rows, dim3((unsigned)B), dim3(256), 0, st, deg, ld, rows, w.idx, w.kept,
                     g.nv_ld, q.ok, q.pos);
  FSEM_CHECK_LAUNCH();
  for (int64_t b0 = 0; b0 < B; b0 += kMaxGridY) {
    hipLaunchKernelGGL(stoi_seg_grad, grid_slice((unsigned)NW, B, b0), dim3(GW), 0, st, w.tob, B, (int64_t)g.tmax,
                       w.kept, q.ok, g_stoi, g_estoi, q.gyw, NW, b0);
    FSEM_CHECK_LAUNCH();
    hipLaunchKernelGGL(stoi_tob_grad, grid_slice((unsigned)((g.tmax + TF - 1) / TF), B, b0), dim3(64 * TGW), 0, st,
                       w.y10, g.y_ld, B, rows, w.idx, w.kept, g.nv_ld, w.tob, (int64_t)g.tmax, q.ok, q.gyw, NW, q.gf,
                       b0);
    FSEM_CHECK_LAUNCH();
    // at 10 kHz the 10 kHz row is the input row: the gradient itself, zeros from the row's end on
    float *out = g.direct ? grad : q.g10;
    const int64_t out_ld = g.direct ? grad_ld : g.y_ld;
    hipLaunchKernelGGL(stoi_ola_grad, grid_slice((unsigned)((g.L10 + 255) / 256), B, b0), dim3(256), 0, st, q.gf,
                       (int64_t)g.tmax, rows, q.pos, w.kept, g.nv_ld, q.ok, out, out_ld, g.L10, b0);
    FSEM_CHECK_LAUNCH();
    if (g.mode == 0) {
      const dim3 grid16 = grid_slice((unsigned)((length + 2047) / 2048), B, b0);
      if ((uintptr_t)grad % 16 == 0 && grad_ld % 4 == 0)
        hipLaunchKernelGGL(stoi_resample_grad16<true>, grid16, dim3(256), 0, st, q.g10, g.y_ld, rows, q.ok, grad,
                           grad_ld, length, b0);
      else
        hipLaunchKernelGGL(stoi_resample_grad16<false>, grid16, dim3(256), 0, st, q.g10, g.y_ld, rows, q.ok, grad,
                           grad_ld, length, b0);
      FSEM_CHECK_LAUNCH();
    } else if (!g.direct) {
      hipLaunchKernelGGL(stoi_resample_grad, grid_slice((unsigned)((length + 255) / 256), B, b0), dim3(256), 0, st,
                         q.g10, g.y_ld, rows, q.ok, grad, grad_ld, length, b0, rk);
      FSEM_CHECK_LAUNCH();
    }
  }
  return FSEM_OK;
}

}  // namespace stoi
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_stoi_state_floats(int64_t batch, int64_t length, int32_t sample_rate) {
  if (batch < 0 || length <= 0 || length > kMaxLength) return 0;
  stoi::Geometry g;
  ResampleKernel rk;
  if (stoi::make_geometry(length, sample_rate, &g, &rk) != FSEM_OK) return 0;
  return (int64_t)(layout_bytes(stoi::state_layout, batch > 0 ? batch : 1, g) / sizeof(float));
}

extern "C" int fsem_stoi_state_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                   const int32_t *lengths, int32_t sample_rate, float *stoi_out, float *estoi_out,
                                   int32_t *segments, float *state, void *stream) {
  if (!ref || !deg || !stoi_out || !estoi_out || !state || batch < 0 || length <= 0 || ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  stoi::Geometry g;
  ResampleKernel rk;
  const int rc = stoi::make_geometry(length, sample_rate, &g, &rk);
  if (rc != FSEM_OK) return rc;
  if (batch == 0) return FSEM_OK;
  const int rs = stoi::run(ref, deg, batch, length, ld, lengths, sample_rate, stoi_out, estoi_out, nullptr, nullptr, 0,
                           state, layout_bytes(stoi::state_layout, batch, g), (hipStream_t)stream);
  if (rs != FSEM_OK || !segments) return rs;
  Arena a(state);
  const stoi::State s = stoi::state_layout(a, batch, g);
  hipLaunchKernelGGL(stoi::stoi_segments, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     s.fwd.kept, batch, segments);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}

extern "C" int fsem_stoi_grad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                                  int32_t sample_rate, float *state, const float *g_stoi, const float *g_estoi,
                                  float *grad, int64_t grad_ld, void *stream) {
  if (!deg || !state || !g_stoi || !g_estoi || !grad || batch < 0 || length <= 0 || ld < length || grad_ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  stoi::Geometry g;
  ResampleKernel rk;
  const int rc = stoi::make_geometry(length, sample_rate, &g, &rk);
  if (rc != FSEM_OK) return rc;
  if (batch == 0) return FSEM_OK;
  Arena a(state);
  const stoi::State s = stoi::state_layout(a, batch, g);
  return stoi::run_grad(deg, batch, length, ld, lengths, sample_rate, g, rk, s, g_stoi, g_estoi, grad, grad_ld,
                        (hipStream_t)stream);
}
