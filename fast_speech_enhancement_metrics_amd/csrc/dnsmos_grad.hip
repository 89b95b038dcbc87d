// DNSMOS with gradients (include/fsem.h, "DNSMOS with gradients"): the gradient of
// L = sum_b sum_k g[b][k] score_k(b) with respect to the 16 kHz rows.  In libfsem.so: libfsem_dnsmos.so's
// entry set is pinned.  Nothing is kept from the forward call: each pass of P segments is recomputed with
// the forward's own kernels (fsem_dnsmos_kernels.h, REC set: re and im of the front end, the pool winners and
// the positions of conv7's block maxima are left in the pass's scratch), then its adjoint runs, pass after
// pass on the stream.
//
//   dn_dense_grad  one block per segment.  The dense layers again (dense_forward, the forward's), the seed
//                  g[b][k] (c1_k + 2 c2_k r_k) / S_b, the three dense layers transposed in float32 (ReLU
//                  masks h > 0), and for each of conv7's 64 channels the first position that attains the
//                  maximum (nothing when the maximum is 0).  The 64 values are scaled by the power of two
//                  that puts the largest magnitude into [8, 16): the f16 gradients of the convolutions keep
//                  clear of f16's subnormals whatever the seed's size; the inverse goes to inv[segment].
//                  A zero or non-finite seed, or a flagged segment, marks the segment skipped: every later
//                  kernel returns on it and it adds nothing to its row.
//   dn_dconv       the data gradient of conv7 ... conv2: the forward's implicit GEMM (16 x 16 pixel tile,
//                  18 x 18 halo in LDS, wave w owns four rows of the tile, v_mfma_f32_16x16x32_f16, float32
//                  accumulation) with C_in and C_out exchanged and the weights packed flipped and
//                  transposed, [2 - ky, 2 - kx][C_in][C_out].  The loader forms the pre-activation gradient
//                  while staging: conv7's from the 64 scaled values and their positions; a pooled layer's
//                  from the half-resolution gradient, the recorded winner and the pooled activation (the
//                  value at the winning position where the activation is positive, 0 elsewhere and in the
//                  row and column the pooling's floor dropped); conv3's and conv2's from the full-resolution
//                  gradient where the recomputed f16 activation is positive.  Epilogue: the f16 gradient,
//                  no bias, no ReLU.  conv2's (128 channels at 900 x 161) is not stored: the epilogue
//                  recomputes conv1's pre-activation for the mask (nine FMAs from the image, the forward
//                  loader's order) and contracts the pixel's 128 channels with w1 into nine float32
//                  partials (in-lane over the eight fragments, then the 16 lanes of the accumulator's
//                  channel index by DPP adds: one order).
//   dn_gather      image gradient [900][161]: the nine partials of the neighbouring pixels, taps in
//                  ascending order, times the inverse scale (a power of two: exact).
//   dn_front_grad  grid (57 blocks of 16 frames, segment), 320 threads.  g_p = g_img / (p ln 10) where
//                  p > 1e-12, g_re = 2 re g_p, g_im = 2 im g_p in double into LDS; thread j owns frame
//                  sample j and sums over the bins in ascending order, in double.
//   dn_rows_grad   one thread per row sample u < n: for each segment of its row in the pass, in ascending
//                  order, the sum in double over the segment positions t = u - 16000 s (mod n), ascending,
//                  of the two frames that cover t (the earlier frame first), added onto grad[u] with one
//                  float32 rounding per segment.  A pass boundary stores and reloads that float32, so the
//                  result does not depend on P.  No atomics.
#include "fsem_dnsmos_kernels.h"

namespace fsem {
namespace dnsmos {

struct GBlob {
  Blob f;           // the forward's blob
  float *re, *im;   // [161][320], the checkpoint's layout
  _Float16 *gw[6];  // conv2 ... conv7: [8 - tap][Cin][Cout]
};
inline GBlob gblob_layout(Arena &a) {
  GBlob g;
  g.f = blob_layout(a);
  g.re = a.take<float>(NB * FL);
  g.im = a.take<float>(NB * FL);
  for (int l = 0; l < 6; ++l) g.gw[l] = a.take<_Float16>((size_t)9 * kCin[l] * kCout[l]);
  return g;
}

struct GWs {
  Ws w;
  Rec rec;
  int *rowflag;  // [batch]
  int *skip;     // [P]
  double *inv;   // [P] the inverse of the segment's scale
  float *g7;     // [P][64] scaled gradient at conv7's maxima
  int *i7;       // [P][64] their positions
  _Float16 *g6, *g5, *g4, *g3, *g2;  // with respect to a6, a5, a4, conv3's output, conv2's output
  float *part;   // [P][900][161][9]
  float *gimg;   // [P][900][161]
  double *gx;    // [P][900][320] frame-sample gradients
};
inline GWs glayout(Arena &a, int64_t batch, int P) {
  GWs g;
  const size_t p = (size_t)P;
  g.w = layout(a, P);
  g.rec.reim = a.take<float>(p * 2 * NF * NB);
  g.rec.win4 = a.take<uint8_t>(p * H2 * W2 * 32);
  g.rec.win5 = a.take<uint8_t>(p * H3 * W3 * 32);
  g.rec.win6 = a.take<uint8_t>(p * H4 * W4 * 32);
  g.rec.pidx = a.take<int>(p * NB7 * 64);
  g.rowflag = a.take<int>((size_t)batch);
  g.skip = a.take<int>(p);
  g.inv = a.take<double>(p);
  g.g7 = a.take<float>(p * 64);
  g.i7 = a.take<int>(p * 64);
  g.g6 = a.take<_Float16>(p * H4 * W4 * 32);
  g.g5 = a.take<_Float16>(p * H3 * W3 * 32);
  g.g4 = a.take<_Float16>(p * H2 * W2 * 32);
  g.g3 = a.take<_Float16>(p * H1 * W1 * 64);
  g.g2 = a.take<_Float16>(p * H1 * W1 * 64);
  g.part = a.take<float>(p * H1 * W1 * 9);
  g.gimg = a.take<float>(p * H1 * W1);
  g.gx = a.take<double>(p * NF * FL);
  return g;
}

__global__ void pack_gconv(const float *__restrict__ src, _Float16 *__restrict__ dst, int cout, int cin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * cout * cin) return;
  const int co = i % cout, ci = (i / cout) % cin, tap = i / (cin * cout);
  dst[i] = (_Float16)src[(co * cin + ci) * 9 + 8 - tap];
}

// grad[b][0 .. length) = 0 for every row (rowflag null) or for the flagged rows
__global__ __launch_bounds__(256) void dn_zero_rows(float *__restrict__ grad, int64_t ldg, int64_t batch,
                                                    int64_t length, const int *__restrict__ rowflag) {
  const int64_t total = batch * length;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total; v += (int64_t)gridDim.x * 256) {
    const int64_t b = v / length, u = v - b * length;
    if (!rowflag || rowflag[b]) grad[b * ldg + u] = 0.f;
  }
}
__global__ __launch_bounds__(256) void dn_zero_flags(int *__restrict__ rowflag, int64_t batch) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b < batch) rowflag[b] = 0;
}

// ---- the dense layers' adjoint
__global__ __launch_bounds__(128) void dn_dense_grad(const float *__restrict__ pmax, const int *__restrict__ pidx,
                                                     const SegMap *__restrict__ map, const int *__restrict__ segflag,
                                                     Blob b, const float *__restrict__ g_scores,
                                                     float *__restrict__ g7, int *__restrict__ i7,
                                                     int *__restrict__ skip, double *__restrict__ inv,
                                                     int *__restrict__ rowflag) {
  __shared__ float h0[64], h1[128], h2[64], gr[3], t2[64], t1[128], t0[64];
  __shared__ float scale;
  const int i = blockIdx.x, tid = threadIdx.x;
  const SegMap m = map[i];
  if (m.row < 0) return;
  const float r = dense_forward(pmax, b, i, h0, h1, h2);
  if (tid < 3)
    gr[tid] = (float)((double)g_scores[(int64_t)m.row * 3 + tid] *
                      ((double)kPoly1[tid] + 2.0 * (double)kPoly2[tid] * (double)r) / (double)m.S);
  __syncthreads();
  if (tid < 64) {
    float v = 0.f;
    for (int k = 0; k < 3; ++k) v = fmaf(b.d3w[k * 64 + tid], gr[k], v);
    t2[tid] = h2[tid] > 0.f ? v : 0.f;
  }
  __syncthreads();
  {
    float v = 0.f;
    for (int j = 0; j < 64; ++j) v = fmaf(b.d2w[j * 128 + tid], t2[j], v);
    t1[tid] = h1[tid] > 0.f ? v : 0.f;
  }
  __syncthreads();
  if (tid < 64) {
    float v = 0.f;
    for (int j = 0; j < 128; ++j) v = fmaf(b.d1w[j * 64 + tid], t1[j], v);
    t0[tid] = h0[tid] > 0.f ? v : 0.f;  // (nothing when the maximum is 0)
    const float *__restrict__ p = pmax + (size_t)i * NB7 * 64 + tid;
    const int *__restrict__ q = pidx + (size_t)i * NB7 * 64 + tid;
    int ix = 0x7fffffff;
    for (int k = 0; k < NB7; ++k)
      if (p[k * 64] == h0[tid] && q[k * 64] < ix) ix = q[k * 64];
    i7[i * 64 + tid] = ix;
  }
  __syncthreads();
  if (tid == 0) {
    float mx = 0.f;
    bool finite = true;
    for (int c = 0; c < 64; ++c) {
      mx = fmaxf(mx, fabsf(t0[c]));
      finite &= isfinite(t0[c]);
    }
    const bool flagged = segflag[i] != 0;
    const bool ok = finite && mx > 0.f && !flagged;
    int e = 0;
    frexpf(mx, &e);  // mx = f 2^e, f in [0.5, 1): mx 2^(4 - e) lies in [8, 16)
    int k = 4 - e;
    k = k > 100 ? 100 : k;
    scale = ok ? ldexpf(1.f, k) : 0.f;
    inv[i] = ok ? ldexp(1.0, -k) : 0.0;
    skip[i] = ok ? 0 : 1;
    if (flagged) rowflag[m.row] = 1;  // (every writer writes 1)
  }
  __syncthreads();
  if (tid < 64) g7[i * 64 + tid] = t0[tid] * scale;
}

// ---- data gradient of a 3 x 3 convolution, padding 1
enum { LD_SPARSE = 0, LD_POOL = 1, LD_RELU = 2 };
enum { EP_STORE = 0, EP_CONV1 = 1 };

__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror
  return v;
}

// CR: the channels summed over (the convolution's C_out); CO: the channels produced (its C_in).  H x W is
// the layer's map, the same for the gradient read and the gradient written.
//   LD_SPARSE  g7, i7: 64 values per segment and their positions (conv7)
//   LD_POOL    gin, act, win [segment][H / 2][W / 2][CR]: gradient at the pooled output, pooled activation, winner
//   LD_RELU    gin, act [segment][H][W][CR]: gradient at the layer's output, the output
//   EP_STORE   out [segment][H][W][CO] f16
//   EP_CONV1   part [segment][H][W][9] float32 (CO = 128 = conv1's channels; img the segment's image)
template <int CR, int CO, int LOAD, int EPI>
__global__ __launch_bounds__(256) void dn_dconv(const _Float16 *__restrict__ gin, const _Float16 *__restrict__ act,
                                                const uint8_t *__restrict__ win, const float *__restrict__ g7,
                                                const int *__restrict__ i7, const _Float16 *__restrict__ wgt,
                                                _Float16 *__restrict__ out, const float *__restrict__ img,
                                                const float *__restrict__ w1, const float *__restrict__ b1,
                                                float *__restrict__ part, const SegMap *__restrict__ map,
                                                const int *__restrict__ skip, int H, int W) {
  constexpr int RW = TH / 4;
  constexpr int PS = CR + 8;  // (the forward's padding)
  constexpr int NFR = CO / 16;
  constexpr int VP = CR / 8;
  static_assert(CR <= 64 && CR % 32 == 0, "one phase over the summed channels");
  static_assert(EPI != EP_CONV1 || CO == 128, "the fused epilogue contracts conv1's 128 channels");
  __shared__ __attribute__((aligned(16))) _Float16 tile[HH * HW * PS];
  __shared__ float simg[EPI == EP_CONV1 ? HH * HW : 1];
  const int seg = blockIdx.z;
  if (map[seg].row < 0 || skip[seg]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int m = lane & 15, kq = lane >> 4;
  const int r0 = RW * wave;
  if (EPI == EP_CONV1) {
    const float *__restrict__ im = img + (size_t)seg * H * W;
    for (int v = tid; v < HH * HW; v += 256) {
      const int y = y0 - 1 + v / HW, x = x0 - 1 + v % HW;
      simg[v] = (y >= 0 && y < H && x >= 0 && x < W) ? im[y * W + x] : 0.f;
    }
  }
  if (LOAD == LD_SPARSE) {
    for (int v = tid; v < HH * HW * PS / 8; v += 256) reinterpret_cast<uint4 *>(tile)[v] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (tid < CR) {
      const int ix = i7[seg * 64 + tid];
      if (ix < H * W) {  // (ix >= 0)
        const int hy = ix / W - y0 + 1, hx = ix % W - x0 + 1;
        if (hy >= 0 && hy < HH && hx >= 0 && hx < HW) tile[(hy * HW + hx) * PS + tid] = (_Float16)g7[seg * 64 + tid];
      }
    }
  } else if (LOAD == LD_POOL) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t base = (size_t)seg * Ho * Wo * CR;
    for (int v = tid; v < HH * HW * VP; v += 256) {
      const int pix = v / VP, cv = v % VP;
      const int y = y0 + pix / HW - 1, x = x0 + pix % HW - 1;
      half8 res = {0, 0, 0, 0, 0, 0, 0, 0};
      if (y >= 0 && y < 2 * Ho && x >= 0 && x < 2 * Wo) {  // (the row and column the floor dropped stay 0)
        const size_t off = base + ((size_t)(y >> 1) * Wo + (x >> 1)) * CR + cv * 8;
        const half8 g = *reinterpret_cast<const half8 *>(gin + off);
        const half8 a = *reinterpret_cast<const half8 *>(act + off);
        const uint2 wv = *reinterpret_cast<const uint2 *>(win + off);
        const unsigned sel = (unsigned)((y & 1) * 2 + (x & 1));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned wb = ((e < 4 ? wv.x : wv.y) >> (8 * (e & 3))) & 0xffu;
          res[e] = (wb == sel && a[e] > (_Float16)0) ? g[e] : (_Float16)0;
        }
      }
      *reinterpret_cast<half8 *>(tile + pix * PS + cv * 8) = res;
    }
  } else {
    const size_t base = (size_t)seg * H * W * CR;
    for (int v = tid; v < HH * HW * VP; v += 256) {
      const int pix = v / VP, cv = v % VP;
      const int y = y0 + pix / HW - 1, x = x0 + pix % HW - 1;
      half8 res = {0, 0, 0, 0, 0, 0, 0, 0};
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const size_t off = base + ((size_t)y * W + x) * CR + cv * 8;
        const half8 g = *reinterpret_cast<const half8 *>(gin + off);
        const half8 a = *reinterpret_cast<const half8 *>(act + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) res[e] = a[e] > (_Float16)0 ? g[e] : (_Float16)0;
      }
      *reinterpret_cast<half8 *>(tile + pix * PS + cv * 8) = res;
    }
  }
  __syncthreads();

  float4v acc[RW][NFR];
#pragma unroll
  for (int mi = 0; mi < RW; ++mi)
#pragma unroll
    for (int nf = 0; nf < NFR; ++nf) acc[mi][nf] = (float4v){0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int tap = ky * 3 + kx;
#pragma unroll
      for (int kc = 0; kc < CR / 32; ++kc) {
        half8 a[RW], b[NFR];
#pragma unroll
        for (int mi = 0; mi < RW; ++mi)
          a[mi] = *reinterpret_cast<const half8 *>(tile + ((r0 + mi + ky) * HW + m + kx) * PS + kc * 32 + kq * 8);
#pragma unroll
        for (int nf = 0; nf < NFR; ++nf)
          b[nf] = *reinterpret_cast<const half8 *>(wgt + ((size_t)(tap * CO + nf * 16 + m) * CR + kc * 32 + kq * 8));
#pragma unroll
        for (int mi = 0; mi < RW; ++mi)
#pragma unroll
          for (int nf = 0; nf < NFR; ++nf)
            acc[mi][nf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[mi], b[nf], acc[mi][nf], 0, 0, 0);
      }
    }
  }

  // the accumulator: channel nf 16 + (lane & 15); pixel (row y0 + r0 + mi, column x0 + 4 (lane >> 4) + reg)
  if (EPI == EP_STORE) {
    _Float16 *__restrict__ dst = out + (size_t)seg * H * W * CO;
#pragma unroll
    for (int nf = 0; nf < NFR; ++nf)
#pragma unroll
      for (int mi = 0; mi < RW; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int y = y0 + r0 + mi, x = x0 + 4 * kq + r;
          if (y < H && x < W) dst[((size_t)y * W + x) * CO + nf * 16 + m] = (_Float16)acc[mi][nf][r];
        }
  } else {
    // the lane's 4 x 4 pixels read a 6 x 6 patch of the image (simg's origin is (y0 - 1, x0 - 1))
    float pat[RW + 2][6];
#pragma unroll
    for (int a = 0; a < RW + 2; ++a)
#pragma unroll
      for (int c = 0; c < 6; ++c) pat[a][c] = simg[(r0 + a) * HW + 4 * kq + c];
    float p[RW][4][9];
#pragma unroll
    for (int mi = 0; mi < RW; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < 9; ++t) p[mi][r][t] = 0.f;
#pragma unroll
    for (int nf = 0; nf < NFR; ++nf) {
      const int ch = nf * 16 + m;
      float w[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) w[t] = w1[ch * 9 + t];
      const float bc = b1[ch];
#pragma unroll
      for (int mi = 0; mi < RW; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z = bc;  // conv1's pre-activation, the forward loader's order
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) z = fmaf(w[ky * 3 + kx], pat[mi + ky][r + kx], z);
          const float g = z > 0.f ? acc[mi][nf][r] : 0.f;
#pragma unroll
          for (int t = 0; t < 9; ++t) p[mi][r][t] = fmaf(g, w[t], p[mi][r][t]);
        }
    }
    float *__restrict__ dst = part + (size_t)seg * H * W * 9;
#pragma unroll
    for (int mi = 0; mi < RW; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mine = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const float s = row16_sum(p[mi][r][t]);
          mine = m == t ? s : mine;
        }
        const int y = y0 + r0 + mi, x = x0 + 4 * kq + r;
        if (m < 9 && y < H && x < W) dst[((size_t)y * W + x) * 9 + m] = mine;
      }
  }
}

// ---- the image gradient from the nine partials
__global__ __launch_bounds__(256) void dn_gather(const float *__restrict__ part, const SegMap *__restrict__ map,
                                                 const int *__restrict__ skip, const double *__restrict__ inv,
                                                 float *__restrict__ gimg) {
  const int i = blockIdx.y;
  if (map[i].row < 0) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= H1 * W1) return;
  float s = 0.f;
  if (!skip[i]) {
    const int y = v / W1, x = v % W1;
    const float *__restrict__ p = part + (size_t)i * H1 * W1 * 9;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y - ky + 1, xx = x - kx + 1;
        if (yy >= 0 && yy < H1 && xx >= 0 && xx < W1) s += p[((size_t)yy * W1 + xx) * 9 + ky * 3 + kx];
      }
    s = (float)((double)s * inv[i]);
  }
  gimg[(size_t)i * H1 * W1 + v] = s;
}

// ---- the front end's adjoint
__global__ __launch_bounds__(FL) void dn_front_grad(const float *__restrict__ gimg, const float *__restrict__ reim,
                                                    const SegMap *__restrict__ map, const int *__restrict__ skip,
                                                    const float *__restrict__ wre, const float *__restrict__ wim,
                                                    double *__restrict__ gx) {
  __shared__ double gre[FB * NB], gim[FB * NB];
  const int i = blockIdx.y;
  if (map[i].row < 0 || skip[i]) return;
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * FB;
  const float *__restrict__ re = reim + (size_t)i * 2 * NF * NB;
  const float *__restrict__ g = gimg + (size_t)i * NF * NB;
  for (int v = tid; v < FB * NB; v += FL) {
    const int f = f0 + v / NB, k = v % NB;
    double a = 0.0, c = 0.0;
    if (f < NF) {
      const float r = re[f * NB + k], q = re[NF * NB + f * NB + k];
      const float p = r * r + q * q;
      if (p > 1e-12f) {
        const double gp = (double)g[f * NB + k] / ((double)p * 2.302585092994046);
        a = 2.0 * (double)r * gp;
        c = 2.0 * (double)q * gp;
      }
    }
    gre[v] = a;
    gim[v] = c;
  }
  __syncthreads();
  double acc[FB];
#pragma unroll
  for (int f = 0; f < FB; ++f) acc[f] = 0.0;
  for (int k = 0; k < NB; ++k) {
    const double wr = wre[k * FL + tid], wi = wim[k * FL + tid];
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      acc[f] = fma(wr, gre[f * NB + k], acc[f]);
      acc[f] = fma(wi, gim[f * NB + k], acc[f]);
    }
  }
  double *__restrict__ o = gx + (size_t)i * NF * FL;
#pragma unroll
  for (int f = 0; f < FB; ++f)
    if (f0 + f < NF) o[(size_t)(f0 + f) * FL + tid] = acc[f];
}

// ---- back to the rows
__global__ __launch_bounds__(256) void dn_rows_grad(const double *__restrict__ gx, const SegMap *__restrict__ map,
                                                    const int *__restrict__ skip, int P, float *__restrict__ grad,
                                                    int64_t ldg) {
  const int i = blockIdx.y;
  const SegMap m = map[i];
  if (m.row < 0 || (i > 0 && map[i - 1].row == m.row)) return;  // (the first segment of its row in the pass)
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= m.n) return;
  float *__restrict__ dst = grad + (int64_t)m.row * ldg + u;
  float acc = *dst;
  for (int j = i; j < P && map[j].row == m.row; ++j) {
    if (skip[j]) continue;
    const double *__restrict__ x = gx + (size_t)j * NF * FL;
    int64_t t0 = (u - (int64_t)SHOP * map[j].s) % m.n;
    if (t0 < 0) t0 += m.n;
    double sum = 0.0;
    for (int64_t t = t0; t < SEG; t += m.n) {
      const int f = (int)(t / FH), o = (int)(t - (int64_t)f * FH);
      double v = 0.0;
      if (f >= 1) v = x[(size_t)(f - 1) * FL + o + FH];
      if (f < NF) v += x[(size_t)f * FL + o];
      sum += v;
    }
    acc = (float)((double)acc + sum);
  }
  *dst = acc;
}

template <int CR, int CO, int LOAD, int EPI>
inline void launch_dconv(hipStream_t st, int P, int H, int W, const _Float16 *gin, const _Float16 *act,
                         const uint8_t *win, const GWs &g, const GBlob &b, int l, _Float16 *out) {
  const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH), (unsigned)P);
  hipLaunchKernelGGL((dn_dconv<CR, CO, LOAD, EPI>), grid, dim3(256), 0, st, gin, act, win, g.g7, g.i7, b.gw[l], out,
                     g.w.img, b.f.w1, b.f.b1, g.part, g.w.map, g.skip, H, W);
}

// grad (the rows' gradient) or gimage (the stage entry: [S_total][900][161]) is given, not both.
inline int run_grad(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                    const void *weights, const float *g_scores, float *grad, int64_t ld_grad, float *gimage,
                    float *raw, float *scratch, int64_t pass, void *stream) {
  if (!deg || !weights || !g_scores || !(grad || gimage) || !scratch || batch < 1 || length < 1 || ld < length ||
      length > kMaxLength || pass < 1 || pass > MAXP || (grad && ld_grad < length))
    return FSEM_EINVAL;
  const int P = (int)pass;
  Arena a(scratch);
  const GWs g = glayout(a, batch, P);
  Arena ba(const_cast<void *>(weights));
  const GBlob b = gblob_layout(ba);
  hipStream_t st = (hipStream_t)stream;
  const unsigned zb = (unsigned)(((batch * length + 255) / 256) < (1 << 20) ? (batch * length + 255) / 256 : (1 << 20));
  hipLaunchKernelGGL(dn_zero_flags, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, g.rowflag, batch);
  FSEM_CHECK_LAUNCH();
  if (grad) {
    hipLaunchKernelGGL(dn_zero_rows, dim3(zb), dim3(256), 0, st, grad, ld_grad, batch, length, (const int *)nullptr);
    FSEM_CHECK_LAUNCH();
  }
  const int64_t total = batch * max_segs(length, lengths != nullptr);
  for (int64_t g0 = 0; g0 < total; g0 += P) {
    const int rc = forward_pass<true>(st, deg, batch, length, ld, lengths, b.f, g.w, P, g0, g.w.img, false, raw, g.rec);
    if (rc != FSEM_OK) return rc;
    hipLaunchKernelGGL(dn_dense_grad, dim3((unsigned)P), dim3(128), 0, st, g.w.pmax, g.rec.pidx, g.w.map, g.w.segflag,
                       b.f, g_scores, g.g7, g.i7, g.skip, g.inv, g.rowflag);
    FSEM_CHECK_LAUNCH();
    launch_dconv<64, 32, LD_SPARSE, EP_STORE>(st, P, H4, W4, nullptr, nullptr, nullptr, g, b, 5, g.g6);
    FSEM_CHECK_LAUNCH();
    launch_dconv<32, 32, LD_POOL, EP_STORE>(st, P, H3, W3, g.g6, g.w.a6, g.rec.win6, g, b, 4, g.g5);
    FSEM_CHECK_LAUNCH();
    launch_dconv<32, 32, LD_POOL, EP_STORE>(st, P, H2, W2, g.g5, g.w.a5, g.rec.win5, g, b, 3, g.g4);
    FSEM_CHECK_LAUNCH();
    launch_dconv<32, 64, LD_POOL, EP_STORE>(st, P, H1, W1, g.g4, g.w.a4, g.rec.win4, g, b, 2, g.g3);
    FSEM_CHECK_LAUNCH();
    launch_dconv<64, 64, LD_RELU, EP_STORE>(st, P, H1, W1, g.g3, g.w.a3, nullptr, g, b, 1, g.g2);
    FSEM_CHECK_LAUNCH();
    launch_dconv<64, 128, LD_RELU, EP_CONV1>(st, P, H1, W1, g.g2, g.w.a2, nullptr, g, b, 0, nullptr);
    FSEM_CHECK_LAUNCH();
    float *gi = gimage ? gimage + (size_t)g0 * NF * NB : g.gimg;
    hipLaunchKernelGGL(dn_gather, dim3((H1 * W1 + 255) / 256, (unsigned)P), dim3(256), 0, st, g.part, g.w.map, g.skip,
                       g.inv, gi);
    FSEM_CHECK_LAUNCH();
    if (gimage) continue;
    hipLaunchKernelGGL(dn_front_grad, dim3((NF + FB - 1) / FB, (unsigned)P), dim3(FL), 0, st, g.gimg, g.rec.reim,
                       g.w.map, g.skip, b.re, b.im, g.gx);
    FSEM_CHECK_LAUNCH();
    hipLaunchKernelGGL(dn_rows_grad, dim3((unsigned)((length + 255) / 256), (unsigned)P), dim3(256), 0, st, g.gx,
                       g.w.map, g.skip, P, grad, ld_grad);
    FSEM_CHECK_LAUNCH();
  }
  if (grad) {
    hipLaunchKernelGGL(dn_zero_rows, dim3(zb), dim3(256), 0, st, grad, ld_grad, batch, length, (const int *)g.rowflag);
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}

}  // namespace dnsmos
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_dnsmos_grad_scratch_floats(int64_t batch, int64_t length, int64_t pass) {
  if (batch < 1 || length < 1 || length > kMaxLength || pass < 1 || pass > dnsmos::MAXP) return 0;
  return (int64_t)(layout_bytes(dnsmos::glayout, batch, (int)pass) / sizeof(float));
}

extern "C" int64_t fsem_dnsmos_grad_weights_floats(void) {
  return (int64_t)(layout_bytes(dnsmos::gblob_layout) / sizeof(float));
}

extern "C" int fsem_dnsmos_grad_pack_weights_f32(const float *const *t, float *blob, int64_t blob_floats,
                                                 void *stream) {
  if (!t || !blob) return FSEM_EINVAL;
  for (int i = 0; i < FSEM_DNSMOS_NUM_TENSORS; ++i)
    if (!t[i]) return FSEM_EINVAL;
  Arena a(blob);
  const dnsmos::GBlob b = dnsmos::gblob_layout(a);
  if (blob_floats < 0 || !a.fits((size_t)blob_floats * sizeof(float))) return FSEM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int rc = dnsmos::pack_blob(t, b.f, st);
  if (rc != FSEM_OK) return rc;
  auto blocks = [](int n) { return dim3((unsigned)((n + 255) / 256)); };
  hipLaunchKernelGGL(dnsmos::pack_copy, blocks(dnsmos::NB * dnsmos::FL), dim3(256), 0, st, t[0], b.re,
                     dnsmos::NB * dnsmos::FL);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(dnsmos::pack_copy, blocks(dnsmos::NB * dnsmos::FL), dim3(256), 0, st, t[1], b.im,
                     dnsmos::NB * dnsmos::FL);
  FSEM_CHECK_LAUNCH();
  for (int l = 0; l < 6; ++l) {
    const int cin = dnsmos::kCin[l], cout = dnsmos::kCout[l];
    hipLaunchKernelGGL(dnsmos::pack_gconv, blocks(9 * cin * cout), dim3(256), 0, st, t[4 + 2 * l], b.gw[l], cout, cin);
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}

extern "C" int fsem_dnsmos_grad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld,
                                    const int32_t *lengths, const float *weights, const float *g_scores, float *grad,
                                    int64_t ld_grad, float *raw, float *scratch, int64_t pass, void *stream) {
  if (!grad) return FSEM_EINVAL;
  return dnsmos::run_grad(deg, batch, length, ld, lengths, weights, g_scores, grad, ld_grad, nullptr, raw, scratch,
                          pass, stream);
}

extern "C" int fsem_dnsmos_grad_image_f32(const float *deg, int64_t batch, int64_t length, int64_t ld,
                                          const int32_t *lengths, const float *weights, const float *g_scores,
                                          float *g_image, float *scratch, int64_t pass, void *stream) {
  if (!g_image) return FSEM_EINVAL;
  return dnsmos::run_grad(deg, batch, length, ld, lengths, weights, g_scores, nullptr, 0, g_image, nullptr, scratch,
                          pass, stream);
}
