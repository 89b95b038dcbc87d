// The DNSMOS forward (include/fsem_dnsmos.h): its constants, blob and workspace layouts, kernels and the
// launch sequence of one pass.  Two translation units compile it: dnsmos.hip (libfsem_dnsmos.so, the
// scores) and dnsmos_grad.hip (libfsem.so, which recomputes each pass before its adjoint).  The kernels
// that take REC record, when it is set, what the adjoint needs and the scores do not: re and im of the
// front end, the winner of each pooled element, the position of each block's maximum.  REC changes no
// value the forward computes.
//
// A call is a loop of passes over at most P segments each (at most 16); a segment's work never depends
// on which other segments share its pass.
//
//   dn_map      one block per pass.  The rows' segment counts are summed (256 chunks of rows, a scan over
//               the chunks), and the pass's segments g0 ... g0 + P - 1 get their (row, segment of the
//               row, row length, row's segment count); segments past the batch's last get row = -1 and
//               every later kernel returns on them.  Integers only.  Also clears the pass's flags.
//   dn_front    grid (57 blocks of 16 frames, segment).  The 2720 samples of the 16 frames are read as
//               x[i mod n] into LDS (a non-finite one flags the segment); thread k < 161 owns bin k and
//               sums re and im of the 16 frames over the 320 taps in double, taps in ascending order
//               (the matrices are stored transposed: a wave reads consecutive bins of one tap); then
//               log10(max(re^2 + im^2, 1e-12)).
//   dn_conv     one template for conv2 ... conv7: implicit GEMM with M = a tile of 16 x 16 output pixels,
//               N = C_out, K = 9 C_in on v_mfma_f32_16x16x32_f16.  The block stages the tile's 18 x 18
//               halo of input pixels (NHWC f16, zero outside the image) in LDS; wave w owns output
//               rows 4w ... 4w + 3 of the tile (four 16-pixel A fragments) and every output channel
//               (C_out / 16 B fragments read from the packed weights [tap][C_out][C_in], L1/L2 resident;
//               with two rows per wave the same kernel ran at 208 instead of 280 TFLOP/s: the B reads
//               per MFMA halve).  For conv2 the loader computes conv1 (1 -> 128, float32, ReLU) on the
//               halo from a 20 x 20 patch of the image instead of reading it, 64 channels at a time (two
//               phases over K, so that the halo stays at 46 KiB): conv1's output is never stored.
//               Epilogue: bias + ReLU in float32; the accumulator's four registers are four consecutive
//               columns of one row and the wave's fragments are consecutive rows from an even one, so
//               the 2 x 2 max-pool is a maximum over registers of one lane (tile origins are even;
//               pooled positions past floor(H / 2), floor(W / 2) are not stored).  conv7 instead writes
//               the block's maximum per channel (xor exchanges over the lane's pixel groups, LDS over
//               the waves): 14 x 64 values per segment, no atomics.
//   dn_dense    one block per segment: the maximum over the 14 blocks, the three dense layers in float32
//               (one output per thread, inputs in ascending order), the polynomial.
//   dn_finish   one block per pass: the first segment of each row in the pass adds the row's segments of
//               this pass in double, in order, onto 0 or onto the sums the previous pass left for the
//               row it did not finish (two slots, by the pass's parity), and writes the row's means when
//               its last segment is in the pass.  The order of the additions is the segments' order
//               whatever the pass size.
#pragma once
#include <math.h>

#include "../../include/fsem_dnsmos.h"
#include "fsem_common.h"

namespace fsem {
namespace dnsmos {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int SEG = 144160;  // samples of a segment (9.01 s)
constexpr int SHOP = 16000;  // segment hop
constexpr int NF = 900;      // frames of a segment
constexpr int NB = 161;      // bins
constexpr int FL = 320;      // frame length
constexpr int FH = 160;      // frame hop
constexpr int MAXP = FSEM_DNSMOS_MAX_PASS;
constexpr int FB = 16;       // frames per front-end block
constexpr int FS = (FB - 1) * FH + FL;  // samples of a front-end block
constexpr int TW = 16, TH = 16;         // output tile of a convolution block (columns, rows)
constexpr int HW = TW + 2, HH = TH + 2;
constexpr int H1 = 900, W1 = 161, H2 = 450, W2 = 80, H3 = 225, W3 = 40, H4 = 112, W4 = 20;
constexpr int NB7 = ((W4 + TW - 1) / TW) * ((H4 + TH - 1) / TH);  // conv7's blocks per segment

__host__ __device__ inline int64_t segs_of(int64_t n) {
  if (n < 1) return 0;
  int64_t m = n;
  while (m < SEG) m *= 2;
  return (m - SEG) / SHOP + 1;
}
// The largest segment count of a row of at most `length` samples (a row shorter than a segment has
// up to 10: 144159 samples double to 288318).
inline int64_t max_segs(int64_t length, bool ragged) {
  const int64_t s = segs_of(length);
  return ragged && s < 10 ? 10 : s;
}

struct SegMap {
  int32_t row, s, n, S;
};

struct Blob {
  float *re_t, *im_t;  // [320][161]
  float *w1, *b1;      // [128][9], [128]
  _Float16 *cw[6];     // conv2 ... conv7: [9][Cout][Cin]
  float *cb[6];
  float *d1w, *d1b, *d2w, *d2b, *d3w, *d3b;
};
constexpr int kCin[6] = {128, 64, 64, 32, 32, 32};
constexpr int kCout[6] = {64, 64, 32, 32, 32, 64};
inline Blob blob_layout(Arena &a) {
  Blob b;
  b.re_t = a.take<float>(FL * NB);
  b.im_t = a.take<float>(FL * NB);
  b.w1 = a.take<float>(128 * 9);
  b.b1 = a.take<float>(128);
  for (int l = 0; l < 6; ++l) {
    b.cw[l] = a.take<_Float16>((size_t)9 * kCin[l] * kCout[l]);
    b.cb[l] = a.take<float>(kCout[l]);
  }
  b.d1w = a.take<float>(128 * 64);
  b.d1b = a.take<float>(128);
  b.d2w = a.take<float>(64 * 128);
  b.d2b = a.take<float>(64);
  b.d3w = a.take<float>(3 * 64);
  b.d3b = a.take<float>(3);
  return b;
}

struct Ws {
  SegMap *map;
  int *segflag;
  double *carry;  // [2][4]
  float *img;
  _Float16 *a2, *a3, *a4, *a5, *a6;
  float *pmax, *poly;
};
inline Ws layout(Arena &a, int P) {
  Ws w;
  const size_t p = (size_t)P;
  w.map = a.take<SegMap>(p);
  w.segflag = a.take<int>(p);
  w.carry = a.take<double>(8);
  w.img = a.take<float>(p * H1 * W1);
  w.a2 = a.take<_Float16>(p * H1 * W1 * 64);
  w.a3 = a.take<_Float16>(p * H1 * W1 * 64);
  w.a4 = a.take<_Float16>(p * H2 * W2 * 32);
  w.a5 = a.take<_Float16>(p * H3 * W3 * 32);
  w.a6 = a.take<_Float16>(p * H4 * W4 * 32);
  w.pmax = a.take<float>(p * NB7 * 64);
  w.poly = a.take<float>(p * 3);
  return w;
}

// ---- weights
__global__ void pack_stft(const float *__restrict__ src, float *__restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= FL * NB) return;
  const int j = i / NB, k = i % NB;
  dst[i] = src[k * FL + j];
}
__global__ void pack_conv(const float *__restrict__ src, _Float16 *__restrict__ dst, int cout, int cin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * cout * cin) return;
  const int ci = i % cin, co = (i / cin) % cout, tap = i / (cin * cout);
  dst[i] = (_Float16)src[(co * cin + ci) * 9 + tap];
}
__global__ void pack_copy(const float *__restrict__ src, float *__restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

__global__ void fill_nan(float *__restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = __builtin_nanf("");
}

// ---- the pass's segments
__global__ __launch_bounds__(256) void dn_map(const int32_t *__restrict__ lengths, int length, int64_t batch,
                                              int64_t g0, int P, SegMap *__restrict__ map,
                                              int *__restrict__ segflag) {
  __shared__ int64_t pre[257];
  const int tid = threadIdx.x;
  for (int i = tid; i < P; i += 256) {
    map[i] = {-1, 0, 0, 0};
    segflag[i] = 0;
  }
  const int64_t chunk = (batch + 255) / 256;
  const int64_t b0 = tid * chunk < batch ? tid * chunk : batch;
  const int64_t b1 = b0 + chunk < batch ? b0 + chunk : batch;
  int64_t sum = 0;
  for (int64_t b = b0; b < b1; ++b) sum += segs_of(row_length(lengths, b, length));
  pre[tid + 1] = sum;
  __syncthreads();
  if (tid == 0) {
    pre[0] = 0;
    for (int i = 1; i <= 256; ++i) pre[i] += pre[i - 1];
  }
  __syncthreads();
  int64_t p = pre[tid];
  const int64_t g1 = g0 + P;
  if (p >= g1 || pre[tid + 1] <= g0) return;
  for (int64_t b = b0; b < b1 && p < g1; ++b) {
    const int n = row_length(lengths, b, length);
    const int64_t S = segs_of(n);
    const int64_t lo = p > g0 ? p : g0, hi = p + S < g1 ? p + S : g1;
    for (int64_t g = lo; g < hi; ++g) map[g - g0] = {(int32_t)b, (int32_t)(g - p), n, (int32_t)S};
    p += S;
  }
}

// ---- front end (REC: re and im as float32 into reim [segment][2][900][161])
template <bool REC>
__global__ __launch_bounds__(256) void dn_front(const float *__restrict__ deg, int64_t ld,
                                                const SegMap *__restrict__ map, const float *__restrict__ re_t,
                                                const float *__restrict__ im_t, float *__restrict__ img,
                                                int *__restrict__ segflag, float *__restrict__ reim) {
  __shared__ float smp[FS];
  const int i = blockIdx.y;
  const SegMap m = map[i];
  if (m.row < 0) return;
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * FB;
  const float *__restrict__ x = deg + (int64_t)m.row * ld;
  const int base = m.s * SHOP + f0 * FH;  // < 2^30 + 2^18
  bool bad = false;
  for (int j = tid; j < FS; j += 256) {
    float v = 0.f;
    if (f0 * FH + j < SEG) {
      v = x[(base + j) % m.n];
      bad |= !isfinite(v);
    }
    smp[j] = v;
  }
  if (bad) segflag[i] = 1;  // (every writer writes 1)
  __syncthreads();
  if (tid >= NB) return;
  double re[FB], im[FB];
#pragma unroll
  for (int f = 0; f < FB; ++f) re[f] = im[f] = 0.0;
  for (int j = 0; j < FL; ++j) {
    const double wr = re_t[j * NB + tid], wi = im_t[j * NB + tid];
#pragma unroll
    for (int f = 0; f < FB; ++f) {
      const double v = smp[f * FH + j];
      re[f] = fma(wr, v, re[f]);
      im[f] = fma(wi, v, im[f]);
    }
  }
  float *__restrict__ o = img + (size_t)i * NF * NB;
#pragma unroll
  for (int f = 0; f < FB; ++f) {
    if (f0 + f >= NF) break;
    const float r = (float)re[f], q = (float)im[f];
    const float p = fmaxf(r * r + q * q, 1e-12f);
    o[(f0 + f) * NB + tid] = (float)log10((double)p);
    if (REC) {
      float *__restrict__ ri = reim + (size_t)i * 2 * NF * NB + (f0 + f) * NB + tid;
      ri[0] = r;
      ri[NF * NB] = q;
    }
  }
}

// ---- 3 x 3 convolution, padding 1, + ReLU (+ 2 x 2 max-pool | + the maximum over positions)
// REC: OUT_POOL also writes which of its 2 x 2 inputs each pooled element is (0 ... 3, row-major, the first
// that attains the maximum, taken on the float32 values) into win, laid out as the pooled output; OUT_MAX
// also writes the row-major position y W + x of the first pixel of the block that attains the block's
// maximum into pidx, laid out as pmax.
enum { OUT_STORE = 0, OUT_POOL = 1, OUT_MAX = 2 };

template <int CIN, int COUT, int OUT, bool CONV1, bool REC>
__global__ __launch_bounds__(256) void dn_conv(const _Float16 *__restrict__ in, const float *__restrict__ img,
                                               const float *__restrict__ w1, const float *__restrict__ b1,
                                               const _Float16 *__restrict__ wgt, const float *__restrict__ bias,
                                               _Float16 *__restrict__ out, float *__restrict__ pmax,
                                               const SegMap *__restrict__ map, int H, int W,
                                               uint8_t *__restrict__ win, int *__restrict__ pidx) {
  constexpr int RW = TH / 4;                // output rows of a wave
  constexpr int KS = CIN > 64 ? 64 : CIN;   // input channels staged at a time
  constexpr int NPH = CIN / KS;             // phases over the input channels (2 for conv2)
  constexpr int PS = KS + 8;  // halves per staged pixel: 16 bytes of padding spread the 16 pixels of a fragment over the banks
  constexpr int NFR = COUT / 16;
  static_assert(CONV1 || NPH == 1, "only the fused conv1 loader stages its channels in phases");
  __shared__ __attribute__((aligned(16))) _Float16 tile[HH * HW * PS];
  __shared__ float simg[CONV1 ? (HH + 2) * (HW + 2) : 1];
  __shared__ float red[OUT == OUT_MAX ? 4 * COUT : 1];
  __shared__ int redi[OUT == OUT_MAX && REC ? 4 * COUT : 1];
  const int seg = blockIdx.z;
  if (map[seg].row < 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int m = lane & 15, kq = lane >> 4;
  const int r0 = RW * wave;
  float4v acc[RW][NFR];
#pragma unroll
  for (int mi = 0; mi < RW; ++mi)
#pragma unroll
    for (int nf = 0; nf < NFR; ++nf) acc[mi][nf] = (float4v){0.f, 0.f, 0.f, 0.f};
  if (CONV1) {
    const float *__restrict__ im = img + (size_t)seg * H * W;
    for (int v = tid; v < (HH + 2) * (HW + 2); v += 256) {
      const int y = y0 - 2 + v / (HW + 2), x = x0 - 2 + v % (HW + 2);
      simg[v] = (y >= 0 && y < H && x >= 0 && x < W) ? im[y * W + x] : 0.f;
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int ph = 0; ph < NPH; ++ph) {
    if (CONV1) {
      if (ph) __syncthreads();  // (every wave has read the previous phase's channels)
      const int c = tid % KS, cg = ph * KS + c;
      float w[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) w[t] = w1[cg * 9 + t];
      const float bc = b1[cg];
      for (int pix = tid / KS; pix < HH * HW; pix += 256 / KS) {
        const int hy = pix / HW, hx = pix % HW;
        const int y = y0 + hy - 1, x = x0 + hx - 1;
        float v = 0.f;  // (conv2's zero padding, not conv1 of the padding)
        if (y >= 0 && y < H && x >= 0 && x < W) {
          v = bc;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) v = fmaf(w[ky * 3 + kx], simg[(hy + ky) * (HW + 2) + hx + kx], v);
          v = fmaxf(v, 0.f);
        }
        tile[pix * PS + c] = (_Float16)v;
      }
    } else {
      constexpr int VP = KS / 8;  // 16-byte pieces per pixel
      const _Float16 *__restrict__ src = in + (size_t)seg * H * W * CIN;
      for (int v = tid; v < HH * HW * VP; v += 256) {
        const int pix = v / VP, cv = v % VP;
        const int y = y0 + pix / HW - 1, x = x0 + pix % HW - 1;
        uint4 val = make_uint4(0, 0, 0, 0);
        if (y >= 0 && y < H && x >= 0 && x < W)
          val = *reinterpret_cast<const uint4 *>(src + ((size_t)y * W + x) * CIN + cv * 8);
        *reinterpret_cast<uint4 *>(tile + pix * PS + cv * 8) = val;
      }
    }
    __syncthreads();
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int tap = ky * 3 + kx;
#pragma unroll
        for (int kc = 0; kc < KS / 32; ++kc) {
          half8 a[RW], b[NFR];
#pragma unroll
          for (int mi = 0; mi < RW; ++mi)
            a[mi] = *reinterpret_cast<const half8 *>(tile + ((r0 + mi + ky) * HW + m + kx) * PS + kc * 32 + kq * 8);
#pragma unroll
          for (int nf = 0; nf < NFR; ++nf)
            b[nf] = *reinterpret_cast<const half8 *>(
                wgt + ((size_t)(tap * COUT + nf * 16 + m) * CIN + ph * KS + kc * 32 + kq * 8));
#pragma unroll
          for (int mi = 0; mi < RW; ++mi)
#pragma unroll
            for (int nf = 0; nf < NFR; ++nf)
              acc[mi][nf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[mi], b[nf], acc[mi][nf], 0, 0, 0);
        }
      }
    }
  }

  // the accumulator: channel nf 16 + (lane & 15); pixel (row y0 + r0 + mi, column x0 + 4 (lane >> 4) + reg)
  float vmax[NFR];
  int imax[REC ? NFR : 1];
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) {
    const int ch = nf * 16 + m;
    const float bv = bias[ch];
    float v[RW][4];
#pragma unroll
    for (int mi = 0; mi < RW; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[mi][r] = fmaxf(acc[mi][nf][r] + bv, 0.f);
    if (OUT == OUT_STORE) {
      _Float16 *__restrict__ dst = out + (size_t)seg * H * W * COUT;
#pragma unroll
      for (int mi = 0; mi < RW; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int y = y0 + r0 + mi, x = x0 + 4 * kq + r;
          if (y < H && x < W) dst[((size_t)y * W + x) * COUT + ch] = (_Float16)v[mi][r];
        }
    } else if (OUT == OUT_POOL) {
      const int Ho = H / 2, Wo = W / 2;
      _Float16 *__restrict__ dst = out + (size_t)seg * Ho * Wo * COUT;
#pragma unroll
      for (int p = 0; p < RW / 2; ++p) {
        const int py = (y0 + r0) / 2 + p;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int px = x0 / 2 + 2 * kq + j;
          const float pv = fmaxf(fmaxf(v[2 * p][2 * j], v[2 * p][2 * j + 1]),
                                 fmaxf(v[2 * p + 1][2 * j], v[2 * p + 1][2 * j + 1]));
          if (py < Ho && px < Wo) dst[((size_t)py * Wo + px) * COUT + ch] = (_Float16)pv;
          if (REC && py < Ho && px < Wo) {
            const int wn = v[2 * p][2 * j] == pv ? 0 : v[2 * p][2 * j + 1] == pv ? 1 : v[2 * p + 1][2 * j] == pv ? 2 : 3;
            win[((size_t)seg * Ho * Wo + (size_t)py * Wo + px) * COUT + ch] = (uint8_t)wn;
          }
        }
      }
    } else {
      float mx = 0.f;  // (after ReLU no value is below 0, and every block has a pixel inside the image)
#pragma unroll
      for (int mi = 0; mi < RW; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int y = y0 + r0 + mi, x = x0 + 4 * kq + r;
          if (y < H && x < W) mx = fmaxf(mx, v[mi][r]);
        }
      int ix = 0x7fffffff;
      if (REC) {  // the lane's pixels in ascending row-major order: the first that attains its maximum
#pragma unroll
        for (int mi = RW - 1; mi >= 0; --mi)
#pragma unroll
          for (int r = 3; r >= 0; --r) {
            const int y = y0 + r0 + mi, x = x0 + 4 * kq + r;
            if (y < H && x < W && v[mi][r] == mx) ix = y * W + x;
          }
#pragma unroll
        for (int off = 16; off <= 32; off *= 2) {
          const float om = __shfl_xor(mx, off, 64);
          const int oi = __shfl_xor(ix, off, 64);
          if (om > mx || (om == mx && oi < ix)) ix = oi;
          mx = fmaxf(mx, om);
        }
        imax[nf] = ix;
      } else {
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      }
      vmax[nf] = mx;
    }
  }
  if (OUT == OUT_MAX) {
    if (lane < 16) {
#pragma unroll
      for (int nf = 0; nf < NFR; ++nf) {
        red[wave * COUT + nf * 16 + lane] = vmax[nf];
        if (REC) redi[wave * COUT + nf * 16 + lane] = imax[nf];
      }
    }
    __syncthreads();
    if (tid < COUT) {
      const float mx = fmaxf(fmaxf(red[tid], red[COUT + tid]), fmaxf(red[2 * COUT + tid], red[3 * COUT + tid]));
      const int blk = blockIdx.y * gridDim.x + blockIdx.x;
      pmax[((size_t)seg * (gridDim.x * gridDim.y) + blk) * COUT + tid] = mx;
      if (REC) {
        int ix = 0x7fffffff;
        for (int w = 3; w >= 0; --w)
          if (red[w * COUT + tid] == mx && redi[w * COUT + tid] < ix) ix = redi[w * COUT + tid];
        pidx[((size_t)seg * (gridDim.x * gridDim.y) + blk) * COUT + tid] = ix;
      }
    }
  }
}

// ---- dense layers and the polynomial
// the reference's polynomial (DNSMOS.py:101-103,122)
__device__ constexpr float kPoly0[3] = {0.0052439f, -0.39604546f, 0.04602535f};
__device__ constexpr float kPoly1[3] = {1.22083953f, 1.60915514f, 1.11546468f};
__device__ constexpr float kPoly2[3] = {-0.08397278f, -0.13166888f, -0.06766283f};

// Segment i's dense layers by a block of 128 threads: h0 [64] (the maximum over the blocks), h1 [128],
// h2 [64] in LDS (complete for every thread on return), and thread k < 3 returns raw output k.
__device__ __forceinline__ float dense_forward(const float *__restrict__ pmax, const Blob &b, int i, float *h0,
                                               float *h1, float *h2) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const float *__restrict__ p = pmax + (size_t)i * NB7 * 64 + tid;
    float mx = p[0];
    for (int k = 1; k < NB7; ++k) mx = fmaxf(mx, p[k * 64]);
    h0[tid] = mx;
  }
  __syncthreads();
  {
    float v = b.d1b[tid];
    for (int j = 0; j < 64; ++j) v = fmaf(b.d1w[tid * 64 + j], h0[j], v);
    h1[tid] = fmaxf(v, 0.f);
  }
  __syncthreads();
  if (tid < 64) {
    float v = b.d2b[tid];
    for (int j = 0; j < 128; ++j) v = fmaf(b.d2w[tid * 128 + j], h1[j], v);
    h2[tid] = fmaxf(v, 0.f);
  }
  __syncthreads();
  float r = 0.f;
  if (tid < 3) {
    r = b.d3b[tid];
    for (int j = 0; j < 64; ++j) r = fmaf(b.d3w[tid * 64 + j], h2[j], r);
  }
  return r;
}

__global__ __launch_bounds__(128) void dn_dense(const float *__restrict__ pmax, const SegMap *__restrict__ map,
                                                Blob b, float *__restrict__ poly, float *__restrict__ raw_out,
                                                int64_t g0) {
  __shared__ float h0[64], h1[128], h2[64];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (map[i].row < 0) return;
  const float r = dense_forward(pmax, b, i, h0, h1, h2);
  if (tid < 3) {
    poly[i * 3 + tid] = kPoly0[tid] + kPoly1[tid] * r + kPoly2[tid] * (r * r);
    if (raw_out) raw_out[(g0 + i) * 3 + tid] = r;
  }
}

__global__ __launch_bounds__(64) void dn_finish(const SegMap *__restrict__ map, const float *__restrict__ poly,
                                                const int *__restrict__ segflag, double *__restrict__ carry,
                                                int P, int parity, float *__restrict__ out) {
  const int i = threadIdx.x;
  if (i >= P) return;
  const SegMap m = map[i];
  if (m.row < 0 || (i > 0 && map[i - 1].row == m.row)) return;
  const double *__restrict__ cin = carry + 4 * parity;
  double *__restrict__ cout = carry + 4 * (parity ^ 1);
  double a[3] = {0.0, 0.0, 0.0};
  bool bad = false;
  if (m.s != 0) {  // (i == 0: the row the previous pass left unfinished)
    a[0] = cin[0], a[1] = cin[1], a[2] = cin[2];
    bad = cin[3] != 0.0;
  }
  int last = m.s;
  for (int j = i; j < P && map[j].row == m.row; ++j) {
    for (int k = 0; k < 3; ++k) a[k] += (double)poly[j * 3 + k];
    bad |= segflag[j] != 0;
    last = map[j].s;
  }
  if (last == m.S - 1) {
    for (int k = 0; k < 3; ++k)
      out[(int64_t)m.row * 3 + k] = bad ? __builtin_nanf("") : (float)(a[k] / (double)m.S);
  } else {
    cout[0] = a[0], cout[1] = a[1], cout[2] = a[2];
    cout[3] = bad ? 1.0 : 0.0;
  }
}

// ---- one pass
// What a recording pass leaves beside the forward's workspace (null pointers without REC).
struct Rec {
  float *reim;               // [P][2][900][161]
  uint8_t *win4, *win5, *win6;  // as a4, a5, a6
  int *pidx;                 // as pmax
};

template <int CIN, int COUT, int OUT, bool CONV1, bool REC>
inline void launch_conv(hipStream_t st, int P, int H, int W, const _Float16 *in, const float *img, const Blob &b,
                        int l, _Float16 *out, float *pmax, const SegMap *map, uint8_t *win, int *pidx) {
  const dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)((H + TH - 1) / TH), (unsigned)P);
  hipLaunchKernelGGL((dn_conv<CIN, COUT, OUT, CONV1, REC>), grid, dim3(256), 0, st, in, img, b.w1, b.b1, b.cw[l],
                     b.cb[l], out, pmax, map, H, W, win, pidx);
}

// The segments g0 ... g0 + P - 1: the map, the front end into img, and unless front_only the network up to
// the polynomial (w.poly) and the raw outputs (raw + 3 g0, unless null).
template <bool REC>
inline int forward_pass(hipStream_t st, const float *deg, int64_t batch, int64_t length, int64_t ld,
                        const int32_t *lengths, const Blob &b, const Ws &w, int P, int64_t g0, float *img,
                        bool front_only, float *raw, const Rec &rec) {
  hipLaunchKernelGGL(dn_map, dim3(1), dim3(256), 0, st, lengths, (int)length, batch, g0, P, w.map, w.segflag);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(dn_front<REC>, dim3((NF + FB - 1) / FB, (unsigned)P), dim3(256), 0, st, deg, ld, w.map, b.re_t,
                     b.im_t, img, w.segflag, rec.reim);
  FSEM_CHECK_LAUNCH();
  if (front_only) return FSEM_OK;
  launch_conv<128, 64, OUT_STORE, true, REC>(st, P, H1, W1, nullptr, img, b, 0, w.a2, nullptr, w.map, nullptr, nullptr);
  FSEM_CHECK_LAUNCH();
  launch_conv<64, 64, OUT_STORE, false, REC>(st, P, H1, W1, w.a2, nullptr, b, 1, w.a3, nullptr, w.map, nullptr, nullptr);
  FSEM_CHECK_LAUNCH();
  launch_conv<64, 32, OUT_POOL, false, REC>(st, P, H1, W1, w.a3, nullptr, b, 2, w.a4, nullptr, w.map, rec.win4, nullptr);
  FSEM_CHECK_LAUNCH();
  launch_conv<32, 32, OUT_POOL, false, REC>(st, P, H2, W2, w.a4, nullptr, b, 3, w.a5, nullptr, w.map, rec.win5, nullptr);
  FSEM_CHECK_LAUNCH();
  launch_conv<32, 32, OUT_POOL, false, REC>(st, P, H3, W3, w.a5, nullptr, b, 4, w.a6, nullptr, w.map, rec.win6, nullptr);
  FSEM_CHECK_LAUNCH();
  launch_conv<32, 64, OUT_MAX, false, REC>(st, P, H4, W4, w.a6, nullptr, b, 5, nullptr, w.pmax, w.map, nullptr, rec.pidx);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(dn_dense, dim3((unsigned)P), dim3(128), 0, st, w.pmax, w.map, b, w.poly, raw, g0);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}

// The 22 tensors (a host array of device pointers, state-dict order) into the blob's regions.
inline int pack_blob(const float *const *t, const Blob &b, hipStream_t st) {
  const unsigned T = 256;
  auto blocks = [](int n) { return dim3((unsigned)((n + 255) / 256)); };
  hipLaunchKernelGGL(pack_stft, blocks(FL * NB), dim3(T), 0, st, t[0], b.re_t);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(pack_stft, blocks(FL * NB), dim3(T), 0, st, t[1], b.im_t);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(pack_copy, blocks(128 * 9), dim3(T), 0, st, t[2], b.w1, 128 * 9);
  FSEM_CHECK_LAUNCH();
  hipLaunchKernelGGL(pack_copy, blocks(128), dim3(T), 0, st, t[3], b.b1, 128);
  FSEM_CHECK_LAUNCH();
  for (int l = 0; l < 6; ++l) {
    const int cin = kCin[l], cout = kCout[l];
    hipLaunchKernelGGL(pack_conv, blocks(9 * cin * cout), dim3(T), 0, st, t[4 + 2 * l], b.cw[l], cout, cin);
    FSEM_CHECK_LAUNCH();
    hipLaunchKernelGGL(pack_copy, blocks(cout), dim3(T), 0, st, t[5 + 2 * l], b.cb[l], cout);
    FSEM_CHECK_LAUNCH();
  }
  float *dst[6] = {b.d1w, b.d1b, b.d2w, b.d2b, b.d3w, b.d3b};
  const int cnt[6] = {128 * 64, 128, 64 * 128, 64, 3 * 64, 3};
  for (int k = 0; k < 6; ++k) {
    hipLaunchKernelGGL(pack_copy, blocks(cnt[k]), dim3(T), 0, st, t[16 + k], dst[k], cnt[k]);
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}

}  // namespace dnsmos
}  // namespace fsem
