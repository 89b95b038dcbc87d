// What the LSD forward (lsd.hip, libfsem_lsd.so) and its backward (lsd_grad.hip, libfsem.so) share:
// the geometry, the (row, chunk) records of the two scale sums with the kernels that write and add
// them, the twiddle table, the one-wave 512-point complex transform in double and the load of one
// frame.  Each library compiles its own copy (one source per library includes this header); the
// backward's scale a is therefore the forward's, bit for bit.
//
//   lsd_tables   the transform's twiddles W^k = exp(-2 pi i k / 512) in double, once per call (at the
//                head of the workspace); the window is w[t] = 0.5 (1 - Re W^t).
//   lsd_partial  grid (chunk, row).  A chunk is C = 8192 samples: thread t takes the float4s t,
//                t + 256, ... of the chunk, in that order, and adds s h and h h in double (products
//                of float32 samples, exact in double); elements at or past n are replaced by zeros.
//                The block's 256 sums are added in a fixed tree.  One 16-byte record per
//                (row, chunk); no atomics.
//   lsd_scale    one thread per row: the chunk records in ascending order, a = sum s h /
//                (sum h h + 1e-8) in double; NaN for a row with a non-finite sample.
#pragma once
#include <math.h>

#include "fsem_complex.h"

namespace fsem {
namespace lsd {

constexpr int T = 256;            // threads of a block (4 waves)
constexpr int NWAVE = T / 64;
constexpr int NFFT = 512;
constexpr int HOP = 256;
constexpr int NBIN = NFFT / 2 + 1;
constexpr int C = 8192;           // samples per chunk: 8 float4s per thread
constexpr int KF = 16;            // frames per frame block
constexpr int ST = 64;            // threads of a scale block

// One (row, chunk) record.
struct Part {
  double sh, hh;  // sum s h, sum h h over the chunk's samples
};
static_assert(sizeof(Part) == 16, "one record is 16 bytes");

struct cd {
  double r, i;
};
static_assert(sizeof(cd) == 16, "a complex double is 16 bytes");

inline int64_t chunks(int64_t length) { return (length + C - 1) / C; }
inline int64_t frames_of(int64_t n) { return 1 + n / HOP; }

__global__ void lsd_tables(cd *__restrict__ tw) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= NFFT) return;
  double sn, cs;
  sincospi((double)t / (double)(NFFT / 2), &sn, &cs);
  tw[t] = {cs, -sn};
}

// S: the rows' sample type, float, or double for the backward's rows resampled in double (plain 8-byte loads,
// VEC unused; the products are then rounded, in double).
template <class S, bool VEC>
__global__ __launch_bounds__(T) void lsd_partial(const S *__restrict__ ref, const S *__restrict__ deg,
                                                 int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                 int64_t r0, Part *__restrict__ part, int nchunk) {
  __shared__ double red[NWAVE][2];
  const int tid = threadIdx.x;
  const int64_t row = r0 + blockIdx.y;
  const int c = blockIdx.x;
  const int n = row_length(lengths, row, length);
  const int base = c * C;  // < length + C <= 2^29 + 2^13
  if (base >= n) return;   // (lsd_scale reads ceil(n / C) records of this row)
  const S *__restrict__ srow = ref + row * ld;
  const S *__restrict__ hrow = deg + row * ld;
  double sh = 0, hh = 0;
#pragma unroll
  for (int j = 0; j < C / (4 * T); ++j) {
    const int a = base + 4 * (tid + T * j);
    if (a >= n) continue;
    S sv[4], hv[4];  // zeros from sample n on
    if constexpr (sizeof(S) == sizeof(float)) {
      load4<VEC>(srow, a, n, sv);
      load4<VEC>(hrow, a, n, hv);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sv[e] = a + e < n ? srow[a + e] : (S)0;
        hv[e] = a + e < n ? hrow[a + e] : (S)0;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double sd = sv[e], hd = hv[e];
      sh = fma(sd, hd, sh);
      hh = fma(hd, hd, hh);
    }
  }
  sh = wave_sum_d(sh);
  hh = wave_sum_d(hh);
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = sh;
    red[tid >> 6][1] = hh;
  }
  __syncthreads();
  if (tid < 2) {
    const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    Part *__restrict__ p = part + (row * nchunk + c);
    if (tid == 0) p->sh = v;
    else p->hh = v;
  }
}

__global__ __launch_bounds__(ST) void lsd_scale(const Part *__restrict__ part, int nchunk,
                                                const int32_t *__restrict__ lengths, int length, int64_t B,
                                                double *__restrict__ scale) {
  const int64_t b = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (b >= B) return;
  const int n = row_length(lengths, b, length);
  const int nc = (n + C - 1) / C;
  const Part *__restrict__ p = part + b * nchunk;
  double sh = 0, hh = 0;
  for (int c = 0; c < nc; ++c) {
    sh += p[c].sh;
    hh += p[c].hh;
  }
  // a non-finite sample in either row makes one of the sums non-finite (inf * 0 is NaN)
  scale[b] = (isfinite(sh) && isfinite(hh)) ? sh / (hh + 1e-8) : (double)__builtin_nanf("");
}

// The twiddles, then both scale sums of every row: lsd_tables, lsd_partial over the grid.y slices,
// lsd_scale.  `vec`: 16-byte loads (every row of both operands starts on a 16-byte boundary).
inline int launch_scales(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                         const int32_t *lengths, bool vec, cd *tw, Part *part, double *scale, hipStream_t st) {
  const int nchunk = (int)chunks(length);
  hipLaunchKernelGGL(lsd_tables, dim3(NFFT / 256), dim3(256), 0, st, tw);
  FSEM_CHECK_LAUNCH();
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)nchunk, batch, r0);
    if (vec)
      hipLaunchKernelGGL((lsd_partial<float, true>), grid, dim3(T), 0, st, ref, deg, ld, lengths, (int)length, r0, part, nchunk);
    else
      hipLaunchKernelGGL((lsd_partial<float, false>), grid, dim3(T), 0, st, ref, deg, ld, lengths, (int)length, r0, part, nchunk);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(lsd_scale, dim3((unsigned)((batch + ST - 1) / ST)), dim3(ST), 0, st, part, nchunk, lengths,
                     (int)length, batch, scale);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}

// ---- one-wave 512-point complex transform in double: fsem_fft.h's radix-8 Stockham scheme (the
// same stages, exchange pattern and swizzle) on complex doubles, twiddles read from an LDS table;
// the butterflies, the complex arithmetic and the swizzle are fsem_complex.h's.
// v[r] = z[lane + 64 r] -> v[r] = Z[lane + 64 r].  `buf`: this wave's 512 complex doubles of LDS;
// `tw`: W^k, k = 0 ... 511, in LDS.
__device__ __forceinline__ void fft512_wave_d(cd v[8], cd *buf, int lane, const cd *tw) {
  dft8(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[fpad(8 * lane + r)] = v[r];
  wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[fpad(lane + 64 * r)];
#pragma unroll
  for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[(8 * r * (lane & 7)) & 511]);
  dft8(v);
  wave_lds_fence();
  const int o1 = (lane >> 3) * 64 + (lane & 7);
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[fpad(o1 + 8 * r)] = v[r];
  wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[fpad(lane + 64 * r)];
#pragma unroll
  for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], tw[(r * lane) & 511]);
  dft8(v);
  wave_lds_fence();
}

// The 512 samples of both rows from sample p0 on (p0 % 256 == 0; -256 for frame 0), zero outside
// [0, n), in the transform's order: sv[r], hv[r] = sample p0 + lane + 64 r (float sv[8], hv[8]).
// 16-byte loads (VEC): a lane loads 8 consecutive samples of each signal and the wave transposes
// them through its exchange area `fb` (1024 floats) to that order; 4-byte loads read the order
// directly.  The same values either way.  A macro, not a function: expanded in the kernel the
// forward compiles to the instructions it had when the text stood there (through a function the
// register allocation came out differently).
#define FSEM_LSD_LOAD_FRAME(VEC, srow, hrow, p0, n, lane, fb, sv, hv)                                        \
  if (VEC) {                                                                                                 \
    _Pragma("unroll") for (int half = 0; half < 2; ++half) {                                                 \
      /* q % 4 == 0; 0 <= q < n: the float4 lies inside the row's ceil4(length) floats */                    \
      const int q = p0 + 8 * lane + 4 * half;                                                                \
      float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f), h4 = s4;                                                  \
      if (q >= 0 && q < n) {                                                                                 \
        s4 = *reinterpret_cast<const float4 *>(srow + q);                                                    \
        h4 = *reinterpret_cast<const float4 *>(hrow + q);                                                    \
      }                                                                                                      \
      const bool i0 = q >= 0 && q < n, i1 = q >= 0 && q + 1 < n, i2 = q >= 0 && q + 2 < n,                   \
                 i3 = q >= 0 && q + 3 < n;                                                                   \
      const float4 so = make_float4(i0 ? s4.x : 0.f, i1 ? s4.y : 0.f, i2 ? s4.z : 0.f, i3 ? s4.w : 0.f);     \
      const float4 ho = make_float4(i0 ? h4.x : 0.f, i1 ? h4.y : 0.f, i2 ? h4.z : 0.f, i3 ? h4.w : 0.f);     \
      *reinterpret_cast<float4 *>(fb + 8 * lane + 4 * half) = so;                                            \
      *reinterpret_cast<float4 *>(fb + NFFT + 8 * lane + 4 * half) = ho;                                     \
    }                                                                                                        \
    wave_lds_fence();                                                                                        \
    _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                                          \
      sv[r] = fb[lane + 64 * r];                                                                             \
      hv[r] = fb[NFFT + lane + 64 * r];                                                                      \
    }                                                                                                        \
    wave_lds_fence(); /* (the transform's first scatter overwrites the area) */                              \
  } else {                                                                                                   \
    _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                                          \
      const int t = p0 + lane + 64 * r;                                                                      \
      const bool in = t >= 0 && t < n;                                                                       \
      sv[r] = in ? srow[t] : 0.f;                                                                            \
      hv[r] = in ? hrow[t] : 0.f;                                                                            \
    }                                                                                                        \
  }

}  // namespace lsd
}  // namespace fsem
