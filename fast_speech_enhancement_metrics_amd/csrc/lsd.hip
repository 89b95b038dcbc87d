// Log-spectral distance of (clean, denoised) rows (include/fsem_lsd.h), the reference's
// fast_se_metrics.LSD (LSD.py:32-52).  Two reads of each input.
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
//   lsd_frames   grid (16 frames, row), 4 waves, a wave takes every fourth frame.  The frame's 512
//                samples of s and of a h (zero outside [0, n)) times the window, and ONE 512-point
//                complex transform of z = w s + i w a h, all in double; the two spectra come from
//                Z[k] +- conj(Z[512 - k]).  Then the 257 log terms (lane l: bins l, l + 64,
//                l + 128, l + 192, lane 0 also bin 256), their squares summed over the wave in
//                double by xor exchanges.  One float32 value per frame to the workspace.
//                Why double: the log ratio weighs every bin alike, also those 100 dB below the
//                frame's peak (the upper half of the spectrum of rows resampled from 8 kHz), where a
//                float32 transform's rounding, 1e-7 of the peak, is a tenth of the bin: the float32
//                form of this kernel (two transforms through fsem_fft.h) was 1.2e-4 off the float64
//                definition on such rows, as is the reference's own float32 STFT.  In double the
//                shared transform leaks 1e-16 of one signal into the other, far below the float32
//                samples' own rounding; a frame of one signal that is all zero gets an exactly
//                zero spectrum (the leak would otherwise stand beside the definition's 1e-8).
//                16-byte loads: a lane loads 8 consecutive samples of each signal and the wave
//                transposes them through its exchange area to the transform's lane + 64 r order;
//                4-byte loads read that order directly.  The same values either way.
//   lsd_finish   one wave per row: lane l adds the frame values l, l + 64, ... in double, in that
//                order, then the 64 sums by xor exchanges; the mean over the F frames.
//
// Every sum has one order that depends on n alone: a row's score does not depend on the batch
// size, the row's position, the row capacity, the alignment or the stream.
#include <math.h>

#include "../../include/fsem_lsd.h"
#include "fsem_build_marker.h"
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

template <bool VEC>
__global__ __launch_bounds__(T) void lsd_partial(const float *__restrict__ ref, const float *__restrict__ deg,
                                                 int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                 int64_t r0, Part *__restrict__ part, int nchunk) {
  __shared__ double red[NWAVE][2];
  const int tid = threadIdx.x;
  const int64_t row = r0 + blockIdx.y;
  const int c = blockIdx.x;
  const int n = row_length(lengths, row, length);
  const int base = c * C;  // < length + C <= 2^29 + 2^13
  if (base >= n) return;   // (lsd_scale reads ceil(n / C) records of this row)
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  double sh = 0, hh = 0;
#pragma unroll
  for (int j = 0; j < C / (4 * T); ++j) {
    const int a = base + 4 * (tid + T * j);
    if (a >= n) continue;
    float sv[4], hv[4];  // zeros from sample n on
    load4<VEC>(srow, a, n, sv);
    load4<VEC>(hrow, a, n, hv);
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

// ln(S^2 / (H + 1e-8)^2 + 1e-8) of one bin from the squared magnitudes (double, rounded to float32
// here): root, ratio and logarithm in float32, each within an ulp -- 2e-7 in a term, against terms
// of magnitude 1 to 40 (a double root and quotient: 5.30 instead of 5.01 ms per 4096 x 160000 call,
// the same scores to the last printed digit).  The ratio is kept below float32's largest number (NaN stays NaN); an S^2 or H^2 below float32's
// smallest changes nothing beside the two 1e-8.
__device__ __forceinline__ float log_term(double S2, double H2) {
  const float Hm = sqrtf((float)H2) + 1e-8f;
  const float q = (float)S2 / (Hm * Hm) + 1e-8f;
  return logf(q > 3.0e38f ? 3.0e38f : q);
}

template <bool VEC>
__global__ __launch_bounds__(T) void lsd_frames(const float *__restrict__ ref, const float *__restrict__ deg,
                                                int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                int64_t r0, const cd *__restrict__ twg,
                                                const double *__restrict__ scale, float *__restrict__ fv,
                                                int64_t fcap) {
  __shared__ __attribute__((aligned(16))) cd xbuf[NWAVE * NFFT];  // a wave's exchange area: 512 complex doubles
  __shared__ __attribute__((aligned(16))) cd tw[NFFT];  // (40 KiB with the exchange areas: 4 blocks per CU)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = r0 + blockIdx.y;
  const int n = row_length(lengths, row, length);
  const int F = 1 + n / HOP;
  const int f0 = blockIdx.x * KF;
  if (f0 >= F) return;  // (the whole block)
  for (int i = threadIdx.x; i < NFFT; i += T) tw[i] = twg[i];
  __syncthreads();
  const double a = scale[row];
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  cd *buf = xbuf + wave * NFFT;
  float *fb = reinterpret_cast<float *>(buf);
  const int plane = (64 - lane) & 63;
  for (int u = 0; u < KF / NWAVE; ++u) {
    const int f = f0 + wave + NWAVE * u;  // (wave-uniform)
    if (f >= F) break;
    const int p0 = f * HOP - HOP;  // the frame's first sample; -256 for frame 0
    float sv[8], hv[8];            // zero outside [0, n)
    if (VEC) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        // q % 4 == 0; 0 <= q < n: the float4 lies inside the row's ceil4(length) floats
        const int q = p0 + 8 * lane + 4 * half;
        float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f), h4 = s4;
        if (q >= 0 && q < n) {
          s4 = *reinterpret_cast<const float4 *>(srow + q);
          h4 = *reinterpret_cast<const float4 *>(hrow + q);
        }
        const bool i0 = q >= 0 && q < n, i1 = q >= 0 && q + 1 < n, i2 = q >= 0 && q + 2 < n,
                   i3 = q >= 0 && q + 3 < n;
        const float4 so = make_float4(i0 ? s4.x : 0.f, i1 ? s4.y : 0.f, i2 ? s4.z : 0.f, i3 ? s4.w : 0.f);
        const float4 ho = make_float4(i0 ? h4.x : 0.f, i1 ? h4.y : 0.f, i2 ? h4.z : 0.f, i3 ? h4.w : 0.f);
        *reinterpret_cast<float4 *>(fb + 8 * lane + 4 * half) = so;
        *reinterpret_cast<float4 *>(fb + NFFT + 8 * lane + 4 * half) = ho;
      }
      wave_lds_fence();
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        sv[r] = fb[lane + 64 * r];
        hv[r] = fb[NFFT + lane + 64 * r];
      }
      wave_lds_fence();  // (the transform's first scatter overwrites the area)
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int t = p0 + lane + 64 * r;
        const bool in = t >= 0 && t < n;
        sv[r] = in ? srow[t] : 0.f;
        hv[r] = in ? hrow[t] : 0.f;
      }
    }
    // a frame of one signal that is all zero has an exactly zero spectrum (NaN != 0: not zero)
    bool snz = false, hnz = false;
    cd v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      snz |= sv[r] != 0.f;
      hnz |= hv[r] != 0.f;
      const double w = 0.5 * (1.0 - tw[lane + 64 * r].r);  // periodic Hann
      v[r] = {w * (double)sv[r], w * (a * (double)hv[r])};
    }
    const bool s_zero = !__any(snz), h_zero = !__any(hnz) || a == 0.0;
    fft512_wave_d(v, buf, lane, tw);  // v[r] = Z[lane + 64 r]
    double acc = 0;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      // M = Z[512 - k] for k = lane + 64 r: lane 64 - lane's v[7 - r]; for lane 0 its own v[8 - r]
      // (k = 0: Z[0] itself).  r = 4 is bin 256, kept in lane 0 only.
      const cd m = r < 4 ? mirror_bin(v, r, lane, plane) : v[4];
      const double mr = m.r, mi = m.i;
      // S = (Z + conj M) / 2, H = (Z - conj M) / (2 i)
      const double sr = v[r].r + mr, si = v[r].i - mi, hr = v[r].i + mi, hi = v[r].r - mr;
      const double S2 = s_zero ? 0.0 : 0.25 * fma(sr, sr, si * si);
      const double H2 = h_zero ? 0.0 : 0.25 * fma(hr, hr, hi * hi);
      const double t = (double)log_term(S2, H2);
      acc = (r < 4 || lane == 0) ? fma(t, t, acc) : acc;
    }
    const double tot = wave_sum_d(acc);
    if (lane == 0) fv[row * fcap + f] = (float)sqrt(tot / (double)NBIN);
  }
}

__global__ __launch_bounds__(T) void lsd_finish(const float *__restrict__ fv, int64_t fcap,
                                                const double *__restrict__ scale,
                                                const int32_t *__restrict__ lengths, int length, int64_t B,
                                                float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * NWAVE + (threadIdx.x >> 6);
  if (b >= B) return;
  const int n = row_length(lengths, b, length);
  const int F = 1 + n / HOP;
  const float *__restrict__ p = fv + b * fcap;
  double acc = 0;
  for (int f = lane; f < F; f += 64) acc += (double)p[f];
  acc = wave_sum_d(acc);
  // a row with a non-finite sample: NaN (its scale is NaN, and so is every frame value)
  if (lane == 0) out[b] = isnan(scale[b]) ? __builtin_nanf("") : (float)(acc / (double)F);
}

// Workspace: the twiddles, the rows' scales, one record per (row, chunk), one value
// per (row, frame).
struct Ws {
  cd *tw;
  double *scale;
  Part *part;
  float *fv;
};
inline Ws layout(Arena &a, int64_t batch, int64_t length) {
  Ws w;
  w.tw = a.take<cd>((size_t)NFFT);
  w.scale = a.take<double>((size_t)batch);
  w.part = a.take<Part>((size_t)batch * (size_t)chunks(length));
  w.fv = a.take<float>((size_t)batch * (size_t)frames_of(length));
  return w;
}

}  // namespace lsd
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_lsd_frames(int64_t length) { return length < 0 ? 0 : lsd::frames_of(length); }

extern "C" int64_t fsem_lsd_chunk(void) { return lsd::C; }

extern "C" size_t fsem_lsd_workspace_bytes(int64_t batch, int64_t length) {
  if (batch < 1 || length < 1 || length > kMaxLength) return 0;
  return layout_bytes(lsd::layout, batch, length);
}

extern "C" int fsem_lsd_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                            const int32_t *lengths, float *lsd_out, void *ws, size_t ws_bytes, void *stream) {
  if (!ref || !deg || !lsd_out || batch < 1 || length < 1 || ld < length || length > kMaxLength) return FSEM_EINVAL;
  Arena a(ws);
  const lsd::Ws w = lsd::layout(a, batch, length);
  if (!a.fits(ws_bytes)) return FSEM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = (int)lsd::chunks(length);
  const int64_t fcap = lsd::frames_of(length);
  hipLaunchKernelGGL(lsd::lsd_tables, dim3(lsd::NFFT / 256), dim3(256), 0, st, w.tw);
  FSEM_CHECK_LAUNCH();
  // 16-byte loads where every row of both operands starts on a 16-byte boundary
  const bool vec = (((uintptr_t)ref | (uintptr_t)deg) & 15) == 0 && ld % 4 == 0;
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)nchunk, batch, r0);
    if (vec)
      hipLaunchKernelGGL(lsd::lsd_partial<true>, grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length, r0,
                         w.part, nchunk);
    else
      hipLaunchKernelGGL(lsd::lsd_partial<false>, grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length, r0,
                         w.part, nchunk);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(lsd::lsd_scale, dim3((unsigned)((batch + lsd::ST - 1) / lsd::ST)), dim3(lsd::ST), 0, st, w.part,
                     nchunk, lengths, (int)length, batch, w.scale);
  FSEM_CHECK_LAUNCH();
  const unsigned fblocks = (unsigned)((fcap + lsd::KF - 1) / lsd::KF);
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice(fblocks, batch, r0);
    if (vec)
      hipLaunchKernelGGL(lsd::lsd_frames<true>, grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length, r0,
                         w.tw, w.scale, w.fv, fcap);
    else
      hipLaunchKernelGGL(lsd::lsd_frames<false>, grid, dim3(lsd::T), 0, st, ref, deg, ld, lengths, (int)length, r0,
                         w.tw, w.scale, w.fv, fcap);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(lsd::lsd_finish, dim3((unsigned)((batch + lsd::NWAVE - 1) / lsd::NWAVE)), dim3(lsd::T), 0, st,
                     w.fv, fcap, w.scale, lengths, (int)length, batch, lsd_out);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}
