// Resampling kernel descriptor shared by resample.hip and the fused STOI kernels.
#pragma once
#include <math.h>

#include "fsem_common.h"

#define FSEM_RS_MAX_COEF 512

namespace fsem {

// Largest filter (taps = 2 * width + orig) any rate pair may have: FSEM_ERATE beyond it.
#define RS_BIG_TAPS 8192

struct ResampleKernel {
  int orig, nw, taps, width;  // reduced rates, taps = 2*width + orig
  int big;                    // nw * taps > FSEM_RS_MAX_COEF: k unused, built on the device
  float k[FSEM_RS_MAX_COEF];  // [nw][taps]
};

// Coefficient (phase j, tap t) of torchaudio 2.8's _get_sinc_resample_kernel (sinc_interp_hann,
// lowpass_filter_width 6, rolloff 0.99; float64 build, float32 phase offsets, cast to float32)
// for the reduced rate pair orig -> nw.  Host and device evaluate the same float64 expression.
__host__ __device__ inline float sinc_coef(int j, int t, int orig, int nw, int width) {
  const double pi = 3.14159265358979323846;
  const double base = (double)(orig < nw ? orig : nw) * 0.99;
  const float ph32 = (float)(-j) / (float)nw;  // int arange / int -> float32 in torchaudio
  double tt = ((double)ph32 + (double)(t - width) / orig) * base;
  if (tt < -6.0) tt = -6.0;
  if (tt > 6.0) tt = 6.0;
  const double c = cos(tt * pi / 6.0 / 2.0);
  const double win = c * c;
  tt *= pi;
  const double s = (tt == 0.0) ? 1.0 : sin(tt) / tt;
  return (float)(s * (win * (base / orig)));
}

int make_resample_kernel(int32_t orig_freq, int32_t new_freq, ResampleKernel *rk);

// Polyphase resampler for any rate pair (resample.hip): rows r of `in` (row length n = lens[r]
// clamped to [0, n_in], or n_in) -> out + r * ld_out, ceil(n * nw / orig) samples; columns
// [ceil(n * nw / orig), zc) are zeroed (zc <= ceil(n_in * nw / orig); 0: none).
int launch_resample_tiled(const float *in, int64_t rows, int64_t n_in, int64_t ld_in, const int32_t *lens,
                          float *out, int64_t ld_out, int64_t zc, const ResampleKernel &rk, hipStream_t st);

// One output sample o of a row x[0..n): torchaudio's pad + strided conv1d.
__device__ __forceinline__ float resample_at(const float *__restrict__ x, int64_t n, int64_t o,
                                             const ResampleKernel &rk) {
  const int64_t m = o / rk.nw;
  const int j = (int)(o - m * rk.nw);
  const int64_t base = m * rk.orig - rk.width;
  const float *kj = rk.k + j * rk.taps;
  float acc = 0.f;
  if (base >= 0 && base + rk.taps <= n) {
    for (int t = 0; t < rk.taps; ++t) acc = fmaf(kj[t], x[base + t], acc);
  } else {
    for (int t = 0; t < rk.taps; ++t) {
      const int64_t i = base + t;
      const float v = (i >= 0 && i < n) ? x[i] : 0.f;
      acc = fmaf(kj[t], v, acc);
    }
  }
  return acc;
}

// The resampler's transpose (fsem_resample_rows_grad_f32; on a double gradient: fsem_lsd_grad_rate_f32): grad_in[r, i] = sum_o K[o mod nw][i - first(o)] g_out[r, o] over the row's output
// samples o = m nw + j < ceil(n nw / orig) whose taps reach input sample i (first(o) = m orig - width),
// m then j ascending; 0 from the row's length n on.  One thread per input sample, the forward's
// float32 taps, the sum in double and rounded once.  Any rate pair (a large table's coefficients are
// evaluated where they are used, by the forward's formula).
constexpr int RS_GRAD_T = 256;
template <class G>
__global__ void __launch_bounds__(RS_GRAD_T) resample_rows_grad(const G *__restrict__ g_out, int64_t n_in, int64_t ld_out,
                                                          const int32_t *__restrict__ lens, float *__restrict__ grad_in,
                                                          int64_t ld_in, int64_t r0, ResampleKernel rk) {
  __shared__ float ks[FSEM_RS_MAX_COEF];
  const int tid = threadIdx.x;
  const int64_t r = r0 + blockIdx.y;
  const int orig = rk.orig, nw = rk.nw, taps = rk.taps, width = rk.width;
  if (!rk.big)
    for (int i = tid; i < nw * taps; i += RS_GRAD_T) ks[i] = rk.k[i];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * RS_GRAD_T + tid;
  if (i >= n_in) return;
  int64_t n = n_in;
  if (lens) {
    const int64_t v = lens[r];
    n = v < 0 ? 0 : (v > n_in ? n_in : v);
  }
  double acc = 0.0;
  if (i < n) {
    const int64_t n_out = (n * nw + orig - 1) / orig;
    const G *__restrict__ g = g_out + r * ld_out;
    const int64_t num = i + width - taps + 1;
    const int64_t m_lo = num <= 0 ? 0 : (num + orig - 1) / orig;
    const int64_t m_hi = (i + width) / orig;
    for (int64_t m = m_lo; m <= m_hi; ++m) {
      const int t = (int)(i - (m * orig - width));  // 0 <= t < taps
      for (int j = 0; j < nw; ++j) {
        const int64_t o = m * nw + j;
        if (o < n_out)
          acc = fma((double)(rk.big ? sinc_coef(j, t, orig, nw, width) : ks[j * taps + t]), (double)g[o], acc);
      }
    }
  }
  grad_in[r * ld_in + i] = (float)acc;
}

}  // namespace fsem
