// Log-spectral distance of (clean, denoised) rows (include/fsem_lsd.h), the reference's
// fast_se_metrics.LSD (LSD.py:32-52).  Two reads of each input.
//
//   lsd_tables, lsd_partial, lsd_scale   the twiddles and the scale a = sum s h / (sum h h + 1e-8) of every
//                row: fsem_lsd_kernels.h, shared with the backward (lsd_grad.hip).
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
#include "fsem_lsd_kernels.h"

namespace fsem {
namespace lsd {

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
    FSEM_LSD_LOAD_FRAME(VEC, srow, hrow, p0, n, lane, fb, sv, hv)
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
  const int64_t fcap = lsd::frames_of(length);
  // 16-byte loads where every row of both operands starts on a 16-byte boundary
  const bool vec = (((uintptr_t)ref | (uintptr_t)deg) & 15) == 0 && ld % 4 == 0;
  const int rc = lsd::launch_scales(ref, deg, batch, length, ld, lengths, vec, w.tw, w.part, w.scale, st);
  if (rc != FSEM_OK) return rc;
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
