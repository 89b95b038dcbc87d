// Declarations shared by the STOI engine (stoi.hip) and its backward (stoi_grad.hip): the
// constants of the metric, the per-row lengths, the geometry of a call, the forward's
// workspace layout, which the backward reads as its state, and the device code by which
// stoi_tob and stoi_tob_grad build the same frame pairs.
#pragma once
#include "fsem_fft.h"
#include "fsem_resample.h"
#include "fsem_vad.h"

namespace fsem {
namespace stoi {

constexpr int NB = 15;     // one-third octave bands
constexpr int NSEG = 30;   // frames per segment
constexpr int VF = 64;     // VAD frames per workgroup
#ifndef FSEM_TOB_TF
#define FSEM_TOB_TF 32
#endif
constexpr int TF = FSEM_TOB_TF;  // STFT frames per workgroup
constexpr float kClip = 1.0f + 5.62341325190349f;  // 1 + 10^(-beta/20), beta = -15 (STOI.py:136-137)

// Per-row lengths: row b holds lens[b] input samples (clamped to [0, ncap]) when lens is
// given, else ncap.  Its 10 kHz length is that of the reference's resampler on the unpadded
// row, ceil(n * nw / orig) (torchaudio Resample, base.py:20), and its VAD frame count
// 1 + (L10 - 256) / 128 (STOI.py:92-94).
struct Rows {
  const int32_t *lens;
  int64_t ncap;
  int orig, nw;  // reduced rate pair (1, 1 for 10 kHz input)
  __device__ __forceinline__ int64_t n(int64_t b) const {
    if (!lens) return ncap;
    const int64_t v = lens[b];
    return v < 0 ? 0 : (v > ncap ? ncap : v);
  }
  __device__ __forceinline__ int64_t l10(int64_t b) const { return (n(b) * nw + orig - 1) / orig; }
  __device__ __forceinline__ int nv(int64_t b) const {
    const int64_t L10 = l10(b);
    return L10 >= 256 ? (int)((L10 - 256) / 128 + 1) : 0;
  }
};

// Peak biased float exponents of a wave's clean and denoised samples (0: all zero or
// denormal), packed (clean << 16 | denoised): per-lane maxima, then a DPP reduction (row
// rotations, row broadcasts) with a packed 16-bit max -- both signals per instruction, no LDS --
// whose last lane holds the wave's maxima (uniform result).
__device__ __forceinline__ uint32_t peak_exponents(float c0, float c1, float c2, float c3, float d0, float d1,
                                                   float d2, float d3) {
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
  // exponent field of the largest magnitude: a float max over |x| (abs source modifiers, max3)
  auto mx4 = [](float a, float b, float c, float d) {
    return __float_as_uint(__builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a), __builtin_fabsf(b)),
                                           __builtin_fmaxf(__builtin_fabsf(c), __builtin_fabsf(d))));
  };
  const uint32_t mc = mx4(c0, c1, c2, c3), md = mx4(d0, d1, d2, d3);
  uint32_t e = ((mc >> 7) & 0xffff0000u) | (md >> 23);
  auto pmax = [](uint32_t x, uint32_t y) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, x), __builtin_bit_cast(us2, y)));
  };
  e = pmax(e, dpp_mov<0x121>(e));  // row_ror:1
  e = pmax(e, dpp_mov<0x122>(e));  // row_ror:2
  e = pmax(e, dpp_mov<0x124>(e));  // row_ror:4
  e = pmax(e, dpp_mov<0x128>(e));  // row_ror:8 -> every lane holds its row's maxima
  // rows 1 and 3 take rows 0 and 2 (row_bcast:15), rows 2 and 3 take lane 31 (row_bcast:31);
  // rows outside the mask read 0, the identity of the max
  e = pmax(e, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)e, 0x142, 0xA, 0xF, false));
  e = pmax(e, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)e, 0x143, 0xC, 0xF, false));
  return __builtin_amdgcn_readlane(e, 63);
}

// ---- what stoi_tob and its backward stoi_tob_grad both do to one signal: the backward has to
// rebuild exactly the frame pairs the forward transformed.

// Sample o of a 10 kHz row through a range-checked descriptor over its [0, L10) (row_rsrc over
// L10 * 4 bytes): samples past the row end read as 0 without a branch per load (torchaudio's zero
// padding of the overlap-added signal).
__device__ __forceinline__ float sample_at(__amdgpu_buffer_rsrc_t r, int64_t o) { return buffer_f32(r, (int)(o * 4)); }

// This lane's four values of the 256-point Hann window: w[lane], w[64 + lane], w[128 + lane],
// w[192 + lane] -- the STFT window on a frame's 256 samples (v[r] takes win[r]), and the
// overlap-add weights of a block's two halves.
__device__ __forceinline__ void hann_quad(int lane, float win[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) win[r] = kHann256s[lane + 64 * r];
}

// Overlap-added block q of the kept frames kidx: block_q[t] = w[t] F_{i_q}[t] + w[128 + t]
// F_{i_{q-1}}[128 + t], F_i = the row's samples from 128 i.  ola_taps loads this lane's four
// samples (t = lane and 64 + lane of both frames), ola_block combines them into block_q[64 h +
// lane]; apart, so that a caller can have several blocks' loads in flight.
__device__ __forceinline__ void ola_taps(__amdgpu_buffer_rsrc_t r, const int *kidx, int q, int lane, float g[4]) {
  const int64_t a0 = 128LL * kidx[q], a1 = 128LL * kidx[q - 1] + 128;
  g[0] = sample_at(r, a0 + lane);
  g[1] = sample_at(r, a1 + lane);
  g[2] = sample_at(r, a0 + 64 + lane);
  g[3] = sample_at(r, a1 + 64 + lane);
}
__device__ __forceinline__ float ola_block(const float win[4], const float g[4], int h) {
  return win[h] * g[2 * h] + win[2 + h] * g[2 * h + 1];
}

// Both kernels then transform two consecutive STFT frames of ONE signal as z = frame a + i frame
// b, frame a = [block_ja, block_ja+1] * w, zero-padded to 512 points.  That load stays written out
// in both: as a function (whole, per point, block rows by pointer or by reference) it fails
// stoi_tob's static gate (SALU 391 -> 389, s_waitcnt 106 -> 113).

// The frame pair's peak exponents (peak_exponents): ea of frame a, the real parts, eb of frame b.
__device__ __forceinline__ void pair_peaks(const cf v[8], int &ea, int &eb) {
  const uint32_t pk = peak_exponents(v[0].r, v[1].r, v[2].r, v[3].r, v[0].i, v[1].i, v[2].i, v[3].i);
  ea = (int)(pk >> 16), eb = (int)(pk & 0xffffu);
}

// The shared transform's rounding is not exactly Hermitian: it leaks ~1e-7 of the louder frame's
// spectrum into the quieter one's, so a frame ~100 dB or more below its neighbour (an onset after
// silence) would lose its spectrum to the leak.  Pairs with a gap of 2^7 or more in peak sample
// are equalised first: frame b is scaled by 2^sh to frame a's peak exponent (exact in floating
// point; |sh| at most 60), and the caller scales what it derives from frame b's spectrum by 2^-sh
// after the transform (exact again).  Returns sh, 0 for a pair left as it is.
__device__ __forceinline__ int pair_level_shift(cf v[8], int ea, int eb) {
  int sh = (ea > 0 && eb > 0) ? ea - eb : 0;
  sh = (sh >= 7 || sh <= -7) ? max(-60, min(60, sh)) : 0;
  if (sh != 0) {  // uniform
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r].i = __builtin_amdgcn_ldexpf(v[r].i, sh);
  }
  return sh;
}

#ifndef FSEM_SEG_T
#define FSEM_SEG_T 256
#endif
constexpr int SEG_T = FSEM_SEG_T;  // segments per stoi_seg workgroup

// segment blocks per row of a tob buffer with tmax frames (S <= tmax - 29)
inline int seg_blocks(int64_t tmax) { return tmax > 29 ? (int)((tmax - 29 + SEG_T - 1) / SEG_T) : 1; }

struct Geometry {
  int64_t L10;
  int NV, nv_ld, tmax;
  int64_t v_ld;  // VAD quarter sums per row (float2)
  int64_t y_ld;
  bool direct;
  int mode;
};

inline int make_geometry(int64_t length, int32_t sr, Geometry *g, ResampleKernel *rk) {
  g->direct = (sr == 10000);
  if (g->direct) {
    g->L10 = length;
    rk->orig = rk->nw = 1;
    rk->taps = 1;
    rk->width = 0;
  } else {
    const int rc = make_resample_kernel(sr, 10000, rk);
    if (rc != FSEM_OK) return rc;
    g->L10 = (rk->nw * length + rk->orig - 1) / rk->orig;
  }
  g->NV = g->L10 >= 256 ? (int)((g->L10 - 256) / 128 + 1) : 0;
  g->nv_ld = (int)align_up((size_t)(g->NV > 0 ? g->NV : 1), 64);
  g->v_ld = vad_ld(g->L10);
  g->tmax = g->NV > 2 ? g->NV - 2 : 1;
  g->y_ld = (int64_t)align_up((size_t)g->L10, 64);
  g->mode = g->direct ? 1 : ((sr == 16000) ? 0 : 2);
  return FSEM_OK;
}

// The STOI workspace (Arena, fsem_common.h).
struct Ws {
  float2 *vad;
  int *idx, *kept;
  float *tob;
  double *part;
  float *y10;
};
inline Ws layout(Arena &a, int64_t B, const Geometry &g) {
  Ws w;
  w.vad = a.take<float2>((size_t)B * (size_t)g.v_ld);                 // VAD quarter sums
  w.idx = a.take<int>((size_t)B * g.nv_ld);                           // kept indices
  w.kept = a.take<int>((size_t)B);                                    // kept counts
  w.tob = a.take<float>((size_t)(2 * B) * NB * (size_t)g.tmax);       // tob
  w.part = a.take<double>(2 * (size_t)B * (size_t)seg_blocks(g.tmax));  // segment block sums
  w.y10 = a.take<float>((size_t)(2 * B) * (size_t)g.y_ld);            // 10 kHz signals
  return w;
}

// The whole forward on a workspace laid out as above (stoi.hip).
int run(const float *ref, const float *deg, int64_t B, int64_t length, int64_t ld, const int32_t *lengths,
        int32_t sr, float *stoi_out, float *estoi_out, int32_t *kept_out, float *tob_out, int64_t tob_ld, void *ws,
        size_t ws_size, hipStream_t st);

}  // namespace stoi
}  // namespace fsem
