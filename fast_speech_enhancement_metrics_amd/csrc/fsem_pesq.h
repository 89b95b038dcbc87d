// Shared geometry of the PESQ front end (pesq.hip) and back end (pesq_back.hip): frames,
// segments and the band-major Bark layout of a row (PESQ.py:123-140, bark.py:189-204); and the
// device functions that the forward, the backward (pesq_grad.hip) and the time alignment's pooling
// (align.hip) share.
#pragma once
#include "fsem_fft.h"  // (fsem_tables.inc: FSEM_PESQ_CH)

namespace fsem {
namespace pesq {

constexpr int NF = 48;            // frames per segment
constexpr int OWN = NF * 256;     // samples of band-pass power owned per segment
constexpr int NBARK = 49;
constexpr int PESQ_CH = FSEM_PESQ_CH;
constexpr int PESQ_TILE = 256 * PESQ_CH;  // 13312
constexpr int PESQ_WARM = 768;

// Bark bands are stored band-major per signal: bark[(s * NBARK + k) * bark_ld(F) + f], rows
// padded to a multiple of 32 frames: every row starts on a 128-byte line, so the back end's
// loads of one band over 64 consecutive frames (lane = frame) touch exactly two lines (a
// 4-frame padding left them straddling three: 1.25x the HBM reads), and the MFMA tiles' float4
// stores stay aligned.
__host__ __device__ inline int64_t bark_ld(int F) { return (F + 31) & ~31; }

__host__ __device__ inline int frames_of(int64_t L) {
  const int64_t Lp = L + (L % 256);  // PESQ.py:128-130: pad by L % 256 (sic)
  if (Lp < 512) return 0;
  return (int)(1 + (Lp - 512) / 256);
}

struct Geometry {
  int F, nfseg, npseg, nseg;
};

// Segment g owns band-pass power samples [g*OWN, (g+1)*OWN); the LAST segment owns
// [g*OWN, L), which its tile must cover: L - (nseg-1)*OWN <= PESQ_TILE - PESQ_WARM.  Every field is
// non-decreasing in L, so the geometry of the longest row bounds every shorter row's.
__host__ __device__ inline Geometry geometry(int64_t L) {
  Geometry g;
  g.F = frames_of(L);
  g.nfseg = (g.F + NF - 1) / NF;
  const int64_t span = PESQ_TILE - PESQ_WARM;
  g.npseg = L <= span ? 1 : (int)((L - span + OWN - 1) / OWN) + 1;
  g.nseg = g.nfseg > g.npseg ? g.nfseg : g.npseg;
  return g;
}

// Device functions the forward (pesq.hip, pesq_back.hip) and the backward (pesq_grad.hip) share.
// PESQ.py:90,108-109: first 15 samples x (t+1)/16, last 15 samples x (L-t)/16, else 1:
// w(t) = sat((t+1)/16) * sat((L-t)/16), exact in float32 for t, L < 2^24.
__device__ __forceinline__ float taper_w(float tf, float Lf) {
  return __saturatef((tf + 1.f) * 0.0625f) * __saturatef((Lf - tf) * 0.0625f);
}

// x^e for x > 0 (every call site: x >= 0.5 or a ratio of positive terms) via the hardware
// v_log_f32 / v_exp_f32 (~1 ulp each); the reference evaluates these in float64, the
// difference is ~1e-7 relative, far inside the +-0.01 MOS tolerance.
__device__ __forceinline__ float pow_pos(float x, float e) {
  return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x));
}

__device__ __forceinline__ float loud(float p, int b) {
  // loudness.py:64-65: (2T)^e ((0.5 + 0.5 P/T)^e - 1), 0 where P <= T; times Sl (folded).
  // 0.5 P/T as P * (0.5/T) (one rounding instead of a correctly rounded division: <=1 ulp)
  // branch-free (p >= 0: the pow argument is >= 0.5 either way)
  const float v = kLoud2TE[b] * (pow_pos(fmaf(p, kHalfInvThresh[b], 0.5f), kLoudExp[b]) - 1.f);
  return (p > kThresh[b]) ? v : 0.f;
}

// ---- the back end's arithmetic, shared by pesq_back (pesq_back.hip), its reverse pesq_back_grad
// (pesq_grad.hip) and the time alignment's pooling (ta_bad_pool, align.hip).

// PESQ.py:97-100 -- a signal's power = band-pass sum / (L + 5120) / 1.04684, and its samples (here:
// its Bark bands) are scaled by 1e7 / power.
__device__ __forceinline__ float level_scale(float pw, int64_t L) {
  const float p = pw / (float)(L + 5120) / 1.04684f;
  return 1e7f / p;
}

// One band of one frame (PESQ.py:186-224) from the level-equalised clean power ec and denoised
// power en.  band_terms: the loudnesses lc, ln; their difference d0 and its magnitude past the
// dead zone of a quarter of the smaller loudness, mag (the disturbance is mag's positive part with
// d0's sign); wd, the disturbance times the band's width.  asymmetry_raw: ((en + 50) / (ec +
// 50))^1.2 (~1 ulp rcp); asymmetry_factor: that, 0 below 3 and at most 12.  A frame's symmetric
// sum takes wd^2, its asymmetric sum |wd am|.  (wd and am as two calls, the symmetric sum's
// update between them: as one function returning both, pesq_back fails the static gate.)
struct BandTerms {
  float lc, ln, d0, mag, wd;
};
__device__ __forceinline__ BandTerms band_terms(float ec, float en, int k) {
  BandTerms o;
  o.lc = loud(ec, k), o.ln = loud(en, k);
  o.d0 = o.ln - o.lc;
  const float dz = 0.25f * fminf(o.lc, o.ln);
  o.mag = fabsf(o.d0) - dz;
  o.wd = kWidthBark[k] * copysignf(fmaxf(o.mag, 0.f), o.d0);
  return o;
}
__device__ __forceinline__ float asymmetry_raw(float ec, float en) {
  return pow_pos((en + 50.f) * __builtin_amdgcn_rcpf(ec + 50.f), 1.2f);
}
__device__ __forceinline__ float asymmetry_factor(float am0) { return (am0 < 3.f) ? 0.f : fminf(am0, 12.f); }

// L6 norms of window w's 20 frames (hop 10) of the symmetric and the asymmetric frame
// disturbances, in double (PESQ.py:168-170); frame(f, x, y) yields frame f's two.  The callers add
// the squares up over the windows (L2, :171-172).
template <class Frame>
__device__ __forceinline__ void window_l6(int w, Frame frame, double &ps, double &pa) {
  double s6 = 0.0, a6 = 0.0;
  for (int i = 0; i < 20; ++i) {
    double x, y;
    frame(10 * w + i, x, y);
    const double x2 = x * x, y2 = y * y;
    s6 += x2 * x2 * x2;
    a6 += y2 * y2 * y2;
  }
  ps = pow(s6 / 20.0, 1.0 / 6.0);
  pa = pow(a6 / 20.0, 1.0 / 6.0);
}

// The distances' mapping to MOS-LQO: raw = 4.5 - 0.1 ds - 0.0309 da (PESQ.py:240), then
// 0.999 + 4 / (1 + exp(-1.3669 raw + 3.8224)) (PESQ.py:243).
constexpr double kMosBase = 4.5, kMosSym = 0.1, kMosAsym = 0.0309;
constexpr double kMosLo = 0.999, kMosSpan = 4.0, kMosSlope = 1.3669, kMosShift = 3.8224;
__device__ __forceinline__ double mos_raw(double ds, double da) { return kMosBase - kMosSym * ds - kMosAsym * da; }
__device__ __forceinline__ double mos_exp(double raw) { return exp(-kMosSlope * raw + kMosShift); }
__device__ __forceinline__ double mos_of(double ds, double da) {
  return kMosLo + kMosSpan / (1.0 + mos_exp(mos_raw(ds, da)));
}

// Workspace layouts (Arena, fsem_common.h).
// Front end: per-segment power partials [2B, nseg, 4], then the range bookkeeping: the segments'
// range shifts [2B, nseg] (pesq_front's pexp, read by the back end), worklist count, item queue,
// flags [2B], worklist [2B].
struct FrontWs {
  float *ppart;
  int *rng;
};
inline FrontWs front_layout(Arena &a, int64_t batch, int64_t length) {
  const size_t segs = (size_t)(2 * batch) * (size_t)geometry(length).nseg;
  FrontWs w;
  w.ppart = a.take<float>(segs * 4);
  w.rng = a.take<int>(segs + 2 + 4 * (size_t)batch);
  return w;
}
// Back end: its scratch rows.
inline float *back_layout(Arena &a, int64_t batch, int64_t length) {
  return a.take<float>((size_t)batch * (size_t)geometry(length).F * 4);
}
// Whole metric: [front | bark | power | back scratch].
struct WbWs {
  FrontWs front;
  float *bark, *power, *back;
};
inline WbWs wb_layout(Arena &a, int64_t batch, int64_t length) {
  WbWs w;
  w.front = front_layout(a, batch, length);
  w.bark = a.take<float>((size_t)(2 * batch) * NBARK * (size_t)bark_ld(geometry(length).F));
  w.power = a.take<float>((size_t)(2 * batch));
  w.back = back_layout(a, batch, length);
  return w;
}

}  // namespace pesq
}  // namespace fsem
