// PESQ-wb with gradients for gfx950 (MI355X): the backward of fsem_pesq_wb_f32 with respect to the
// denoised rows (include/fsem.h, "PESQ with gradients").
//
// fsem_pesq_state_f32 runs the forward's kernels (pesq.hip, pesq_back.hip) on a caller-owned state
// that keeps both signals' unscaled Bark bands, the power partials and the range bookkeeping.
// fsem_pesq_grad_f32 then runs five kernels on the state's tail:
//
// pesq_back_grad   one 256-thread workgroup per row, a thread per frame.  Recomputes the back end's
//   forward from the state with the forward's device functions (fsem_pesq.h), then reverses the
//   pooling (double, as the forward's pass 3), the frame pass (the 0.8 / 0.2 smoothing couples
//   neighbouring frames: per-frame terms go through a scratch row between two sweeps) and the
//   band ratio (couples all frames of a row: a block reduction between two sweeps).  Writes
//   q[k, f] = dL/dN[f, k] * sigma_d * corr_k and the row's coefficient 2 g^2 (sum G N) / P.
// pesq_pre_fwd     (row, tile): the tapered, pre-emphasised, unscaled row y, by the tile filter below.
// pesq_front_grad  (row, 15 hops): the spectra of the 16 frames that touch the hops, two frames
//   per complex 512-point transform as the forward packs them; W = conj(Ga + i Gb) with
//   G = q Y on bins 1..255 and its mirror; one more forward transform of W gives conj(ga + i gb),
//   the unnormalised inverse transforms; Hann window; the two frames over a sample are summed in a
//   fixed order by the thread that owns the sample.
// pesq_power_grad  (row, tile): band-pass forward, then reversed, on the input row in one LDS tile:
//   grad = -coef BP^T(BP x).  Writes every element of grad[b, 0..length).
// pesq_pre_grad    (row, tile): the reversed pre-emphasis of the front gradient, times the taper,
//   added to grad by the thread that owns the sample.
//
// The tile filter (iir_tile) is the forward's chunk scan without its tables: lane j owns a
// 52-sample chunk; its zero-state end state e_j comes from one run over the chunk, the chunk
// transition M (the end state of a zero-input run from each unit state) and its powers are formed
// in the kernel, and a 4-level Hillis-Steele scan gives the lane's true start state from the 16
// chunks before it: both filters forget their state within that (pesq.hip: <1e-11 within 16
// chunks), so a tile's first 15 chunks are warm-up (look-ahead for the reversed filters, which run
// the same code on the tile read backwards).  No tables beyond the filters' coefficients; no
// atomics; every sum in a fixed order.
#include <type_traits>

#include "fsem_fft.h"
#include "fsem_internal.h"
#include "fsem_pesq.h"

namespace fsem {
namespace pesq {

constexpr int GT = 256;                 // threads per workgroup, every kernel here
constexpr int GCH = FSEM_PESQ_CH;       // 52 samples per lane
constexpr int GTILE = GT * GCH;         // 13312
constexpr int GWC = 15;                 // warm-up chunks
constexpr int GWARM = GWC * GCH;        // 780 samples
constexpr int OWN_PRE = GTILE - GWARM;  // samples a one-way filter tile owns (12532)
constexpr int OWN_BP = GTILE - 2 * GWARM;  // samples a forward + reversed tile owns (11752)
constexpr int NHOP = 15;                // hops of 256 samples per pesq_front_grad workgroup
constexpr int SCR = 6;                  // float scratch rows of Fcap per utterance (pesq_back_grad)

// ------------------------------------------------------------------------------ back end, reversed
// One frame's forward quantities (the arithmetic of pesq_back's pass 2).
struct FrameOut {
  float s2, as, sy, ay, w, S, A;
};

__device__ __forceinline__ float loud_prime(float p, int k) {
  // d loud / d p = (2T)^e Sl e (0.5 + 0.5 p / T)^(e - 1) 0.5 / T, 0 where p <= T (a constant decision)
  const float v = kLoud2TE[k] * kLoudExp[k] * kHalfInvThresh[k] *
                  pow_pos(fmaf(p, kHalfInvThresh[k], 0.5f), kLoudExp[k] - 1.f);
  return (p > kThresh[k]) ? v : 0.f;
}

// One frame's bands, read where they lie (band-major rows, lane = frame: coalesced, and the six sweeps of
// a row hit the cache): the band loops stay rolled, so nothing of a frame is held in register arrays.
struct Bands {
  const float *c, *n;  // this frame's band 0 of the clean / denoised signal
  int64_t fld;
  float sc, sn;        // level scales
  __device__ __forceinline__ float clean(int k) const { return c[k * fld] * sc; }
  __device__ __forceinline__ float den(int k) const { return n[k * fld] * sn; }
};

// MODE 0: forward only.  MODE 1: backward, the frame-ratio term alone (g_r, and the weight's share
// of g_ac).  MODE 2: backward, final: G[k] (without the band-ratio term) goes to qf[k fld] and the
// band-ratio sums c g_ec, summed over the wave's frames, are added to grho[k] (this wave's LDS row).
template <int MODE>
__device__ __forceinline__ FrameOut frame_pass(const Bands &x, bool valid, const float *rho, float r, float ac,
                                               float gS, float gA, float g_ac, float g_an, float &g_r, float &g_acw,
                                               float *__restrict__ qf, float *grho, int lane) {
  const float sqrt_tw = sqrtf((float)kTotalWidth);
  FrameOut o;
  float s2 = 0.f, as = 0.f;
#pragma unroll 1
  for (int k = 1; k < NBARK; ++k) {
    const float ec = rho[k] * x.clean(k), en = r * x.den(k);
    const float wd = band_terms(ec, en, k).wd;
    s2 = fmaf(wd, wd, s2);
    as += fabsf(wd * asymmetry_factor(asymmetry_raw(ec, en)));
  }
  o.s2 = s2;
  o.as = as;
  const float root = sqrt_tw * sqrtf(s2);
  o.sy = fmaxf(root, 1e-20f);
  o.ay = fmaxf(as, 1e-20f);
  o.w = pow_pos((ac + 1e5f) / 1e7f, 0.04f);
  const float qs = o.sy / o.w, qa = o.ay / o.w;
  o.S = fminf(qs, 45.f);
  o.A = fminf(qa, 45.f);
  if (MODE == 0) return o;
  // every clamp passes the gradient inside its range and 0 outside; the root of a zero sum takes 0
  const float g_sy = (qs <= 45.f) ? gS / o.w : 0.f;
  const float g_ay = (qa <= 45.f) ? gA / o.w : 0.f;
  const float g_w = -((qs <= 45.f) ? gS * qs / o.w : 0.f) - ((qa <= 45.f) ? gA * qa / o.w : 0.f);
  const float g_s2 = (s2 > 0.f && root >= 1e-20f) ? g_sy * sqrt_tw * 0.5f / sqrtf(s2) : 0.f;
  const float g_as = (as >= 1e-20f) ? g_ay : 0.f;
  if (MODE == 1) g_acw = g_w * 0.04f * o.w / (ac + 1e5f);
  float gr = 0.f;
  if (MODE == 2 && valid) qf[0] = 0.f;
#pragma unroll 1
  for (int k = 1; k < NBARK; ++k) {
    const float c = x.clean(k), ns = x.den(k);
    const float ec = rho[k] * c, en = r * ns;
    const BandTerms bt = band_terms(ec, en, k);
    const float lc = bt.lc, ln = bt.ln, d0 = bt.d0, wd = bt.wd;
    const bool act = bt.mag > 0.f;
    const float wb = kWidthBark[k];
    const float am0 = asymmetry_raw(ec, en);
    const float am = asymmetry_factor(am0);
    const float xx = wd * am;
    const float sg = (xx > 0.f) ? 1.f : ((xx < 0.f) ? -1.f : 0.f);
    const float g_d = 2.f * g_s2 * wb * wd + g_as * sg * wb * am;
    const float g_am = (am0 >= 3.f && am0 <= 12.f) ? g_as * sg * wd : 0.f;
    const float t = g_am * 1.2f * am0;
    float g_en = t / (en + 50.f), g_ec = -t / (ec + 50.f);
    const float g_d0 = act ? g_d : 0.f;
    const float g_m = act ? ((d0 > 0.f) ? -g_d : g_d) : 0.f;  // -g_d sign(d0)
    float g_ln = g_d0, g_lc = -g_d0;
    if (lc < ln) g_lc = fmaf(0.25f, g_m, g_lc);
    else g_ln = fmaf(0.25f, g_m, g_ln);
    g_en = fmaf(g_ln, loud_prime(en, k), g_en);
    g_ec = fmaf(g_lc, loud_prime(ec, k), g_ec);
    if (MODE == 1) gr = fmaf(ns, g_en, gr);
    if (MODE == 2) {
      if (valid) qf[k * x.fld] = r * g_en + ((ns > kThresh[k]) ? g_an : 0.f);
      g_ec += (ec > kThresh[k]) ? g_ac : 0.f;
      const float tk = wave_sum(valid ? c * g_ec : 0.f);
      if (lane == 0) grho[k] += tk;
    }
  }
  if (MODE == 1) g_r = gr;
  return o;
}

__global__ void __launch_bounds__(GT)
    pesq_back_grad(const float *__restrict__ bark, const float *__restrict__ ppart, const int *__restrict__ rng, int nseg,
                   int64_t B, int64_t Lcap, const int32_t *__restrict__ lens, int Fcap,
                   const float *__restrict__ g_mos, const float *__restrict__ g_sym, const float *__restrict__ g_asym,
                   float *__restrict__ scratch, double *__restrict__ dscratch, float *__restrict__ q,
                   float *__restrict__ coef, int *__restrict__ okv) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;
  const int64_t L = row_length(lens, b, Lcap);
  const int F = frames_of(L);
  __shared__ float pw_s[2];
  __shared__ int bad_s[2];
  __shared__ float tot[2][4][NBARK];
  __shared__ float rho_s[NBARK], gmn_s[NBARK];
  __shared__ double dred[2][4];
  __shared__ double gd_s[2];
  if (F < 20) {  // the score is NaN: a zero gradient row
    if (tid == 0) {
      okv[b] = 0;
      coef[b] = 0.f;
    }
    return;
  }
  // signal powers in the forward's order (pesq_back); a row with a range-shifted segment or a
  // flagged signal gets a zero gradient row
  if (tid < 2) {
    const float *__restrict__ pp = ppart + (b + tid * B) * (int64_t)nseg * 4;
    const int *__restrict__ ex = rng + (b + tid * B) * (int64_t)nseg;
    const int *__restrict__ rflag = rng + 2 * B * nseg + 2;
    int any = rflag[b + tid * B];
    for (int g = 0; g < nseg; ++g) any |= ex[g];
    float acc = 0.f;
    for (int g = 0; g < 4 * nseg; ++g) acc += pp[g];
    pw_s[tid] = acc;
    bad_s[tid] = any != 0;
  }
  for (int e = tid; e < 2 * 4 * NBARK; e += GT) (&tot[0][0][0])[e] = 0.f;
  __syncthreads();
  const float pwc = pw_s[0], pwn = pw_s[1];
  const float sc = level_scale(pwc, L), sn = level_scale(pwn, L);
  if (bad_s[0] || bad_s[1] || !__builtin_isfinite(sc) || !__builtin_isfinite(sn)) {  // (uniform)
    if (tid == 0) {
      okv[b] = 0;
      coef[b] = 0.f;
    }
    return;
  }
  const int64_t fld = bark_ld(Fcap);
  const float *__restrict__ bc = bark + b * NBARK * fld;
  const float *__restrict__ bn = bark + (b + B) * NBARK * fld;
  float *__restrict__ qb = q + b * NBARK * fld;
  float *__restrict__ frv = scratch + b * (int64_t)Fcap * SCR;  // frame ratios
  float *__restrict__ Sv = frv + Fcap, *__restrict__ Av = Sv + Fcap;
  float *__restrict__ gtv = Av + Fcap, *__restrict__ gav = gtv + Fcap, *__restrict__ keepv = gav + Fcap;
  double *__restrict__ winv = dscratch + b * (int64_t)Fcap;  // per window: ps^-4, then pa^-4 from nw on
  // every sweep: frame f = f0 + tid, a uniform trip count (the wave sums take every lane); lanes
  // past the last frame read it again and contribute nothing
  auto bands = [&](int f) { return Bands{bc + f, bn + f, fld, sc, sn}; };

  // ---- pass 1: silent frames and the band totals of the audible power of the others
  for (int f0 = 0; f0 < F; f0 += GT) {
    const int f = f0 + tid;
    const bool valid = f < F;
    const Bands x = bands(valid ? f : F - 1);
    float a = 0.f;
#pragma unroll 1
    for (int k = 0; k < NBARK; ++k) {
      const float cl = x.clean(k);
      a += (cl > kThresh[k] * 100.f) ? cl : 0.f;
    }
    const bool keep = valid && !(a < 1e7f);
    if (valid) keepv[f] = keep ? 1.f : 0.f;
#pragma unroll 1
    for (int k = 0; k < NBARK; ++k) {
      const float cl = x.clean(k), n = x.den(k);
      const float t0 = wave_sum((keep && cl > kThresh[k] * 100.f) ? cl : 0.f);
      const float t1 = wave_sum((keep && n > kThresh[k] * 100.f) ? n : 0.f);
      if (lane == 0) {
        tot[0][wv][k] += t0;
        tot[1][wv][k] += t1;
      }
    }
  }
  __syncthreads();
  if (tid < NBARK) {
    const float mc = ((tot[0][0][tid] + tot[0][1][tid]) + tot[0][2][tid]) + tot[0][3][tid];
    const float mn = ((tot[1][0][tid] + tot[1][1][tid]) + tot[1][2][tid]) + tot[1][3][tid];
    const float cm = mc / (float)F, nm = mn / (float)F;
    const float raw = (nm + 1000.f) / (cm + 1000.f);
    rho_s[tid] = fminf(fmaxf(raw, 0.01f), 100.f);
    // d rho / d (one band power of a kept, audible frame), 0 outside the clamp
    gmn_s[tid] = (raw >= 0.01f && raw <= 100.f) ? 1.f / ((cm + 1000.f) * (float)F) : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < 4 * NBARK; e += GT) (&tot[0][0][0])[e] = 0.f;  // (pass 5's band-ratio sums)

  // the audible sums of a frame
  auto sums = [&](const Bands &x, float &ac, float &an) {
    ac = 0.f;
    an = 0.f;
#pragma unroll 1
    for (int k = 0; k < NBARK; ++k) {
      const float ec = rho_s[k] * x.clean(k), n = x.den(k);
      ac += (ec > kThresh[k]) ? ec : 0.f;
      an += (n > kThresh[k]) ? n : 0.f;
    }
  };
  // ---- pass 2a: frame ratios
  for (int f = tid; f < F; f += GT) {
    float ac, an;
    sums(bands(f), ac, an);
    frv[f] = (ac + 5e3f) / (an + 5e3f);
  }
  __syncthreads();
  auto ratio = [&](int f) { return (f >= 1) ? 0.8f * frv[f] + 0.2f * frv[f - 1] : frv[f]; };
  float dummy = 0.f;
  // ---- pass 2b: frame disturbances
  for (int f = tid; f < F; f += GT) {
    const Bands x = bands(f);
    float ac, an;
    sums(x, ac, an);
    const float r = fminf(fmaxf(ratio(f), 3e-4f), 5.f);
    const FrameOut o = frame_pass<0>(x, true, rho_s, r, ac, 0.f, 0.f, 0.f, 0.f, dummy, dummy, nullptr, nullptr, lane);
    Sv[f] = o.S;
    Av[f] = o.A;
  }
  __syncthreads();
  // ---- pass 3: pooling in double, and what its reverse needs: ps^-4 per window, the distances
  const int nw = (F - 20) / 10 + 1;
  double as_ = 0.0, aa_ = 0.0;
  for (int w = tid; w < nw; w += GT) {
    double ps, pa;
    window_l6(w, [&](int f, double &xs, double &y) { xs = Sv[f], y = Av[f]; }, ps, pa);
    as_ += ps * ps;
    aa_ += pa * pa;
    const double ps2 = ps * ps, pa2 = pa * pa;
    winv[w] = ps > 0.0 ? 1.0 / (ps2 * ps2) : 0.0;
    winv[nw + w] = pa > 0.0 ? 1.0 / (pa2 * pa2) : 0.0;
  }
  as_ = wave_sum_d(as_);
  aa_ = wave_sum_d(aa_);
  if (lane == 0) {
    dred[0][wv] = as_;
    dred[1][wv] = aa_;
  }
  __syncthreads();
  if (tid == 0) {
    const double ts = ((dred[0][0] + dred[0][1]) + dred[0][2]) + dred[0][3];
    const double ta = ((dred[1][0] + dred[1][1]) + dred[1][2]) + dred[1][3];
    const double ds = sqrt(ts / nw), da = sqrt(ta / nw);
    const double e = mos_exp(mos_raw(ds, da));
    const double dm = (double)g_mos[b] * kMosSpan * kMosSlope * e / ((1.0 + e) * (1.0 + e));  // dL/d raw (mos_of)
    const double gds = (g_sym ? (double)g_sym[b] : 0.0) - kMosSym * dm;
    const double gda = (g_asym ? (double)g_asym[b] : 0.0) - kMosAsym * dm;
    // d ds / d S_f = S_f^5 / (20 nw ds) sum over the frame's windows of ps^-4
    gd_s[0] = ds > 0.0 ? gds / (20.0 * nw * ds) : 0.0;
    gd_s[1] = da > 0.0 ? gda / (20.0 * nw * da) : 0.0;
  }
  __syncthreads();
  const double cs = gd_s[0], ca = gd_s[1];
  auto pooled = [&](int f, float &gS, float &gA) {
    const int j1 = f / 10, j0 = j1 - 1;
    double is = 0.0, ia = 0.0;
    if (j0 >= 0 && j0 < nw) {  // (f < 10 j0 + 20 always)
      is += winv[j0];
      ia += winv[nw + j0];
    }
    if (j1 < nw) {
      is += winv[j1];
      ia += winv[nw + j1];
    }
    const double xs = Sv[f], y = Av[f];
    const double x2 = xs * xs, y2 = y * y;
    gS = (float)(cs * (x2 * x2 * xs) * is);
    gA = (float)(ca * (y2 * y2 * y) * ia);
  };
  // ---- pass 4: each frame's gradient of its smoothed ratio, and the weight's share of g_ac
  for (int f = tid; f < F; f += GT) {
    const Bands x = bands(f);
    float ac, an, gS, gA, g_r = 0.f, g_acw = 0.f;
    sums(x, ac, an);
    pooled(f, gS, gA);
    const float raw_r = ratio(f);
    const float r = fminf(fmaxf(raw_r, 3e-4f), 5.f);
    frame_pass<1>(x, true, rho_s, r, ac, gS, gA, 0.f, 0.f, g_r, g_acw, nullptr, nullptr, lane);
    gtv[f] = (raw_r >= 3e-4f && raw_r <= 5.f) ? g_r : 0.f;
    gav[f] = g_acw;
  }
  __syncthreads();
  // ---- pass 5: the frames' gradients, final but for the band ratio, and the band ratio's sums
  for (int f0 = 0; f0 < F; f0 += GT) {
    const int f = f0 + tid;
    const bool valid = f < F;
    const int fi = valid ? f : F - 1;
    const Bands x = bands(fi);
    float ac, an, gS, gA;
    sums(x, ac, an);
    pooled(fi, gS, gA);
    const float r = fminf(fmaxf(ratio(fi), 3e-4f), 5.f);
    // raw_r[f] = (0.8 | 1) fr[f] + 0.2 fr[f - 1]: fr[f] reaches frames f and f + 1
    const float g_fr = ((fi >= 1) ? 0.8f : 1.f) * gtv[fi] + ((fi + 1 < F) ? 0.2f * gtv[fi + 1] : 0.f);
    const float g_ac = gav[fi] + g_fr / (an + 5e3f);
    const float g_an = -g_fr * frv[fi] / (an + 5e3f);
    frame_pass<2>(x, valid, rho_s, r, ac, gS, gA, g_ac, g_an, dummy, dummy, qb + fi, tot[0][wv], lane);
  }
  __syncthreads();  // (a thread's q stores are its own to read back)
  if (tid < NBARK) gmn_s[tid] *= ((tot[0][0][tid] + tot[0][1][tid]) + tot[0][2][tid]) + tot[0][3][tid];
  __syncthreads();
  // ---- pass 6: the band ratio's term, sum G N, and q = G sigma_d corr
  double dot = 0.0;
  for (int f = tid; f < F; f += GT) {
    const bool keep = keepv[f] != 0.f;
    const Bands x = bands(f);
    float d = 0.f;
#pragma unroll 1
    for (int k = 0; k < NBARK; ++k) {
      const float n = x.den(k);
      const float G = qb[k * fld + f] + ((keep && n > kThresh[k] * 100.f) ? gmn_s[k] : 0.f);
      d = fmaf(G, n, d);
      qb[k * fld + f] = G * sn * kBarkCorr[k];
    }
    dot += (double)d;
  }
  dot = wave_sum_d(dot);
  if (lane == 0) dred[0][wv] = dot;
  __syncthreads();
  if (tid == 0) {
    const double t = ((dred[0][0] + dred[0][1]) + dred[0][2]) + dred[0][3];
    // d sigma / d x = -(sigma / P) 2 BP^T u, with u = g BP_raw x and P = g^2 sum (BP_raw x)^2
    coef[b] = (float)(2.0 * (double)(kBpGain * kBpGain) * t / (double)pwn);
    okv[b] = 1;
  }
}

// ------------------------------------------------------------------------------ tile filters
// Band-pass cascade, one sample (the forward's bp_section, five sections, no gain).  T = float for
// the samples, double for the chunk transition (iir_tile).
template <class T>
__device__ __forceinline__ T bp_run(T u, T z[10]) {
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const T y = u + z[2 * k];
    z[2 * k] = fma(-(T)kBpSecA[k][0], y, z[2 * k + 1]);
    z[2 * k + 1] = fma(-(T)kBpSecA[k][1], y, -u);
    u = y;
  }
  return u;
}
// Pre-emphasis all-pole part on the input's second difference (pesq.hip, pre_fir / pre_ap):
// z[0] = y[n-1], z[1] = y[n-2]; the numerator's b0 multiplies the output.
template <class T>
__device__ __forceinline__ T pre_run(T dd, T z[2]) {
  const T y = fma(-(T)kPreA[1], z[0], fma(-(T)kPreA[2], z[1], dd));
  z[1] = z[0];
  z[0] = y;
  return y;
}

template <bool BP, class T>
__device__ __forceinline__ T iir_run(T v, T *z) {
  if (BP) return bp_run<T>(v, z);
  return pre_run<T>(v, z);
}

// The filter over a tile in LDS, in place: tile[i] is the input at filter time i (REV: stored at
// GTILE - 1 - i), zero state before the tile.  Outputs of the first GWC chunks are warm-up unless
// the input before the tile is truly zero.  est: [GT][NS] doubles, mat: [4][NS][NS] doubles of LDS.
// The lanes' start states come from a 4-level Hillis-Steele scan of the chunks' zero-state end
// states with the chunk transition's powers M^(2^l) (formed here: M from zero-input runs, then
// three squarings): after it lane j holds sum_{m=0..15} M^m e_(j-m), its chunk's true end state.
// The transition, its powers and the scan are in double: in the filters' own state basis the
// pre-emphasis states are two nearly equal numbers (pesq.hip's tables change the basis for that), and
// with a float32 scan the tests' 40000-sample row measured 3.4e-3 of its largest element, 1.3e-3 so.
template <bool BP, bool REV>
__device__ __forceinline__ void iir_tile(float *__restrict__ tile, double *__restrict__ est, double *__restrict__ mat,
                                         int tid) {
  constexpr int NS = BP ? 10 : 2;
  // the pre-emphasis recursion runs in double (two states: no measurable cost): its resonance at 71 Hz
  // (poles at radius 0.973) amplifies a float32 recursion's rounding; measured, the tests' worst row
  // error went from 1.8e-3 to 1.4e-3 of the row's largest element, so it is not the largest term
  using ST = typename std::conditional<BP, float, double>::type;
  float4 *__restrict__ t4 = reinterpret_cast<float4 *>(tile);
  // chunk tid as 13 float4s in filter-time order (REV: read backwards, components swapped)
  auto q4 = [&](int q) -> float4 & { return t4[REV ? GTILE / 4 - 1 - (tid * (GCH / 4) + q) : tid * (GCH / 4) + q]; };
  float x[GCH];
#pragma unroll
  for (int q = 0; q < GCH / 4; ++q) {
    const float4 v = q4(q);
    x[4 * q] = REV ? v.w : v.x;
    x[4 * q + 1] = REV ? v.z : v.y;
    x[4 * q + 2] = REV ? v.y : v.z;
    x[4 * q + 3] = REV ? v.x : v.w;
  }
  if (!BP) {  // second differences of the input, from first differences (exact for neighbours)
    static_assert(BP || !REV, "the pre-emphasis tiles are loaded in filter-time order");
    const int i0 = tid * GCH;
    const float xm1 = tid > 0 ? tile[i0 - 1] : 0.f, xm2 = tid > 0 ? tile[i0 - 2] : 0.f;
    float h1 = xm1, d1 = xm1 - xm2;
#pragma unroll
    for (int i = 0; i < GCH; ++i) {
      const float d = x[i] - h1;
      h1 = x[i];
      x[i] = d - d1;
      d1 = d;
    }
  }
  // chunk transition: column tid of M = the end state of a zero-input run from unit state tid
  if (tid < NS) {
    double z[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = (s == tid) ? 1.0 : 0.0;
    for (int i = 0; i < GCH; ++i) iir_run<BP, double>(0.0, z);
#pragma unroll
    for (int s = 0; s < NS; ++s) mat[s * NS + tid] = z[s];
  }
  double zd[NS];  // zero-state end state of this chunk
  {
    ST z[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) z[s] = 0;
#pragma unroll
    for (int i = 0; i < GCH; ++i) iir_run<BP, ST>((ST)x[i], z);
#pragma unroll
    for (int s = 0; s < NS; ++s) est[tid * NS + s] = zd[s] = (double)z[s];
  }
  __syncthreads();  // (also: every lane holds its inputs before any output is written)
  for (int l = 0; l < 3; ++l) {  // M^(2^(l+1)) = M^(2^l) M^(2^l)
    if (tid < NS * NS) {
      const double *m = mat + l * NS * NS;
      const int r = tid / NS, c = tid - r * NS;
      double a = 0.0;
#pragma unroll
      for (int t = 0; t < NS; ++t) a = fmaf(m[r * NS + t], m[t * NS + c], a);
      mat[(l + 1) * NS * NS + tid] = a;
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int l = 0; l < 4; ++l) {
    const int j = tid - (1 << l);
    double pz[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) pz[s] = (j >= 0) ? est[(j < 0 ? 0 : j) * NS + s] : 0.0;
    __syncthreads();  // every lane has read its partner before anyone overwrites
    const double *m = mat + l * NS * NS;
    double zn[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      double a = zd[s];
#pragma unroll
      for (int t = 0; t < NS; ++t) a = fma(m[s * NS + t], pz[t], a);
      zn[s] = a;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) est[tid * NS + s] = zd[s] = zn[s];
    __syncthreads();
  }
  ST z[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) z[s] = tid > 0 ? (ST)est[(tid - 1) * NS + s] : (ST)0;  // the end state of the chunk before
#pragma unroll
  for (int q = 0; q < GCH / 4; ++q) {
    float y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const ST v = iir_run<BP, ST>((ST)x[4 * q + c], z);
      y[c] = BP ? (float)v : (float)(v * (ST)kPreB[0]);
    }
    q4(q) = REV ? make_float4(y[3], y[2], y[1], y[0]) : make_float4(y[0], y[1], y[2], y[3]);
  }
  __syncthreads();
}

struct TileLds {
  __attribute__((aligned(16))) float tile[GTILE];
  double est[GT * 10];
  double mat[4 * 100];
};
static_assert(2 * sizeof(TileLds) <= 160 * 1024, "two workgroups per CU");

// y = PRE(taper x) of the denoised rows (unscaled), samples [0, L_b) of row b.
__global__ void __launch_bounds__(GT)
    pesq_pre_fwd(const float *__restrict__ deg, int64_t ld, int64_t Lcap, const int32_t *__restrict__ lens,
                 const int *__restrict__ okv, float *__restrict__ ys, int64_t yld, int64_t b0) {
  __shared__ TileLds s;
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int64_t L = row_length(lens, b, Lcap);
  const int64_t own0 = (int64_t)blockIdx.x * OWN_PRE;
  if (!okv[b] || own0 >= L) return;  // (uniform)
  const int64_t t0 = own0 - GWARM;
  const float *__restrict__ xr = deg + b * ld;
  const float Lf = (float)L;
  for (int i = tid; i < GTILE; i += GT) {
    const int64_t t = t0 + i;
    s.tile[i] = (t >= 0 && t < L) ? xr[t] * taper_w((float)t, Lf) : 0.f;
  }
  __syncthreads();
  iir_tile<false, false>(s.tile, s.est, s.mat, tid);
  float *__restrict__ yr = ys + b * yld;
  for (int i = GWARM + tid; i < GTILE; i += GT) {
    const int64_t t = t0 + i;
    if (t < L) yr[t] = s.tile[i];
  }
}

// grad[b, t] = -coef_b BP_raw^T(BP_raw x)[t] for t < L_b (an ok row), 0 elsewhere in [0, length).
__global__ void __launch_bounds__(GT)
    pesq_power_grad(const float *__restrict__ deg, int64_t ld, int64_t Lcap, const int32_t *__restrict__ lens,
                    const int *__restrict__ okv, const float *__restrict__ coef, float *__restrict__ grad,
                    int64_t grad_ld, int64_t b0) {
  __shared__ TileLds s;
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int64_t L = row_length(lens, b, Lcap);
  const int64_t own0 = (int64_t)blockIdx.x * OWN_BP;
  const int64_t t0 = own0 - GWARM;
  float *__restrict__ gr = grad + b * grad_ld;
  if (!okv[b] || own0 >= L) {  // (uniform)
    for (int i = GWARM + tid; i < GWARM + OWN_BP; i += GT)
      if (t0 + i < Lcap) gr[t0 + i] = 0.f;
    return;
  }
  const float *__restrict__ xr = deg + b * ld;
  for (int i = tid; i < GTILE; i += GT) {
    const int64_t t = t0 + i;
    s.tile[i] = (t >= 0 && t < L) ? xr[t] : 0.f;
  }
  __syncthreads();
  iir_tile<true, false>(s.tile, s.est, s.mat, tid);
  // the power sums u over [0, L): nothing after the row's end reaches the reversed filter
  for (int i = tid; i < GTILE; i += GT) {
    const int64_t t = t0 + i;
    if (t < 0 || t >= L) s.tile[i] = 0.f;
  }
  __syncthreads();
  iir_tile<true, true>(s.tile, s.est, s.mat, tid);
  const float cf_ = -coef[b];
  for (int i = GWARM + tid; i < GWARM + OWN_BP; i += GT) {
    const int64_t t = t0 + i;
    if (t < Lcap) gr[t] = (t < L) ? cf_ * s.tile[i] : 0.f;
  }
}

// grad[b, t] += taper(t) PRE^T(gy)[t] for t < L_b (ok rows): filter time i is sample L - 1 - i.
__global__ void __launch_bounds__(GT)
    pesq_pre_grad(const float *__restrict__ gy, int64_t gld, int64_t Lcap, const int32_t *__restrict__ lens,
                  const int *__restrict__ okv, float *__restrict__ grad, int64_t grad_ld, int64_t b0) {
  __shared__ TileLds s;
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.y;
  const int64_t L = row_length(lens, b, Lcap);
  const int64_t own0 = (int64_t)blockIdx.x * OWN_PRE;
  if (!okv[b] || own0 >= L) return;  // (uniform)
  const int64_t i0 = own0 - GWARM;
  const float *__restrict__ gr_in = gy + b * gld;
  for (int i = tid; i < GTILE; i += GT) {
    const int64_t t = L - 1 - (i0 + i);
    s.tile[i] = (t >= 0 && t < L) ? gr_in[t] : 0.f;
  }
  __syncthreads();
  iir_tile<false, false>(s.tile, s.est, s.mat, tid);
  float *__restrict__ gr = grad + b * grad_ld;
  const float Lf = (float)L;
  for (int i = GWARM + tid; i < GTILE; i += GT) {
    const int64_t t = L - 1 - (i0 + i);
    if (t >= 0) gr[t] = fmaf(taper_w((float)t, Lf), s.tile[i], gr[t]);
  }
}

// ------------------------------------------------------------------------------ front end, reversed
// Hops [15 x, 15 x + 15) of row b: gy[t] = sum over the (at most two) frames over sample t of
// hann[n] Re sum_{j=1..255} 2 q[f, band(j)] Y_f[j] e^(+2 pi i j n / 512), 0 from the row's end on.
__global__ void __launch_bounds__(GT)
    pesq_front_grad(const float *__restrict__ ys, int64_t yld, int64_t Lcap, const int32_t *__restrict__ lens,
                    const int *__restrict__ okv, const float *__restrict__ q, int64_t B, int Fcap,
                    float *__restrict__ gy, int64_t gld, int64_t b0) {
  __shared__ float fr[NHOP + 1][512];
  __shared__ float2 xbuf[4 * kFftBuf];
  __shared__ float qb[NHOP + 1][NBARK + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t b = b0 + blockIdx.y;
  const int64_t L = row_length(lens, b, Lcap);
  const int m0 = (int)blockIdx.x * NHOP;
  if (!okv[b] || (int64_t)m0 * 256 >= L) return;  // (uniform; pesq_pre_grad reads gy below L only)
  const int F = frames_of(L);
  const int64_t fld = bark_ld(Fcap);
  const float *__restrict__ qr = q + b * NBARK * fld;
  const float *__restrict__ yr = ys + b * yld;
  // frame i of the workgroup is frame m0 - 1 + i of the row
  for (int e = tid; e < (NHOP + 1) * (NBARK + 1); e += GT) {
    const int i = e / (NBARK + 1), k = e - i * (NBARK + 1);
    const int f = m0 - 1 + i;
    qb[i][k] = (f >= 0 && f < F && k >= 1 && k < NBARK) ? qr[k * fld + f] : 0.f;  // (band 0 is the zeroed bin 0)
  }
  __syncthreads();
  cf tw1[8], tw2[8];
  fft512_twiddles(lane, tw1, tw2);
  float2 *wbuf = xbuf + wave * kFftBuf;
  const int plane = (64 - lane) & 63;
  float win[8];
  int band[4];
#pragma unroll
  for (int r = 0; r < 8; ++r) win[r] = kHann512[lane + 64 * r];
#pragma unroll
  for (int r = 0; r < 4; ++r) band[r] = (lane + 64 * r == 0) ? NBARK : kBandOfBin[lane + 64 * r];  // qb[.][49] = 0
  for (int p = wave; p < (NHOP + 1) / 2; p += 4) {
    const int ia = 2 * p, fa = m0 - 1 + ia, fb = fa + 1;
    const bool has_a = fa >= 0 && fa < F, has_b = fb >= 0 && fb < F;
    cf v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int n = lane + 64 * r;
      const int64_t ta = (int64_t)fa * 256 + n, tb = ta + 256;
      const float a = (has_a && ta < L) ? yr[ta] : 0.f;
      const float bq = (has_b && tb < L) ? yr[tb] : 0.f;
      v[r] = {a * win[r], bq * win[r]};
    }
    fft512_wave<false>(v, wbuf, lane, tw1, tw2);
    // Ya = (Z[k] + conj Z[N-k]) / 2, Yb = (Z[k] - conj Z[N-k]) / 2i; G = q Y on bins 1..255;
    // W[k] = conj(Ga + i Gb), W[N-k] = conj(conj Ga + i conj Gb): the transform of W is
    // conj(ga + i gb) with g = Re sum 2 G e^(+i ...), both frames' sample gradients
    cf u[8];
    pair_grad_fold(
        v,
        [&](int r, float &ca, float &cb) {
          ca = 0.5f * qb[ia][band[r]];
          cb = 0.5f * qb[ia + 1][band[r]];
        },
        lane, plane, u);
    fft512_wave<false>(u, wbuf, lane, tw1, tw2);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      fr[ia][lane + 64 * r] = win[r] * u[r].r;
      fr[ia + 1][lane + 64 * r] = -win[r] * u[r].i;
    }
    wave_lds_fence();
  }
  __syncthreads();
  float *__restrict__ go = gy + b * gld;
  for (int h = 0; h < NHOP; ++h) {
    const int64_t t = (int64_t)(m0 + h) * 256 + tid;
    // frame m0 + h - 1's upper half, then frame m0 + h's lower half
    if (t < L) go[t] = fr[h][256 + tid] + fr[h + 1][tid];
  }
}

// ------------------------------------------------------------------------------ host side
struct GradState {
  WbWs fwd;
  float *scratch;
  double *dscratch;
  float *q, *coef;
  int *ok;
  float *ys, *gy;
  int64_t yld;
};
static GradState state_layout(Arena &a, int64_t batch, int64_t length) {
  GradState s;
  const Geometry g = geometry(length);
  s.fwd = wb_layout(a, batch, length);
  s.scratch = a.take<float>((size_t)batch * (size_t)g.F * SCR);
  s.dscratch = a.take<double>((size_t)batch * (size_t)g.F);
  s.q = a.take<float>((size_t)batch * NBARK * (size_t)bark_ld(g.F));
  s.coef = a.take<float>((size_t)batch);
  s.ok = a.take<int>((size_t)batch);
  s.yld = (length + 255) / 256 * 256;
  s.ys = a.take<float>((size_t)batch * (size_t)s.yld);
  s.gy = a.take<float>((size_t)batch * (size_t)s.yld);
  return s;
}

static int run_grad(const float *deg, int64_t B, int64_t length, int64_t ld, const int32_t *lengths, const GradState &s,
                    const float *g_mos, const float *g_sym, const float *g_asym, float *grad, int64_t grad_ld,
                    hipStream_t st) {
  const Geometry g = geometry(length);
  if (B > 0x7fffffff) return FSEM_EINVAL;
  hipLaunchKernelGGL(pesq_back_grad, dim3((unsigned)B), dim3(GT), 0, st, s.fwd.bark, s.fwd.front.ppart, s.fwd.front.rng,
                     g.nseg, B, length, lengths, g.F, g_mos, g_sym, g_asym, s.scratch, s.dscratch, s.q, s.coef, s.ok);
  FSEM_CHECK_LAUNCH();
  const unsigned npre = (unsigned)((length + OWN_PRE - 1) / OWN_PRE), nbp = (unsigned)((length + OWN_BP - 1) / OWN_BP);
  const unsigned nhop = (unsigned)(((length + 255) / 256 + NHOP - 1) / NHOP);
  for (int64_t b0 = 0; b0 < B; b0 += kMaxGridY) {
    hipLaunchKernelGGL(pesq_pre_fwd, grid_slice(npre, B, b0), dim3(GT), 0, st, deg, ld, length, lengths, s.ok, s.ys,
                       s.yld, b0);
    FSEM_CHECK_LAUNCH();
    hipLaunchKernelGGL(pesq_front_grad, grid_slice(nhop, B, b0), dim3(GT), 0, st, s.ys, s.yld, length, lengths, s.ok,
                       s.q, B, g.F, s.gy, s.yld, b0);
    FSEM_CHECK_LAUNCH();
    hipLaunchKernelGGL(pesq_power_grad, grid_slice(nbp, B, b0), dim3(GT), 0, st, deg, ld, length, lengths, s.ok, s.coef,
                       grad, grad_ld, b0);
    FSEM_CHECK_LAUNCH();
    hipLaunchKernelGGL(pesq_pre_grad, grid_slice(npre, B, b0), dim3(GT), 0, st, s.gy, s.yld, length, lengths, s.ok,
                       grad, grad_ld, b0);
    FSEM_CHECK_LAUNCH();
  }
  return FSEM_OK;
}

}  // namespace pesq
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_pesq_state_floats(int64_t batch, int64_t length) {
  if (batch < 0 || length <= 0 || length > kMaxLength) return 0;
  return (int64_t)(layout_bytes(pesq::state_layout, batch > 0 ? batch : 1, length) / sizeof(float));
}

extern "C" int fsem_pesq_state_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                   const int32_t *lengths, float *mos, float *dist, float *state, void *stream) {
  if (!ref || !deg || !mos || !state || batch < 0 || length <= 0 || ld < length || length > kMaxLength)
    return FSEM_EINVAL;
  if (pesq::geometry(length).F < 20 && !lengths) return FSEM_ESHORT;
  if (batch == 0) return FSEM_OK;
  Arena a(state);
  const pesq::GradState s = pesq::state_layout(a, batch, length);
  const hipStream_t st = (hipStream_t)stream;
  const int rc = pesq::launch_front(ref, deg, batch, length, ld, lengths, s.fwd.bark, s.fwd.power, s.fwd.front, nullptr,
                                    0, nullptr, 0, st, /*power_sums=*/false);
  if (rc != FSEM_OK) return rc;
  return pesq::launch_back(s.fwd.bark, nullptr, &s.fwd.front, batch, length, lengths, mos, s.fwd.back, st, dist, nullptr);
}

extern "C" int fsem_pesq_grad_f32(const float *deg, int64_t batch, int64_t length, int64_t ld, const int32_t *lengths,
                                  float *state, const float *g_mos, const float *g_sym, const float *g_asym,
                                  float *grad, int64_t grad_ld, void *stream) {
  if (!deg || !state || !g_mos || !grad || batch < 0 || length <= 0 || ld < length || grad_ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  if (batch == 0) return FSEM_OK;
  Arena a(state);
  const pesq::GradState s = pesq::state_layout(a, batch, length);
  return pesq::run_grad(deg, batch, length, ld, lengths, s, g_mos, g_sym, g_asym, grad, grad_ld, (hipStream_t)stream);
}
