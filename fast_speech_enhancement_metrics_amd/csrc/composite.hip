// Composite measures of (clean, denoised) rows after Hu & Loizou 2008: CSIG, CBAK, COVL from the
// engine's PESQ MOS, the log-likelihood ratio (LLR), the weighted spectral slope (WSS) and the
// segmental SNR (include/fsem_composite.h).  Replaces nothing in the reference.
//
//   composite_tables  the frame window (evaluated in double, stored float32) and the sparse band
//                     filters: 25 bands x GW bins from bin f0 - GO of each band (the filters are
//                     zero outside +-14 bins after the threshold), once per call.
//   composite_frames  grid (chunk, row), 4 waves.  A chunk is KF frames: its (KF + 3) hop samples
//                     of both rows are staged in LDS once (frames overlap by 75 %), with the
//                     row's non-finite flag of the chunk.  A wave takes every fourth frame:
//                       - the windowed frames w[t] x[t] (float32 products) to LDS;
//                       - autocorrelation R[0..P] of both in double: a lane takes RUN consecutive
//                         samples and their P successors from LDS into registers, the lags are
//                         register FMAs, the P + 1 sums (and the frame's noise energy for SegSNR)
//                         are reduced over the wave by xor exchanges (the same value in every lane);
//                       - Levinson-Durbin in double, even lanes on the clean frame, odd lanes on
//                         the denoised one, each lane's quadratic form with the clean Toeplitz
//                         matrix, LLR = ln(q_odd / q_even);
//                       - both spectra with fft512_wave_x2: at 16 kHz the 1024-point real
//                         transform as a 512-point complex one on even / odd samples plus the
//                         split step, at 8 kHz a 512-point transform with a zero imaginary part
//                         (clean and denoised never share a transform: a silent clean frame has
//                         an exactly zero spectrum);
//                       - the 25 band energies (one lane per signal and band, float32), then
//                         slopes, nearest peaks, weights and the weighted sum in double.
//                     One LLR, WSS and SegSNR value per frame to the workspace.
//   composite_rows    grid (value, row): LLR and WSS: the mean of the K smallest of the row's F
//                     frame values by a radix select over the floats' ordered bit patterns (four
//                     256-bin histogram passes, integer counts: any F), then the sum in double of
//                     everything below the K-th value plus its copies; SegSNR: the mean of all F.
//                     Each thread sums its strided values in order, the block's 256 sums are
//                     added in a fixed tree.
//   composite_combine one thread per row: non-finite and empty rows to NaN, the three composites.
//
// PESQ comes from the engine's whole-metric entry on the same stream (8 kHz rows resampled to
// 16 kHz into the workspace first, as the PESQ class does).  Every sum has one order, fixed by
// the sample rate alone: a row's scores do not depend on the batch size, the row's position, the
// row capacity or the stream.
#include <algorithm>
#include <math.h>

#include "../../include/fsem_composite.h"
#include "fsem_build_marker.h"
#include "fsem_internal.h"
#include "fsem_select.h"
#include "fsem_speech_frames.h"

namespace fsem {
namespace composite {

constexpr int T = 256;      // threads of a frame block
constexpr int NWAVE = T / 64;
constexpr int KF = 16;      // frames per chunk (under 64 KiB of LDS at both rates)
constexpr int NB = 25;      // critical bands
constexpr int GW = 32;      // bins per band in the sparse table
constexpr int GO = 15;      // table bin q of band i is spectrum bin f0_i - GO + q
constexpr int RT = 256;     // threads of a row block
constexpr int CT = 64;      // threads of a combine block

struct Geo : FrameGeo {
  int H, S;
  int64_t C;  // samples a chunk owns: KF hops (it stages S = (KF + 3) hop)
};

inline bool make_geo(int32_t sr, Geo *g) {
  if (!make_frame_geo(sr, g)) return false;
  g->H = sr == 8000 ? 256 : 512;
  g->S = (KF + 3) * g->hop;
  g->C = (int64_t)KF * g->hop;
  return true;
}

inline int64_t chunks(int64_t length, const Geo &g) { return (length + g.C - 1) / g.C; }

// Centre frequencies and bandwidths (Hz) of the 25 critical bands.
__constant__ double kCentreD[NB] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,   540.0,   617.372,
                                    703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54, 1610.70, 1794.16,
                                    1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
__constant__ double kWidthD[NB] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    77.3724,
                                   86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457,
                                   199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

// Tables in the workspace: win floats of window, NB * GW filter weights, NB first bins.
struct Tables {
  float *win;
  float *g;
  int *j0;
  float *tw;  // [512][2]: W_1024^j = tw[2 j] - i tw[2 j + 1], the split step's twiddles
};

__global__ void composite_tables(Tables tb, int win, int H, int sr) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < win) tb.win[t] = (float)(0.5 * (1.0 - cos(2.0 * 3.14159265358979323846 * (double)(t + 1) / (double)(win + 1))));
  if (t < NB * GW) {
    const int i = t / GW, q = t % GW;
    const double half = (double)sr / 2.0;
    const int f0 = (int)floor(kCentreD[i] * (double)H / half);
    const double bw = kWidthD[i] * (double)H / half;
    const int j = f0 - GO + q;
    const double x = (double)(j - f0) / bw;
    double v = exp(-11.0 * x * x + log(kWidthD[0]) - log(kWidthD[i]));
    if (v <= exp(-30.0 / (2.0 * 2.303)) || j < 0 || j >= H) v = 0.0;
    tb.g[t] = (float)v;
    if (q == 0) tb.j0[i] = f0 - GO;
  }
  if (t < 512) {
    double sn, cs;
    sincospi((double)t / 512.0, &sn, &cs);
    tb.tw[2 * t] = (float)cs;
    tb.tw[2 * t + 1] = (float)sn;
  }
}

__device__ __forceinline__ float frame_db(float S, float D) {
  const float v = 10.f * log10f(S / (D + 1e-10f) + 1e-10f);
  return fminf(fmaxf(v, -10.f), 35.f);
}

// R[k] = sum_t x[t] x[t + k], k = 0 .. P, over the windowed frame fw (win floats, then P zeros):
// this lane's RUN samples against their successors (the lane's part: the caller sums over the wave).
template <int P, int RUN>
__device__ __forceinline__ void autocorr(const float *__restrict__ fw, int lane, int win, double R[P + 1]) {
  double a[RUN + P];
  const int base = lane * RUN;
  const bool on = base < win;  // (win is a multiple of RUN)
#pragma unroll
  for (int i = 0; i < RUN + P; ++i) a[i] = on ? (double)fw[base + i] : 0.0;
#pragma unroll
  for (int k = 0; k <= P; ++k) {
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < RUN; ++i) r = fma(a[i], a[i + k], r);
    R[k] = r;
  }
}

// Prediction-error filter A = [1, a_1 .. a_P] of R by Levinson-Durbin, then q = A Toeplitz(Rs) A^T
// = Rs[0] sum a_i^2 + 2 sum_k Rs[k] sum_i a_i a_{i+k}: fsem_lpc.h's levinson and quadratic in one
// body.  Written as those two calls it computes the same bits, but composite_frames then compiles
// to other code (one index multiply signed, one or two more s_nop), so this one stays as it was.
template <int P>
__device__ __forceinline__ double lpc_quadratic(const double R[P + 1], const double Rs[P + 1]) {
  double a[P + 1];
  a[0] = 1.0;
#pragma unroll
  for (int i = 1; i <= P; ++i) a[i] = 0.0;
  double E = R[0];
#pragma unroll
  for (int i = 1; i <= P; ++i) {
    double acc = R[i];
#pragma unroll
    for (int j = 1; j < i; ++j) acc = fma(a[j], R[i - j], acc);
    const double k = -acc / E;
#pragma unroll
    for (int j = 1; 2 * j <= i; ++j) {
      const double u = a[j], v = a[i - j];
      a[j] = fma(k, v, u);
      if (j != i - j) a[i - j] = fma(k, u, v);
    }
    a[i] = k;
    E *= 1.0 - k * k;
  }
  double q = 0.0;
#pragma unroll
  for (int k = P; k >= 0; --k) {
    double c = 0.0;
#pragma unroll
    for (int i = 0; i + k <= P; ++i) c = fma(a[i], a[i + k], c);
    q = fma(k ? 2.0 * c : c, Rs[k], q);
  }
  return q;
}

// Band energies of one signal in registers (the same in every lane), their maximum, and the index
// of this lane's nearest peak (lane = band i < 24) for slopes sl[j] = e[j + 1] - e[j] (the published
// search, its quirk kept): rising, the band before the first slope m >= i that does not rise (24
// when all do); else the band after the last slope m <= i that does not fall (-1 when all do).
__device__ __forceinline__ int nearest_peak_index(const float *__restrict__ e, int lane, float *emax) {
  float ev[NB];
#pragma unroll
  for (int m = 0; m < NB; ++m) ev[m] = e[m];
  float mx = ev[0];
#pragma unroll
  for (int m = 1; m < NB; ++m) mx = fmaxf(mx, ev[m]);
  *emax = mx;
  int cur = NB - 1, nxt = NB - 1;
#pragma unroll
  for (int m = NB - 2; m >= 0; --m) {
    cur = ev[m + 1] > ev[m] ? cur : m;
    if (m == lane) nxt = cur;
  }
  int prv = -1;
  cur = -1;
#pragma unroll
  for (int m = 0; m < NB - 1; ++m) {
    cur = ev[m + 1] <= ev[m] ? cur : m;
    if (m == lane) prv = cur;
  }
  return e[lane + 1] > e[lane] ? nxt - 1 : prv + 1;
}

struct FrameOut {
  float *llr, *wss, *seg;  // [batch, Fld] each
};

inline size_t frames_lds(const Geo &g) {
  size_t b = 2 * (size_t)g.S * 4;                       // staged rows
  b += (size_t)g.win * 4;                               // window
  b += (size_t)NB * GW * 4 + 32 * 4;                    // filters, first bins
  b += (size_t)NWAVE * 2 * (size_t)(g.win + g.P) * 4;   // windowed frames
  b += (size_t)NWAVE * kFftBuf * 8;                     // FFT exchange / power spectra
  b += (size_t)NWAVE * 64 * 4;                          // band energies
  return align_up(b, 16) + 64;
}

template <int P, bool WIDE>
__global__ __launch_bounds__(T) void composite_frames(const float *__restrict__ ref, const float *__restrict__ deg,
                                                      int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                      int64_t r0, Tables tb, FrameOut out, int64_t Fld,
                                                      int *__restrict__ flags, int nchunk) {
  constexpr int RUN = WIDE ? 8 : 4;
  constexpr int hop = frame_hop(WIDE ? 16000 : 8000), win = 4 * hop, H = WIDE ? 512 : 256;
  constexpr int S = (KF + 3) * hop, FW = win + P;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2 *fbuf = reinterpret_cast<float2 *>(smem);       // [NWAVE][kFftBuf] (16-byte aligned rows)
  float *xs = reinterpret_cast<float *>(fbuf + NWAVE * kFftBuf);
  float *xd = xs + S;
  float *w = xd + S;
  float *gt = w + win;
  int *gj0 = reinterpret_cast<int *>(gt + NB * GW);
  float *fw = reinterpret_cast<float *>(gj0 + 32);       // [NWAVE][2][FW]
  float *eb = fw + NWAVE * 2 * FW;                       // [NWAVE][2][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = r0 + blockIdx.y;
  const int c = blockIdx.x;
  const int n = row_length(lengths, row, length);
  const int base = c * (KF * hop);
  if (base >= n) return;  // (the combine pass reads ceil(n / C) flags of this row)
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  int bad = 0;
  for (int i = tid; i < S; i += T) {
    const int gidx = base + i;
    const float a = gidx < n ? srow[gidx] : 0.f, b = gidx < n ? hrow[gidx] : 0.f;
    bad |= !(isfinite(a) && isfinite(b));
    xs[i] = a;
    xd[i] = b;
  }
  for (int i = tid; i < win; i += T) w[i] = tb.win[i];
  for (int i = tid; i < NB * GW; i += T) gt[i] = tb.g[i];
  if (tid < NB) gj0[tid] = tb.j0[tid];
  bad = __syncthreads_or(bad);
  if (tid == 0) flags[row * nchunk + c] = bad;
  const int F = frames_of(n, win, hop);
  float *fws = fw + wave * 2 * FW, *fwd = fws + FW;
  float2 *buf = fbuf + wave * kFftBuf;
  float *pw = reinterpret_cast<float *>(buf);  // [2][512] power spectra, after the transforms
  float *e = eb + wave * 64;                   // [2][32] band energies
  cf tw1[8], tw2[8];
  fft512_twiddles(lane, tw1, tw2);
  float wc[8], wsn[8];  // W_1024^j = wc - i wsn, j = lane + 64 r
  if (WIDE) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      wc[r] = tb.tw[2 * (lane + 64 * r)];
      wsn[r] = tb.tw[2 * (lane + 64 * r) + 1];
    }
  }
  const int plane = (64 - lane) & 63;
  for (int fl = wave; fl < KF; fl += NWAVE) {
    const int f = c * KF + fl;
    if (f >= F) break;  // (wave-uniform)
    // windowed frames, and the noise energy sum (w (s^ - s))^2 for SegSNR
    double dsum = 0.0;
    for (int t = lane; t < FW; t += 64) {
      float a = 0.f, b = 0.f;
      if (t < win) {
        const float x = xs[fl * hop + t], y = xd[fl * hop + t], wt = w[t];
        a = wt * x;
        b = wt * y;
        const float d = wt * (y - x);
        dsum = fma((double)d, (double)d, dsum);
      }
      fws[t] = a;
      fwd[t] = b;
    }
    wave_lds_fence();
    double Rs[P + 2], Rd[P + 1];
    autocorr<P, RUN>(fws, lane, win, Rs);
    autocorr<P, RUN>(fwd, lane, win, Rd);
    Rs[P + 1] = dsum;
    wave_sums_d<P + 2>(Rs);
    wave_sums_d<P + 1>(Rd);
    dsum = Rs[P + 1];
    double Rm[P + 1];
#pragma unroll
    for (int k = 0; k <= P; ++k) Rm[k] = (lane & 1) ? Rd[k] : Rs[k];
    const double q = lpc_quadratic<P>(Rm, Rs);
    const double qo = __shfl_xor(q, 1, 64);
    const float llr = (float)log((lane & 1) ? q / qo : qo / q);  // (0 / 0 and NaN filters: NaN)
    const float seg = frame_db((float)Rs[0], (float)dsum);
    // spectra
    cf va[8], vb[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int m = lane + 64 * r;
      if (WIDE) {
        const bool in = 2 * m < win;  // (win is even)
        va[r] = {in ? fws[2 * m] : 0.f, in ? fws[2 * m + 1] : 0.f};
        vb[r] = {in ? fwd[2 * m] : 0.f, in ? fwd[2 * m + 1] : 0.f};
      } else {
        const bool in = m < win;
        va[r] = {in ? fws[m] : 0.f, 0.f};
        vb[r] = {in ? fwd[m] : 0.f, 0.f};
      }
    }
    fft512_wave_x2(va, vb, buf, lane, tw1, tw2);
#pragma unroll
    for (int r = 0; r < (WIDE ? 8 : 4); ++r) {
      const int j = lane + 64 * r;
      if (WIDE) {
        cf am, bm;
        split_mirrors(va, vb, r, lane, plane, am, bm);
        const cf xa = split_bin(va[r], am, wc[r], wsn[r]);
        pw[j] = xa.r * xa.r + xa.i * xa.i;
        const cf xb = split_bin(vb[r], bm, wc[r], wsn[r]);
        pw[512 + j] = xb.r * xb.r + xb.i * xb.i;
      } else {
        pw[j] = va[r].r * va[r].r + va[r].i * va[r].i;
        pw[512 + j] = vb[r].r * vb[r].r + vb[r].i * vb[r].i;
      }
    }
    wave_lds_fence();
    // band energies: lanes 0 .. 24 the clean frame's, lanes 32 .. 56 the denoised frame's
    {
      const int sig = lane >> 5, i = lane & 31;
      if (i < NB) {
        const float acc = band_sum<GW>(pw + sig * 512, gt + i * GW, gj0[i], H);
        e[sig * 32 + i] = 10.f * log10f(fmaxf(acc, 1e-10f));
      }
    }
    wave_lds_fence();
    double num = 0.0, den = 0.0;
    if (lane < NB - 1) {
      double W = 0.0, sl[2];
#pragma unroll
      for (int sig = 0; sig < 2; ++sig) {
        const float *__restrict__ es = e + sig * 32;
        float emax;
        const double pk = es[nearest_peak_index(es, lane, &emax)];
        const double ei = es[lane];
        sl[sig] = (double)es[lane + 1] - ei;
        W += 20.0 / (20.0 + (double)emax - ei) * (1.0 / (1.0 + pk - ei));
      }
      W *= 0.5;
      const double ds = sl[0] - sl[1];
      num = W * ds * ds;
      den = W;
    }
    double nd[2] = {num, den};
    wave_sums_d<2>(nd);
    num = nd[0], den = nd[1];
    if (lane == 0) {
      out.llr[row * Fld + f] = llr;
      out.wss[row * Fld + f] = (float)(num / den);
      out.seg[row * Fld + f] = seg;
    }
    wave_lds_fence();  // the next frame overwrites the wave's buffers
  }
}

__global__ __launch_bounds__(RT) void composite_rows(FrameOut fr, int64_t Fld, int64_t B,
                                                     const int32_t *__restrict__ lengths, int length, int hop,
                                                     float *__restrict__ llr, float *__restrict__ wss,
                                                     float *__restrict__ seg) {
  static_assert(RT == 256, "select_kth is a 256-thread block's");
  __shared__ struct {
    SelectLds sel;
    double red[RT / 64];
  } s;
  const int which = blockIdx.x, tid = threadIdx.x;
  const int64_t row = grid_row_yz();
  if (row >= B) return;
  const int n = row_length(lengths, row, length);
  const int win = 4 * hop;
  const int F = frames_of(n, win, hop);
  float *__restrict__ dst = which == 0 ? llr : which == 1 ? wss : seg;
  if (F == 0) {
    if (tid == 0) dst[row] = __builtin_nanf("");
    return;
  }
  const float *__restrict__ v = (which == 0 ? fr.llr : which == 1 ? fr.wss : fr.seg) + row * Fld;
  const bool trimmed = which != 2;
  const int K = trimmed ? (int)((19 * (int64_t)F + 10) / 20) : F;
  uint32_t kth = 0xFFFFFFFFu;  // the K-th smallest key
  int need = 0;                // copies of it among the K smallest
  if (trimmed) kth = select_kth(v, F, K, s.sel, &need);  // (block-uniform)
  double acc = 0.0;
  for (int i = tid; i < F; i += RT) {
    const float x = v[i];
    if (!trimmed || order_key(x) < kth) acc += (double)x;
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) s.red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double total = (s.red[0] + s.red[1]) + (s.red[2] + s.red[3]);
    if (trimmed) total += (double)need * (double)key_value(kth);
    dst[row] = (float)(total / (double)K);
  }
}

__device__ __forceinline__ float clamp15(double v) {
  return v != v ? __builtin_nanf("") : (float)fmin(fmax(v, 1.0), 5.0);
}

__global__ __launch_bounds__(CT) void composite_combine(const int *__restrict__ flags, int nchunk,
                                                        const int32_t *__restrict__ lengths, int length, int64_t B,
                                                        int C, float *__restrict__ csig, float *__restrict__ cbak,
                                                        float *__restrict__ covl, float *__restrict__ pesq,
                                                        float *__restrict__ llr, float *__restrict__ wss,
                                                        float *__restrict__ seg) {
  const int64_t b = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (b >= B) return;
  const int n = row_length(lengths, b, length);
  const int nc = (n + C - 1) / C;
  int bad = n == 0;
  for (int c = 0; c < nc; ++c) bad |= flags[b * nchunk + c];
  if (bad) {  // an empty row, or one holding a non-finite sample
    csig[b] = cbak[b] = covl[b] = pesq[b] = llr[b] = wss[b] = seg[b] = __builtin_nanf("");
    return;
  }
  const double p = pesq[b], l = llr[b], w = wss[b], s = seg[b];
  csig[b] = clamp15(3.093 - 1.029 * l + 0.603 * p - 0.009 * w);
  cbak[b] = clamp15(1.634 + 0.478 * p - 0.007 * w + 0.063 * s);
  covl[b] = clamp15(1.594 + 0.805 * p - 0.512 * l - 0.007 * w);
}

__global__ void composite_len16(const int32_t *__restrict__ lengths, int length, int64_t B, int32_t *__restrict__ len16) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) len16[b] = 2 * row_length(lengths, b, length);
}

// Workspace: tables, per-frame values, chunk flags, the 16 kHz copies of 8 kHz rows with their
// lengths, the PESQ entry's workspace.
struct Ws {
  Tables tb;
  FrameOut fr;
  int64_t Fld;
  int *flags;
  float *up;        // [2 batch, ld16] (8 kHz only)
  int32_t *len16;   // [batch]        (8 kHz only)
  int64_t L16, ld16;
  char *pesq;
  size_t pesq_bytes;
};
inline Ws layout(Arena &a, int64_t batch, int64_t length, const Geo &g) {
  Ws w;
  w.tb.win = a.take<float>((size_t)g.win);
  w.tb.g = a.take<float>((size_t)NB * GW);
  w.tb.j0 = a.take<int>(32);
  w.tb.tw = a.take<float>(1024);
  w.Fld = std::max<int64_t>(frames_of(length, g.win, g.hop), 1);
  w.fr.llr = a.take<float>((size_t)batch * (size_t)w.Fld);
  w.fr.wss = a.take<float>((size_t)batch * (size_t)w.Fld);
  w.fr.seg = a.take<float>((size_t)batch * (size_t)w.Fld);
  w.flags = a.take<int>((size_t)batch * (size_t)chunks(length, g));
  w.L16 = g.sr == 8000 ? 2 * length : length;
  w.ld16 = (w.L16 + 3) & ~(int64_t)3;
  w.up = nullptr;
  w.len16 = nullptr;
  if (g.sr == 8000) {
    w.up = a.take<float>((size_t)(2 * batch) * (size_t)w.ld16);
    w.len16 = a.take<int32_t>((size_t)batch);
  }
  w.pesq_bytes = layout_bytes(pesq::wb_layout, batch, w.L16);
  w.pesq = a.take<char>(w.pesq_bytes);
  return w;
}

}  // namespace composite
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_composite_chunk(int32_t sample_rate) {
  composite::Geo g;
  return composite::make_geo(sample_rate, &g) ? g.C : 0;
}

extern "C" size_t fsem_composite_workspace_bytes(int64_t batch, int64_t length, int32_t sample_rate) {
  composite::Geo g;
  if (!composite::make_geo(sample_rate, &g) || batch < 1 || length < 1 || length > kMaxLength) return 0;
  if (sample_rate == 8000 && 2 * length > kMaxLength) return 0;
  return layout_bytes(composite::layout, batch, length, g);
}

extern "C" int fsem_composite_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                  const int32_t *lengths, int32_t sample_rate, float *csig, float *cbak, float *covl,
                                  float *pesq_out, float *llr, float *wss, float *seg_snr, void *ws, size_t ws_bytes,
                                  void *stream) {
  if (!ref || !deg || !csig || !cbak || !covl || !pesq_out || !llr || !wss || !seg_snr || batch < 1 || length < 1 ||
      ld < length || length > kMaxLength)
    return FSEM_EINVAL;
  composite::Geo g;
  if (!composite::make_geo(sample_rate, &g)) return FSEM_ERATE;
  if (sample_rate == 8000 && 2 * length > kMaxLength) return FSEM_EINVAL;  // (the 16 kHz copy's length)
  Arena a(ws);
  const composite::Ws w = composite::layout(a, batch, length, g);
  if (!a.fits(ws_bytes)) return FSEM_EWORKSPACE;
  if (!lengths && pesq::frames_of(w.L16) < 20) return FSEM_ESHORT;  // as fsem_pesq_wb_f32, before any launch
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = (int)composite::chunks(length, g);
  const int ntab = std::max(g.win, composite::NB * composite::GW);  // (>= 512)
  hipLaunchKernelGGL(composite::composite_tables, dim3((unsigned)((ntab + 255) / 256)), dim3(256), 0, st, w.tb, g.win,
                     g.H, g.sr);
  FSEM_CHECK_LAUNCH();
  const size_t lds = composite::frames_lds(g);
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)nchunk, batch, r0);
    if (g.sr == 16000)
      hipLaunchKernelGGL((composite::composite_frames<16, true>), grid, dim3(composite::T), lds, st, ref, deg, ld,
                         lengths, (int)length, r0, w.tb, w.fr, w.Fld, w.flags, nchunk);
    else
      hipLaunchKernelGGL((composite::composite_frames<10, false>), grid, dim3(composite::T), lds, st, ref, deg, ld,
                         lengths, (int)length, r0, w.tb, w.fr, w.Fld, w.flags, nchunk);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(composite::composite_rows, grid_yz(3, batch), dim3(composite::RT), 0, st, w.fr, w.Fld, batch,
                     lengths, (int)length, g.hop, llr, wss, seg_snr);
  FSEM_CHECK_LAUNCH();
  // PESQ of the rows at 16 kHz
  const float *r16 = ref, *d16 = deg;
  int64_t ld16 = ld;
  const int32_t *l16 = lengths;
  if (g.sr == 8000) {
    float *ur = w.up, *ud = w.up + batch * w.ld16;
    int rc;
    if (lengths) {
      hipLaunchKernelGGL(composite::composite_len16, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, lengths,
                         (int)length, batch, w.len16);
      FSEM_CHECK_LAUNCH();
      rc = fsem_resample_rows_f32(ref, batch, length, ld, lengths, ur, w.ld16, 8000, 16000, stream);
      if (rc == FSEM_OK) rc = fsem_resample_rows_f32(deg, batch, length, ld, lengths, ud, w.ld16, 8000, 16000, stream);
      l16 = w.len16;
    } else {
      rc = fsem_resample_f32(ref, batch, length, ld, ur, w.ld16, 8000, 16000, stream);
      if (rc == FSEM_OK) rc = fsem_resample_f32(deg, batch, length, ld, ud, w.ld16, 8000, 16000, stream);
    }
    if (rc != FSEM_OK) return rc;
    r16 = ur, d16 = ud, ld16 = w.ld16;
  }
  const int rc = fsem_pesq_wb_f32(r16, d16, batch, w.L16, ld16, l16, pesq_out, w.pesq, w.pesq_bytes, stream);
  if (rc != FSEM_OK) return rc;
  hipLaunchKernelGGL(composite::composite_combine, dim3((unsigned)((batch + composite::CT - 1) / composite::CT)),
                     dim3(composite::CT), 0, st, w.flags, nchunk, lengths, (int)length, batch, (int)g.C, csig, cbak,
                     covl, pesq_out, llr, wss, seg_snr);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}
