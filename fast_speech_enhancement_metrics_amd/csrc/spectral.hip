// Spectral measures of (clean, denoised) rows from Hu & Loizou's evaluation set: the
// frequency-weighted segmental SNR (fwSegSNR), the LPC cepstral distance (CD) and the
// Itakura-Saito distance (IS) (include/fsem.h "Spectral").  Replaces nothing in the reference.
// Composite's frames, window, LPC orders and band filters, through the code the two share: the
// frame geometry, the spectra's split step and the band sums (fsem_speech_frames.h), the radix
// select (fsem_select.h) and the wave's double sums (fsem_common.h); the LPC recursion and the
// quadratic form are fsem_lpc.h's.  The tables here are constants (fsem_tables.inc), Composite's
// its own.
//
//   spectral_frames  grid (group, row), 4 waves.  A group is KF = 32 frames: its (KF + 3) hop
//                    samples of both rows are staged in LDS once (frames overlap by 75 %).
//                      - Autocorrelation R[0..P] in double, ONE LANE PER (frame, signal, window
//                        quarter): a wave takes 8 frames; a lane runs over its hop samples with
//                        the next 20 windowed samples (float32 products w[t] x[t]) in registers,
//                        every lag one chain of FMAs in sample order -- no wave-wide reduction;
//                        the four quarters are added by two quad exchanges, R goes to LDS.
//                      - Then, frame by frame (a wave takes every fourth frame of the group): the
//                        windowed frames to the wave's FFT exchange area; both spectra with
//                        fft512_wave_x2 (16 kHz: the 1024-point real transform as a 512-point
//                        complex one plus the split step; 8 kHz: a zero imaginary part; clean and
//                        denoised never share a transform), magnitudes, their sum, the normalised
//                        magnitudes to LDS; the 25 band sums (one lane per signal and band,
//                        float32, sparse table), then the weights, log ratios and the weighted
//                        mean in double: fwSegSNR_f.
//                      - Then wave 0 alone, ONE LANE PER (frame, signal) -- 32 frames x 2 signals:
//                        Levinson-Durbin, the cepstrum of 1 / A(z) and the two quadratic forms in
//                        double (R read from LDS where it is used), a lane and its neighbour (the
//                        frame's other signal) exchanging the cepstra and E: CD_f and IS_f.  One
//                        recursion serves 32 frames.
//   spectral_rows    one block per row: scans the row's n samples of both signals for a
//                    non-finite one (the entry has no flag workspace), then CD and IS as the mean
//                    of the K smallest frame values (radix select over the floats' ordered bit
//                    patterns, four 256-bin histogram passes with integer counts) and fwSegSNR as
//                    the mean of all F; thread t sums its values t, t + 256, ... in order in
//                    double, the 256 sums are added in a fixed halving tree.
//
// The frame values are the caller's `frames` output; there is no workspace and no hidden
// allocation.  Every sum has one order, fixed by the sample rate alone.
#include <algorithm>
#include <math.h>

#include "fsem_lpc.h"
#include "fsem_select.h"
#include "fsem_speech_frames.h"

namespace fsem {
namespace spectral {

constexpr int T = 256;  // threads of a frame block
constexpr int NWAVE = T / 64;
constexpr int KF = 32;  // frames per block: the Levinson lane group (32 frames x 2 signals = 64 lanes)
constexpr int NB = 25;  // critical bands
constexpr int GW = FSEM_SPEC_GW;
constexpr int RT = 256;  // threads of a row block

template <int P, bool WIDE>
__global__ __launch_bounds__(T) void spectral_frames(const float *__restrict__ ref, const float *__restrict__ deg,
                                                     int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                     int64_t r0, int64_t batch, float *__restrict__ frames,
                                                     int64_t ldf) {
  constexpr int hop = frame_hop(WIDE ? 16000 : 8000), win = 4 * hop, H = WIDE ? 512 : 256;
  constexpr int S = (KF + 3) * hop;   // samples a group's frames cover
  constexpr int NK = (win + 63) / 64;  // window samples per lane
  constexpr int NR = WIDE ? 8 : 4;     // spectrum bins per lane
  constexpr int RING = 20;             // samples a lane keeps ahead in registers (> P, divides hop)
  static_assert(2 * win * 4 <= kFftBuf * 8, "the windowed frames live in the wave's FFT exchange area");
  static_assert(RING > P && hop % RING == 0 && KF == 8 * NWAVE, "autocorrelation lane layout");
  __shared__ __attribute__((aligned(16))) float2 fbuf[NWAVE * kFftBuf];
  __shared__ float xs[S], xd[S];  // the group's samples of both rows
  __shared__ float wl[win];
  __shared__ float gt[NB * GW];
  __shared__ int gj0[32];
  __shared__ double Rb[KF * 2 * (P + 1)];  // [frame][signal][lag]
  __shared__ float eb[NWAVE * 64];         // [wave][signal][32] band sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = r0 + blockIdx.y;
  const int n = row_length(lengths, row, length);
  const int F = frames_of(n, win, hop);
  const int f0 = blockIdx.x * KF;
  if (f0 >= F) return;  // (block-uniform, before any barrier)
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  for (int i = tid; i < S; i += T) {
    const int gidx = f0 * hop + i;
    xs[i] = gidx < n ? srow[gidx] : 0.f;
    xd[i] = gidx < n ? hrow[gidx] : 0.f;
  }
  for (int i = tid; i < win; i += T) wl[i] = WIDE ? kSpecWin16k[i] : kSpecWin8k[i];
  const float *__restrict__ gsrc = WIDE ? kSpecG16k[0] : kSpecG8k[0];
  for (int i = tid; i < NB * GW; i += T) gt[i] = gsrc[i];
  if (tid < NB) gj0[tid] = WIDE ? kSpecJ016k[tid] : kSpecJ08k[tid];
  float wt[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int t = lane + 64 * k;
    wt[k] = t < win ? (WIDE ? kSpecWin16k[t] : kSpecWin8k[t]) : 0.f;
  }
  __syncthreads();
  // Autocorrelations of this wave's 8 frames, one lane per (frame, signal, window quarter): the
  // lane's hop samples against their P successors, RING windowed samples ahead in registers
  // (w[t] x[t] as float32, the products the transforms read), every lag one chain of double FMAs
  // in sample order; the four quarters added as (q0 + q1) + (q2 + q3).
  {
    const int fl = wave + NWAVE * (lane >> 3), sg = (lane >> 2) & 1, q = lane & 3;
    const float *__restrict__ x = (sg ? xd : xs) + fl * hop;
    const int t0 = q * hop;
    auto sample = [&](int t) -> double { return t < win ? (double)(wl[t] * x[t]) : 0.0; };
    double b[RING], acc[P + 1];
#pragma unroll
    for (int j = 0; j < RING; ++j) b[j] = sample(t0 + j);
#pragma unroll
    for (int k = 0; k <= P; ++k) acc[k] = 0.0;
    for (int u = 0; u < hop; u += RING) {
#pragma unroll
      for (int j = 0; j < RING; ++j) {
        const double cur = b[j];
#pragma unroll
        for (int k = 0; k <= P; ++k) acc[k] = fma(cur, b[(j + k) % RING], acc[k]);
        b[j] = sample(t0 + u + j + RING);
      }
    }
#pragma unroll
    for (int k = 0; k <= P; ++k) acc[k] += dpp_mov_d<0xB1>(acc[k]);  // quad_perm [1,0,3,2]
#pragma unroll
    for (int k = 0; k <= P; ++k) acc[k] += dpp_mov_d<0x4E>(acc[k]);  // quad_perm [2,3,0,1]
    if (q == 0) {
      double *__restrict__ dst = Rb + (fl * 2 + sg) * (P + 1);
#pragma unroll
      for (int k = 0; k <= P; ++k) dst[k] = acc[k];
    }
  }
  float2 *buf = fbuf + wave * kFftBuf;
  float *fws = reinterpret_cast<float *>(buf), *fwd = fws + win;  // windowed frames, before the transforms
  float *pw = reinterpret_cast<float *>(buf);                    // [2][512] normalised magnitudes, after them
  float *e = eb + wave * 64;
  cf tw1[8], tw2[8];
  fft512_twiddles(lane, tw1, tw2);
  float wc[8], wsn[8];  // W_1024^j = wc - i wsn, j = lane + 64 r
  if (WIDE) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      wc[r] = kSpecTw[lane + 64 * r][0];
      wsn[r] = kSpecTw[lane + 64 * r][1];
    }
  }
  const int plane = (64 - lane) & 63;
  for (int fl = wave; fl < KF; fl += NWAVE) {
    const int f = f0 + fl;
    if (f >= F) break;  // (wave-uniform; the barrier below is outside the loop)
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int t = lane + 64 * k;
      if (t < win) {
        fws[t] = wt[k] * xs[fl * hop + t];
        fwd[t] = wt[k] * xd[fl * hop + t];
      }
    }
    wave_lds_fence();
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
    wave_lds_fence();  // the transforms overwrite the windowed frames
    fft512_wave_x2(va, vb, buf, lane, tw1, tw2);
    float ma[NR], mb[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (WIDE) {
        cf am, bm;
        split_mirrors(va, vb, r, lane, plane, am, bm);
        const cf xa = split_bin(va[r], am, wc[r], wsn[r]);
        ma[r] = sqrtf(xa.r * xa.r + xa.i * xa.i);
        const cf xb = split_bin(vb[r], bm, wc[r], wsn[r]);
        mb[r] = sqrtf(xb.r * xb.r + xb.i * xb.i);
      } else {
        ma[r] = sqrtf(va[r].r * va[r].r + va[r].i * va[r].i);
        mb[r] = sqrtf(vb[r].r * vb[r].r + vb[r].i * vb[r].i);
      }
    }
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      sa += ma[r];
      sb += mb[r];
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int j = lane + 64 * r;
      pw[j] = sa > 0.f ? ma[r] / sa : 0.f;
      pw[512 + j] = sb > 0.f ? mb[r] / sb : 0.f;
    }
    wave_lds_fence();
    // band sums: lanes 0 .. 24 the clean frame's, lanes 32 .. 56 the denoised frame's
    {
      const int sig = lane >> 5, i = lane & 31;
      if (i < NB) e[sig * 32 + i] = band_sum<GW>(pw + sig * 512, gt + i * GW, gj0[i], H);
    }
    wave_lds_fence();
    double nd[2] = {0.0, 0.0};
    if (lane < NB) {
      const double es = (double)e[lane], ed = (double)e[32 + lane];
      const double d = es - ed;
      const double err = fmax(d * d, 0x1p-52);
      const double W = pow(es, 0.2);
      if (W > 0.0) {
        nd[0] = W * (10.0 * log10(es * es / err));
        nd[1] = W;
      }
    }
    wave_sums_d<2>(nd);
    if (lane == 0) {
      const double v = nd[0] / nd[1];
      frames[row * ldf + f] = nd[1] > 0.0 ? (float)fmin(fmax(v, -10.0), 35.0) : __builtin_nanf("");
    }
    wave_lds_fence();  // the next frame overwrites the wave's buffers
  }
  __syncthreads();
  if (wave != 0) return;
  // one lane per (frame, signal): even lanes the clean frame, odd lanes the denoised one
  const int fl = lane >> 1, sig = lane & 1, f = f0 + fl;
  const bool live = f < F;  // (frames past F: R of zero-padded samples, the arithmetic is discarded)
  // (R stays in LDS: the recursion reads each lag where it uses it)
  const double *__restrict__ Rs = Rb + fl * 2 * (P + 1);
  const double *__restrict__ R = Rs + sig * (P + 1);
  double a[P + 1], c[P + 1];
  levinson<P>(R, a);
  // cepstrum of 1 / A(z)
  c[0] = 0.0;
#pragma unroll
  for (int m = 1; m <= P; ++m) {
    double acc = 0.0;
#pragma unroll
    for (int k = 1; k < m; ++k) acc = fma((double)k * c[k], a[m - k], acc);
    c[m] = -a[m] - acc / (double)m;
  }
  double dsum = 0.0;
#pragma unroll
  for (int m = 1; m <= P; ++m) {
    const double d = c[m] - __shfl_xor(c[m], 1, 64);
    dsum = fma(d, d, dsum);
  }
  double cd = (10.0 / 2.302585092994045684) * sqrt(2.0 * dsum);
  cd = cd > 10.0 ? 10.0 : cd;  // (NaN stays NaN)
  const double Eown = quadratic<P>(a, R);     // E_x = A_x T_x A_x'
  const double cross = quadratic<P>(a, Rs);   // odd lanes: A_s^ T_s A_s^'
  const double Es = __shfl(Eown, lane & ~1, 64);
  double is = cross / Eown + log(Eown / Es) - 1.0;
  is = is > 100.0 ? 100.0 : is;
  if (live) frames[((sig ? 2 : 1) * batch + row) * ldf + f] = sig ? (float)is : (float)cd;
}

static_assert(RT == 256, "select_kth is a 256-thread block's");
struct RowLds {
  SelectLds sel;
  double red[RT];
};

// The mean of the K smallest of v[0 .. F) (trimmed) or of all F, by the whole block.
__device__ float row_mean(const float *__restrict__ v, int F, bool trimmed, RowLds &s) {
  const int tid = threadIdx.x;
  const int K = trimmed ? (int)((19 * (int64_t)F + 10) / 20) : F;
  uint32_t kth = 0xFFFFFFFFu;  // the K-th smallest key
  int need = 0;                // copies of it among the K smallest
  if (trimmed) kth = select_kth(v, F, K, s.sel, &need);
  double acc = 0.0;
  for (int i = tid; i < F; i += RT) {
    const float x = v[i];
    if (!trimmed || order_key(x) < kth) acc += (double)x;
  }
  s.red[tid] = acc;
  __syncthreads();
  for (int h = RT / 2; h > 0; h >>= 1) {
    if (tid < h) s.red[tid] += s.red[tid + h];
    __syncthreads();
  }
  double total = s.red[0];
  __syncthreads();  // (the next call rewrites red)
  if (trimmed) total += (double)need * (double)key_value(kth);
  return (float)(total / (double)K);
}

__global__ __launch_bounds__(RT) void spectral_rows(const float *__restrict__ ref, const float *__restrict__ deg,
                                                    int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                    int64_t batch, int hop, const float *__restrict__ frames,
                                                    int64_t ldf, float *__restrict__ fw, float *__restrict__ cd,
                                                    float *__restrict__ is) {
  __shared__ RowLds s;
  const int tid = threadIdx.x;
  const int64_t row = grid_row_xy();
  if (row >= batch) return;
  const int n = row_length(lengths, row, length);
  const int win = 4 * hop;
  const int F = frames_of(n, win, hop);
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  int bad = 0;
  if (F > 0)  // (a row without a frame is NaN whatever it holds)
    for (int i = tid; i < n; i += RT) bad |= !(isfinite(srow[i]) && isfinite(hrow[i]));
  bad = __syncthreads_or(bad);
  if (F == 0 || bad) {  // (block-uniform)
    if (tid == 0) fw[row] = cd[row] = is[row] = __builtin_nanf("");
    return;
  }
  const float a = row_mean(frames + row * ldf, F, false, s);
  const float b = row_mean(frames + (batch + row) * ldf, F, true, s);
  const float c = row_mean(frames + (2 * batch + row) * ldf, F, true, s);
  if (tid == 0) {
    fw[row] = a;
    cd[row] = b;
    is[row] = c;
  }
}

}  // namespace spectral
}  // namespace fsem

using namespace fsem;

extern "C" int fsem_spectral_order(int32_t sample_rate) {
  FrameGeo g;
  return make_frame_geo(sample_rate, &g) ? g.P : 0;
}

extern "C" int fsem_spectral_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                                 const int32_t *lengths, int32_t sample_rate, float *frames, int64_t ldf,
                                 float *fwsegsnr, float *cd, float *is_, void *stream) {
  if (!ref || !deg || !frames || !fwsegsnr || !cd || !is_ || batch < 0 || length < 0 || ld < length ||
      length > kMaxLength)
    return FSEM_EINVAL;
  FrameGeo g;
  if (!make_frame_geo(sample_rate, &g)) return FSEM_ERATE;
  const int64_t F = frames_of(length, g.win, g.hop);
  if (ldf < std::max<int64_t>(F, 1)) return FSEM_EINVAL;
  if (batch == 0) return FSEM_OK;  // (nothing to score)
  hipStream_t st = (hipStream_t)stream;
  const int64_t ngroup = (F + spectral::KF - 1) / spectral::KF;
  for (int64_t r0 = 0; ngroup > 0 && r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)ngroup, batch, r0);
    if (g.sr == 16000)
      hipLaunchKernelGGL((spectral::spectral_frames<16, true>), grid, dim3(spectral::T), 0, st, ref, deg, ld, lengths,
                         (int)length, r0, batch, frames, ldf);
    else
      hipLaunchKernelGGL((spectral::spectral_frames<10, false>), grid, dim3(spectral::T), 0, st, ref, deg, ld,
                         lengths, (int)length, r0, batch, frames, ldf);
    FSEM_CHECK_LAUNCH();
  }
  // (length == 0, or no row with a frame: the row kernel alone, which writes the NaN scores)
  hipLaunchKernelGGL(spectral::spectral_rows, grid_xy(batch), dim3(spectral::RT), 0, st, ref, deg, ld, lengths,
                     (int)length, batch, g.hop, frames, ldf, fwsegsnr, cd, is_);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}
