// Energy-ratio metrics of (clean, denoised) rows: SI-SDR, SNR and segmental SNR (include/fsem.h,
// "SDR").  Replaces nothing in the reference.  One read of each input.
//
//   sdr_window   w2[t] = w[t]^2, w[t] = 0.5 (1 - cos(2 pi (t + 1) / (win + 1))) = sin^2(pi (t + 1) /
//                (win + 1)), evaluated in double once per call (win floats at the head of the
//                workspace); every chunk block copies it to LDS.
//   sdr_partial  grid (chunk, row).  A chunk is K hop blocks (K from the sample rate only, a
//                multiple of 16, about 7680 samples).  16 lanes share a hop block: lane k takes the
//                float4s k, k + 16, ... of the block, counted from the block's first sample rounded
//                down to a multiple of 4 (hop is not always a multiple of 4: elements of a float4
//                outside [block start, min(block end, n)) are replaced by zeros, and the neighbouring
//                block's lanes count them).  Per sample pair: the five energy sums and the two plain
//                sums in double (products of the float32 samples, exact in double), and the four
//                window-quarter sums Q(m, q) = sum_t w2[q hop + t] x^2[m hop + t] of s and of
//                d = s^ - s in float32 (the scheme of fsem_vad.h).  The 8 quarter sums are reduced
//                over the 16 lanes by a fixed halving exchange into LDS; frames wholly inside the
//                chunk (f .. f + 3 all in it) are evaluated there, the three frames that straddle
//                the chunk's end are left as a leading part here and a trailing part in the next
//                chunk's record.  One 128-byte record per (row, chunk); no atomics.
//   sdr_finish   one thread per row: the chunk records in ascending order, the straddling frames,
//                the three scores.
//
// Every sum has one order, fixed by the sample rate alone: a row's scores do not depend on the
// batch size, the row's position, the row capacity or the stream.
#include <algorithm>
#include <math.h>

#include "fsem_sdr_rules.h"

namespace fsem {
namespace sdr {

constexpr int T = 256;              // threads of a chunk block
constexpr int G = 16;               // lanes per hop block
constexpr int NG = T / G;           // hop blocks in flight per chunk block
constexpr int kChunkTarget = 7680;  // samples per chunk, about (rounded up to NG hop blocks)
constexpr int FT = 64;              // threads of a finish block

struct Geo {
  int hop, win, K;
  int64_t C;  // samples per chunk
};

inline bool make_geo(int32_t sr, Geo *g) {
  if (sr < 4000 || sr > 192000) return false;
  g->hop = (int)((int64_t)sr * 30 / 4000);
  g->win = 4 * g->hop;
  g->K = ((kChunkTarget + g->hop - 1) / g->hop + NG - 1) / NG * NG;  // <= 256 = T
  g->C = (int64_t)g->K * g->hop;
  return true;
}

// One (row, chunk) record.
struct Part {
  double e[6];       // sum s^2, s s^, s^^2, d^2, s, s^ over the chunk's samples
  double seg;        // sum of v_f over the frames wholly inside the chunk
  float tail[3][2];  // frame cK + K - 3 + j: its quarters in this chunk, {s, d}
  float head[3][2];  // frame cK - 3 + j: its quarters in this chunk, {s, d}
  double pad[3];
};
static_assert(sizeof(Part) == 128, "one record is 128 bytes");

inline int64_t chunks(int64_t length, const Geo &g) { return (length + g.C - 1) / g.C; }
inline size_t lds_bytes(const Geo &g) {
  return 4 * 7 * sizeof(double) + (size_t)g.K * 8 * sizeof(float) + (size_t)(g.win + 8) * sizeof(float);
}

__global__ void sdr_window(float *__restrict__ w2, int win) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= win) return;
  const double x = sin(3.14159265358979323846 * (double)(t + 1) / (double)(win + 1));
  const double w = x * x;
  w2[t] = (float)(w * w);
}

__device__ __forceinline__ float frame_db(float S, float D) {
  const float v = 10.f * log10f(S / (D + 1e-10f) + 1e-10f);
  return fminf(fmaxf(v, -10.f), 35.f);
}

template <bool VEC>
__global__ __launch_bounds__(T) void sdr_partial(const float *__restrict__ ref, const float *__restrict__ deg,
                                                 int64_t ld, const int32_t *__restrict__ lengths, int length,
                                                 int64_t r0, int hop, int K, const float *__restrict__ w2g,
                                                 Part *__restrict__ part, int nchunk) {
  extern __shared__ double smem[];
  double *red = smem;                                 // [4 waves][7]
  float *Q = reinterpret_cast<float *>(red + 4 * 7);  // [K][4 quarters][s, d]
  float *w2 = Q + K * 8;                              // 4 zeros, w2[0 .. win), 4 zeros
  const int tid = threadIdx.x;
  const int64_t row = r0 + blockIdx.y;
  const int c = blockIdx.x;
  const int n = row_length(lengths, row, length);
  const int win = 4 * hop;
  const int base = c * (K * hop);  // < length + C <= 2^29 + 2^15
  if (base >= n) return;           // (the finish pass reads ceil(n / C) records of this row)
  for (int i = tid; i < win + 8; i += T) w2[i] = (i >= 4 && i < win + 4) ? w2g[i - 4] : 0.f;
  __syncthreads();
  w2 += 4;
  const float *__restrict__ srow = ref + row * ld;
  const float *__restrict__ hrow = deg + row * ld;
  const int g = tid / G, k = tid % G;
  double ss = 0, sh = 0, hh = 0, dd = 0, s1 = 0, h1 = 0;
  for (int mb = g; mb < K; mb += NG) {
    const int P = base + mb * hop;  // the block's first sample
    const int hi = min(P + hop, n);
    float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int a = (P & ~3) + 4 * k; a < hi; a += 4 * G) {
      float sv[4], hv[4];
      if (VEC) {  // a % 4 == 0 and a < n: the float4 lies inside the row's ceil4(length) floats
        const float4 s4 = *reinterpret_cast<const float4 *>(srow + a);
        const float4 h4 = *reinterpret_cast<const float4 *>(hrow + a);
        sv[0] = s4.x, sv[1] = s4.y, sv[2] = s4.z, sv[3] = s4.w;
        hv[0] = h4.x, hv[1] = h4.y, hv[2] = h4.z, hv[3] = h4.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in = a + e >= P && a + e < hi;
          sv[e] = in ? srow[a + e] : 0.f;
          hv[e] = in ? hrow[a + e] : 0.f;
        }
      }
      const int t = a - P;  // -3 .. hop - 1
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = a + e >= P && a + e < hi;
        const float s = in ? sv[e] : 0.f, h = in ? hv[e] : 0.f;
        const double sd = s, hd = h, d = hd - sd;
        ss = fma(sd, sd, ss);
        sh = fma(sd, hd, sh);
        hh = fma(hd, hd, hh);
        dd = fma(d, d, dd);
        s1 += sd;
        h1 += hd;
        const float df = h - s, s2 = s * s, d2 = df * df;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float w = w2[r * hop + t + e];  // (inside the padded table for every t, e)
          q[2 * r] = fmaf(w, s2, q[2 * r]);
          q[2 * r + 1] = fmaf(w, d2, q[2 * r + 1]);
        }
      }
    }
    // the 8 sums over the block's 16 lanes: each step a lane gives away half of its values to the
    // lane 8, 4, 2 away and adds the halves it receives; then lanes k and k ^ 1 hold the same value
    float u[4], v2[2], v1;
    {
      const bool up = k & 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] = (up ? q[4 + i] : q[i]) + __shfl_xor(up ? q[i] : q[4 + i], 8, 64);
    }
    {
      const bool up = k & 4;
#pragma unroll
      for (int i = 0; i < 2; ++i) v2[i] = (up ? u[2 + i] : u[i]) + __shfl_xor(up ? u[i] : u[2 + i], 4, 64);
    }
    {
      const bool up = k & 2;
      v1 = (up ? v2[1] : v2[0]) + __shfl_xor(up ? v2[0] : v2[1], 2, 64);
    }
    v1 += __shfl_xor(v1, 1, 64);
    if (!(k & 1)) Q[mb * 8 + (k >> 1)] = v1;  // index ((k>>3)&1) * 4 + ((k>>2)&1) * 2 + ((k>>1)&1)
  }
  __syncthreads();
  // frames wholly inside the chunk: local blocks fl .. fl + 3 (K <= T: at most one per thread)
  double seg = 0;
  const int F = n >= win ? (n - win) / hop + 1 : 0;
  if (tid <= K - 4 && c * K + tid < F) {
    const float *q0 = Q + tid * 8;
    const float S = ((q0[0] + q0[8 + 2]) + q0[16 + 4]) + q0[24 + 6];
    const float D = ((q0[1] + q0[8 + 3]) + q0[16 + 5]) + q0[24 + 7];
    seg = frame_db(S, D);
  }
  double vals[7] = {ss, sh, hh, dd, s1, h1, seg};
#pragma unroll
  for (int i = 0; i < 7; ++i) vals[i] = wave_sum_d(vals[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) red[(tid >> 6) * 7 + i] = vals[i];
  }
  __syncthreads();
  Part *__restrict__ p = part + (row * nchunk + c);
  if (tid < 7) {
    const double v = ((red[tid] + red[7 + tid]) + red[14 + tid]) + red[21 + tid];
    if (tid < 6) p->e[tid] = v;
    else p->seg = v;
  } else if (tid >= 64 && tid < 64 + 6) {
    // frame cK + K - 3 + j: quarters 0 .. 2 - j are this chunk's blocks K - 3 + j ..
    const int j = (tid - 64) >> 1, x = (tid - 64) & 1;
    float a = 0.f;
    for (int r = 0; r <= 2 - j; ++r) a += Q[(K - 3 + j + r) * 8 + 2 * r + x];
    p->tail[j][x] = a;
  } else if (tid >= 128 && tid < 128 + 6) {
    // frame cK - 3 + j: quarters 3 - j .. 3 are this chunk's blocks 0 .. j
    const int j = (tid - 128) >> 1, x = (tid - 128) & 1;
    float a = 0.f;
    for (int r = 3 - j; r <= 3; ++r) a += Q[(r - 3 + j) * 8 + 2 * r + x];
    p->head[j][x] = a;
  }
}

__global__ __launch_bounds__(FT) void sdr_finish(const Part *__restrict__ part, int nchunk,
                                                 const int32_t *__restrict__ lengths, int length, int64_t B,
                                                 int hop, int K, int zero_mean, float *__restrict__ si_out,
                                                 float *__restrict__ snr_out, float *__restrict__ seg_out) {
  const int64_t b = (int64_t)blockIdx.x * FT + threadIdx.x;
  if (b >= B) return;
  const float nanf_ = __builtin_nanf("");
  const int n = row_length(lengths, b, length);
  if (n == 0) {
    si_out[b] = snr_out[b] = seg_out[b] = nanf_;
    return;
  }
  const int win = 4 * hop, C = K * hop;
  const int F = n >= win ? (n - win) / hop + 1 : 0;
  const int nc = (n + C - 1) / C;
  const Part *__restrict__ p = part + b * nchunk;
  double e[6] = {0, 0, 0, 0, 0, 0}, seg = 0;
  for (int c = 0; c < nc; ++c) {
#pragma unroll
    for (int i = 0; i < 6; ++i) e[i] += p[c].e[i];
    seg += p[c].seg;
    if (c + 1 < nc) {
      for (int j = 0; j < 3; ++j) {
        if (c * K + K - 3 + j < F)
          seg += frame_db(p[c].tail[j][0] + p[c + 1].head[j][0], p[c].tail[j][1] + p[c + 1].head[j][1]);
      }
    }
  }
  const double ss = e[0], sh = e[1], hh = e[2], dd = e[3];
  if (!isfinite(ss) || !isfinite(hh) || !isfinite(dd) || !isfinite(sh)) {  // a non-finite sample in the row
    si_out[b] = snr_out[b] = seg_out[b] = nanf_;
    return;
  }
  const PairScores sc = pair_scores(ss, hh, sh, dd, e[4], e[5], n, zero_mean);
  snr_out[b] = (float)sc.snr;
  seg_out[b] = F > 0 ? (float)(seg / F) : nanf_;
  si_out[b] = (float)sc.si;
}

// Workspace: the squared window, then one record per (row, chunk).
struct Ws {
  float *w2;
  Part *part;
};
inline Ws layout(Arena &a, int64_t batch, int64_t length, const Geo &g) {
  Ws w;
  w.w2 = a.take<float>((size_t)g.win);
  w.part = a.take<Part>((size_t)batch * (size_t)chunks(length, g));
  return w;
}

}  // namespace sdr
}  // namespace fsem

using namespace fsem;

extern "C" int64_t fsem_sdr_hop(int32_t sample_rate) {
  sdr::Geo g;
  return sdr::make_geo(sample_rate, &g) ? g.hop : 0;
}

extern "C" int64_t fsem_sdr_frames(int64_t length, int32_t sample_rate) {
  sdr::Geo g;
  if (!sdr::make_geo(sample_rate, &g) || length < g.win) return 0;
  return (length - g.win) / g.hop + 1;
}

extern "C" int64_t fsem_sdr_chunk(int32_t sample_rate) {
  sdr::Geo g;
  return sdr::make_geo(sample_rate, &g) ? g.C : 0;
}

extern "C" size_t fsem_sdr_workspace_bytes(int64_t batch, int64_t length, int32_t sample_rate) {
  sdr::Geo g;
  if (!sdr::make_geo(sample_rate, &g) || batch < 1 || length < 1 || length > kMaxLength) return 0;
  return layout_bytes(sdr::layout, batch, length, g);
}

extern "C" int fsem_sdr_f32(const float *ref, const float *deg, int64_t batch, int64_t length, int64_t ld,
                            const int32_t *lengths, int32_t sample_rate, int32_t zero_mean, float *si_sdr,
                            float *snr, float *seg_snr, void *ws, size_t ws_bytes, void *stream) {
  if (!ref || !deg || !si_sdr || !snr || !seg_snr || batch < 1 || length < 1 || ld < length || length > kMaxLength)
    return FSEM_EINVAL;
  sdr::Geo g;
  if (!sdr::make_geo(sample_rate, &g)) return FSEM_ERATE;
  Arena a(ws);
  const sdr::Ws w = sdr::layout(a, batch, length, g);
  if (!a.fits(ws_bytes)) return FSEM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = (int)sdr::chunks(length, g);
  hipLaunchKernelGGL(sdr::sdr_window, dim3((unsigned)((g.win + 255) / 256)), dim3(256), 0, st, w.w2, g.win);
  FSEM_CHECK_LAUNCH();
  // 16-byte loads where every row of both operands starts on a 16-byte boundary
  const bool vec = (((uintptr_t)ref | (uintptr_t)deg) & 15) == 0 && ld % 4 == 0;
  const size_t lds = sdr::lds_bytes(g);
  for (int64_t r0 = 0; r0 < batch; r0 += kMaxGridY) {
    const dim3 grid = grid_slice((unsigned)nchunk, batch, r0);
    if (vec)
      hipLaunchKernelGGL(sdr::sdr_partial<true>, grid, dim3(sdr::T), lds, st, ref, deg, ld, lengths, (int)length, r0,
                         g.hop, g.K, w.w2, w.part, nchunk);
    else
      hipLaunchKernelGGL(sdr::sdr_partial<false>, grid, dim3(sdr::T), lds, st, ref, deg, ld, lengths, (int)length, r0,
                         g.hop, g.K, w.w2, w.part, nchunk);
    FSEM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(sdr::sdr_finish, dim3((unsigned)((batch + sdr::FT - 1) / sdr::FT)), dim3(sdr::FT), 0, st, w.part,
                     nchunk, lengths, (int)length, batch, g.hop, g.K, zero_mean, si_sdr, snr, seg_snr);
  FSEM_CHECK_LAUNCH();
  return FSEM_OK;
}
