// Hu & Loizou's analysis frames as composite.hip and spectral.hip take them: 30 ms windows every
// 7.5 ms, LPC order 10 / 16 at 8 / 16 kHz, and per frame pair the spectra by fft512_wave_x2 (at
// 16 kHz with the split step below) and band sums over a sparse table.  The tables stay with their
// users (Composite computes its own into its workspace, Spectral reads fsem_tables.inc): the
// helpers take pointers and twiddles.  The load of a frame pair into the transforms' registers
// stays written out in both kernels: as a function (whole, per point, by value or by reference) it
// made the vectoriser pack the transforms' first butterflies differently.
#pragma once
#include "fsem_fft.h"

namespace fsem {

constexpr int frame_hop(int sr) { return sr * 30 / 4000; }

struct FrameGeo {
  int sr, hop, win, P;
};

inline bool make_frame_geo(int32_t sr, FrameGeo *g) {
  if (sr != 8000 && sr != 16000) return false;
  g->sr = sr;
  g->hop = frame_hop(sr);
  g->win = 4 * g->hop;
  g->P = sr == 8000 ? 10 : 16;
  return true;
}

// Frames of a row of n samples (in n's type: the kernels' row arithmetic is 32-bit).
template <class Len>
__host__ __device__ inline Len frames_of(Len n, int win, int hop) {
  return n >= win ? (n - win) / hop + 1 : 0;
}

// The split step of the 1024-point real transform held as a 512-point complex one, v[r] =
// Z[lane + 64 r], at bin j = lane + 64 r: X[j] = E + W^j O with E = (Z[j] + conj Z[512 - j]) / 2,
// O = (Z[j] - conj Z[512 - j]) / (2 i), W_1024^j = wc - i wsn.
//
// split_mirrors: the mirror bins Z[512 - j] of both transforms of a frame pair, which lie in lane
// plane = (64 - lane) & 63 of register 7 - r (lane 0: its own register 8 - r; bin 0 takes Z[0]).
// The pair goes together, four exchanges and one lane-0 branch, because the kernels' code
// generation depends on it: the vectoriser packs the two signals' arithmetic into two-float
// instructions only when they share the block.
__device__ __forceinline__ void split_mirrors(const cf va[8], const cf vb[8], int r, int lane, int plane, cf &am,
                                              cf &bm) {
  float amr = __shfl(va[7 - r].r, plane, 64), ami = __shfl(va[7 - r].i, plane, 64);
  float bmr = __shfl(vb[7 - r].r, plane, 64), bmi = __shfl(vb[7 - r].i, plane, 64);
  if (lane == 0) {
    amr = va[(8 - r) & 7].r, ami = va[(8 - r) & 7].i;
    bmr = vb[(8 - r) & 7].r, bmi = vb[(8 - r) & 7].i;
  }
  am = {amr, ami};
  bm = {bmr, bmi};
}
// split_bin: X[j] of one signal from z = Z[j] and its mirror m.
__device__ __forceinline__ cf split_bin(cf z, cf m, float wc, float wsn) {
  const float er = 0.5f * (z.r + m.r), ei = 0.5f * (z.i - m.i);
  const float orr = 0.5f * (z.i + m.i), oi = -0.5f * (z.r - m.r);
  return {er + (wc * orr + wsn * oi), ei + (wc * oi - wsn * orr)};
}

// sum_q p[j0 + q] g[q] over one band's row of the sparse table, the bins inside [0, H) in
// ascending order, float32.
template <int GW>
__device__ __forceinline__ float band_sum(const float *p, const float *g, int j0, int H) {
  float acc = 0.f;
#pragma unroll
  for (int qq = 0; qq < GW; ++qq) {
    const int j = j0 + qq;
    if (j >= 0 && j < H) acc = fmaf(p[j], g[qq], acc);
  }
  return acc;
}

}  // namespace fsem
