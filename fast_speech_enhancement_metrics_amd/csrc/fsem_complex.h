// What the one-wave 512-point transforms share whatever their scalar type (fsem_fft.h's complex
// floats, lsd.hip's complex doubles): complex arithmetic on any struct C {r, i}, the 8-point
// butterfly, the exchange area's swizzle and the fetch of a mirror bin.  No tables: lsd.hip
// includes this header alone.
#pragma once
#include "fsem_common.h"

namespace fsem {

template <class C>
__device__ __forceinline__ C cadd(C a, C b) { return {a.r + b.r, a.i + b.i}; }
template <class C>
__device__ __forceinline__ C csub(C a, C b) { return {a.r - b.r, a.i - b.i}; }
template <class C>
__device__ __forceinline__ C cmul(C a, C b) {
  return {fma(a.r, b.r, -a.i * b.i), fma(a.r, b.i, a.i * b.r)};
}
template <class C>
__device__ __forceinline__ C mul_mi(C a) { return {a.i, -a.r}; }  // a * (-i)

// In-register forward DFT of 8 points (radix-2 DIT, W8 = exp(-i pi/4)).
template <class C>
__device__ __forceinline__ void dft8(C v[8]) {
  const decltype(v[0].r) h = 0.70710678118654752440;
  const C a0 = cadd(v[0], v[4]), a1 = csub(v[0], v[4]);
  const C a2 = cadd(v[2], v[6]), a3 = mul_mi(csub(v[2], v[6]));
  const C a4 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]);
  const C a6 = cadd(v[3], v[7]), a7 = mul_mi(csub(v[3], v[7]));
  const C b0 = cadd(a0, a2), b2 = csub(a0, a2), b1 = cadd(a1, a3), b3 = csub(a1, a3);
  const C c0 = cadd(a4, a6), c2 = csub(a4, a6), c1 = cadd(a5, a7), c3 = csub(a5, a7);
  const C w1c1 = {h * (c1.r + c1.i), h * (c1.i - c1.r)};   // c1 * (1 - i)/sqrt2
  const C w3c3 = {h * (c3.i - c3.r), -h * (c3.r + c3.i)};  // c3 * (-1 - i)/sqrt2
  const C mic2 = mul_mi(c2);
  v[0] = cadd(b0, c0);
  v[4] = csub(b0, c0);
  v[1] = cadd(b1, w1c1);
  v[5] = csub(b1, w1c1);
  v[2] = cadd(b2, mic2);
  v[6] = csub(b2, mic2);
  v[3] = cadd(b3, w3c3);
  v[7] = csub(b3, w3c3);
}

// Element i of a wave's 512-element exchange area is stored at fpad(i) = i ^ ((i >> 3) & 15).
// The XOR swizzle keeps all four access patterns bank-conflict-free under the gfx950 LDS
// lane-group rules (stage scatters 8*lane + r and o1 + 8r as ds_write_b64 in 16-lane groups,
// gathers lane + 64r as ds_read_b64 in 32-lane groups) without padding; the former i + i/8
// padding left 2-way conflicts on the gathers.
__device__ __forceinline__ int fpad(int i) { return i ^ ((i >> 3) & 15); }

// Two real frames in one complex 512-point transform (z = frame a + i frame b) are recovered from
// Z[k] and the mirror bin Z[512 - k].  With v[r] = Z[lane + 64 r] and k = lane + 64 r, r < 4, the
// mirror lies in lane plane = (64 - lane) & 63 of register 7 - r; lane 0 holds it itself, in
// register 8 - r (k = 0: Z[0]).
template <class C>
__device__ __forceinline__ C mirror_bin(const C v[8], int r, int lane, int plane) {
  auto mr = __shfl(v[7 - r].r, plane, 64);
  auto mi = __shfl(v[7 - r].i, plane, 64);
  if (lane == 0) {
    mr = v[(8 - r) & 7].r;
    mi = v[(8 - r) & 7].i;
  }
  return {mr, mi};
}

}  // namespace fsem
