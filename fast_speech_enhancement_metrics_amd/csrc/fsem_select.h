// The K-th smallest of a row's frame values by a radix select over the floats' ordered bit
// patterns (composite.hip, spectral.hip): four 256-bin histogram passes with integer counts, so
// any F and no summation order.  The sums over the selected values stay with their kernels.
#pragma once
#include "fsem_common.h"

namespace fsem {

// The float's bits as an unsigned key in the floats' order, every NaN after +inf.
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  if (v != v) return 0xFFFFFFFFu;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);  // (0xFFFFFFFF: a NaN)
}

struct SelectLds {
  int hist[256];
  uint32_t prefix;
  int need;
};

// The K-th smallest key of v[0 .. F), 1 <= K <= F, by a whole block of 256 threads (every thread
// calls it and gets it); *need: the copies of that key among the K smallest.
__device__ __forceinline__ uint32_t select_kth(const float *__restrict__ v, int F, int K, SelectLds &s, int *need) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  int left = K;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t mask = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;
    s.hist[tid] = 0;  // (256 threads, 256 bins)
    __syncthreads();
    for (int i = tid; i < F; i += 256) {
      const uint32_t k = order_key(v[i]);
      if ((k & mask) == prefix) atomicAdd(&s.hist[(k >> shift) & 255], 1);  // integer counts: no order
    }
    __syncthreads();
    if (tid == 0) {
      int cum = 0, b = 0;
      for (; b < 255; ++b) {
        if (cum + s.hist[b] >= left) break;
        cum += s.hist[b];
      }
      s.prefix = prefix | ((uint32_t)b << shift);
      s.need = left - cum;
    }
    __syncthreads();
    prefix = s.prefix;
    left = s.need;
    __syncthreads();
  }
  *need = left;
  return prefix;
}

}  // namespace fsem
