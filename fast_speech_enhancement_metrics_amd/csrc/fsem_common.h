// Shared helpers of libfsem (gfx950 / CDNA4).  Wave size is 64 everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fsem.h"

#define FSEM_WAVE 64

#define FSEM_CHECK_LAUNCH()                                    \
  do {                                                         \
    if (hipGetLastError() != hipSuccess) return FSEM_ELAUNCH;  \
  } while (0)

namespace fsem {

// Workgroup barrier that orders LDS only.  __syncthreads() also waits for every outstanding
// global load/store (vmcnt(0)), which would drain the next tile's prefetch at every barrier;
// kernels that communicate through LDS alone use this instead.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// A wave-uniform 64-bit value (e.g. read from LDS) moved to scalar registers.
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Sum over a 256-thread block (4 waves).  `scratch` >= 4 floats of LDS.  All threads get it.
__device__ __forceinline__ float block_sum_256(float v, float *scratch) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  lds_barrier();
  if (lane == 0) scratch[w] = v;
  lds_barrier();
  return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

__device__ __forceinline__ double block_sum_256_d(double v, double *scratch) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[w] = v;
  __syncthreads();
  return scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

__device__ __forceinline__ float block_max_256(float v, float *scratch) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[w] = v;
  __syncthreads();
  return fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
}

// Compiler barrier for intra-wave LDS exchange (LDS ops of one wave complete in order).
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wait for this wave's outstanding LDS stores (before other waves read the data).
__device__ __forceinline__ void lds_stores_done() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One DPP move of a 32-bit value under control CTRL (all rows and banks, no bound control).
template <int CTRL, class T>
__device__ __forceinline__ T dpp_mov(T v) {
  static_assert(sizeof(T) == 4, "DPP moves one 32-bit register");
  return __builtin_bit_cast(T, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// One DPP move of a double (two 32-bit moves).
template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = dpp_mov<CTRL>((uint32_t)b), hi = dpp_mov<CTRL>((uint32_t)(b >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// The wave's sums of N values at once, the same bits in every lane: pairwise exchanges only (a
// lane and its partner add the same two numbers), inside a row of 16 lanes by DPP (quad
// permutes, then the mirrors of 8 and 16 lanes), across rows by two xor exchanges; step by step
// over all N so that the independent exchanges overlap.  (Another order than wave_sum_d's.)
template <int N>
__device__ __forceinline__ void wave_sums_d(double v[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov_d<0xB1>(v[i]);  // quad_perm [1,0,3,2]
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov_d<0x4E>(v[i]);  // quad_perm [2,3,0,1]
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov_d<0x141>(v[i]);  // row_half_mirror
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_mov_d<0x140>(v[i]);  // row_mirror
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], 16, 64);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], 32, 64);
}

// Row length of utterance b: the per-row length when given (clamped to [0, L]), else L; in L's
// type (int64_t, or int where the kernel's row arithmetic is 32-bit).
template <class Len>
__device__ __forceinline__ Len row_length(const int32_t *__restrict__ lens, int64_t b, Len L) {
  if (!lens) return L;
  const Len n = lens[b];
  return n < 0 ? 0 : (n > L ? L : n);
}

// A wave-uniform buffer descriptor over the nbytes bytes at p: raw buffer loads through it are
// range checked by the hardware, a load past the end returns 0 without a branch.  The words go
// through readfirstlane so that the descriptor sits in scalar registers (as uint32_t:
// readfirstlane returns int, which would sign-extend into the high word).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const void *p, uint32_t nbytes) {
  const uint64_t base = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
  void *q = reinterpret_cast<void *>(((uint64_t)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane(nbytes), 0x00020000);
}
// The float at byte offset voff + soff (soff wave-uniform) behind such a descriptor.
__device__ __forceinline__ float buffer_f32(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff = 0) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, 0));
}

// Four consecutive samples of a row from sample a (a % 4 == 0), zeros from sample `hi` on.  VEC:
// the row is 16-byte aligned, so four samples below hi are one float4.
template <bool VEC>
__device__ __forceinline__ void load4(const float *__restrict__ row, int a, int hi, float v[4]) {
  if (VEC && a + 4 <= hi) {
    const float4 x = *reinterpret_cast<const float4 *>(row + a);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a + j < hi ? row[a + j] : 0.f;
  }
}

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// A workspace as a sequence of 256-byte aligned regions.  Each entry has one layout function
// that takes its regions from an Arena in order: run on Arena(nullptr) it measures (bytes() is
// the entry's *_workspace_bytes), run on Arena(ws) it yields the pointers, so the size and the
// pointers cannot disagree.
class Arena {
 public:
  explicit Arena(void *base) : base_(static_cast<char *>(base)) {}
  template <class T>
  T *take(size_t count) {
    T *p = base_ ? reinterpret_cast<T *>(base_ + used_) : nullptr;
    used_ += align_up(count * sizeof(T), 256);
    return p;
  }
  size_t bytes() const { return used_; }
  // the regions taken so far lie within a workspace of ws_bytes at a non-null base
  bool fits(size_t ws_bytes) const { return base_ && used_ <= ws_bytes; }

 private:
  char *base_;
  size_t used_ = 0;
};

// The bytes a layout function takes: what the entry's *_workspace_bytes reports.
template <class Layout, class... Args>
size_t layout_bytes(Layout layout, const Args &...args) {
  Arena a(nullptr);
  layout(a, args...);
  return a.bytes();
}

// Longest row any entry accepts (input samples, and 10 / 16 kHz samples after resampling): the
// kernels address a row with 32-bit byte offsets (raw buffer loads, range-checked descriptors).
// 2^29 samples = 9.3 h at 16 kHz; longer rows give FSEM_EINVAL (include/fsem.h).
constexpr int64_t kMaxLength = int64_t(1) << 29;

// Launches that map rows (utterances) to grid.y cover at most kMaxGridY rows each; the host loops
// over slices [r0, r0 + kMaxGridY) and passes r0 (HIP's grid.y limit, hipDeviceProp maxGridSize[1]).
constexpr int64_t kMaxGridY = 65535;
inline dim3 grid_slice(unsigned x, int64_t rows, int64_t r0) {
  return dim3(x, (unsigned)(rows - r0 < kMaxGridY ? rows - r0 : kMaxGridY));
}

// Launches that instead fold `rows` over two grid dimensions of at most kMaxGridY each (no host
// loop): grid_ab spreads them over dimensions a and b, the kernel reads its row with grid_row_ab
// and returns when it is past the last.  The third dimension is the caller's.
inline unsigned grid_lo(int64_t rows) { return (unsigned)(rows < kMaxGridY ? rows : kMaxGridY); }
inline unsigned grid_hi(int64_t rows) { return (unsigned)((rows + kMaxGridY - 1) / kMaxGridY); }
inline dim3 grid_xy(int64_t rows) { return dim3(grid_lo(rows), grid_hi(rows)); }
inline dim3 grid_yz(unsigned x, int64_t rows) { return dim3(x, grid_lo(rows), grid_hi(rows)); }
inline dim3 grid_xz(int64_t rows, unsigned y) { return dim3(grid_lo(rows), y, grid_hi(rows)); }
__device__ __forceinline__ int64_t grid_row_xy() { return blockIdx.x + (int64_t)blockIdx.y * kMaxGridY; }
__device__ __forceinline__ int64_t grid_row_yz() { return blockIdx.y + (int64_t)blockIdx.z * kMaxGridY; }
__device__ __forceinline__ int64_t grid_row_xz() { return blockIdx.x + (int64_t)blockIdx.z * kMaxGridY; }

}  // namespace fsem
