// block_ops.h — the wave / workgroup reductions and the scan that several ops of libspx share (gfx950: wave = 64; the
// block forms are for workgroups of exactly 256 threads = 4 waves).  Every sum here has ONE fixed order, so a result does
// not depend on which file calls it.  A helper with another order or block size stays in its own file.
#pragma once
#include "spx_common.h"

// butterfly sum over the wave: every lane gets the total
template <typename T>
__device__ __forceinline__ T spx_wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, SPX_WAVE);
  return v;
}

// the block's sum: a shuffle-down tree per wave, then the four wave sums added in wave order; thread 0 gets it, every
// other thread 0.  sm: 4 elements of LDS, free on return.
template <typename T>
__device__ __forceinline__ T spx_block_sum(T v, T* sm) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
  if (threadIdx.x == 0) t = sm[0] + sm[1] + sm[2] + sm[3];
  __syncthreads();
  return t;
}

// the same sum in every thread
template <typename T>
__device__ __forceinline__ T spx_block_sum_all(T v, T* sm) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  const T t = sm[0] + sm[1] + sm[2] + sm[3];
  __syncthreads();
  return t;
}

// exclusive scan over the 256 threads of a block: wave-level inclusive scan by shuffles, then the waves are combined
// through wsum (4 words of LDS).  total, if given, receives the block's sum in every thread.
__device__ __forceinline__ uint32_t spx_block_excl_scan(uint32_t v, uint32_t* total, uint32_t* wsum) {
  const int lane = spx_lane(), wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  if (total) *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return base + inc - v;
}

// the same with the function's own 4 words of LDS
__device__ __forceinline__ uint32_t spx_block_excl_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wsum[4];
  return spx_block_excl_scan(v, total, wsum);
}

// out[q] = sum over k in [0, nblk) of part[k][q], part [nblk, nq]: one block of 256 threads per q, thread t adds rows
// t, t + 256, ... in ascending order, then a fixed LDS tree.  Launch with grid nq, block 256.
template <typename T>
static __global__ __launch_bounds__(256) void spx_k_column_sum(const T* __restrict__ part, int64_t nblk, int nq,
                                                               T* __restrict__ out) {
  __shared__ T s_v[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  T v = 0;
  for (int64_t k = tid; k < nblk; k += 256) v += part[(size_t)k * nq + q];
  s_v[tid] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) s_v[tid] += s_v[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[q] = s_v[0];
}
