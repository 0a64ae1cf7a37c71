// score_keys.h — the 64-bit (value, index) sort keys and the LDS bitonic sort that the post-processing files (through
// post_nms.h) and center_decode.hip share.  "Value descending, lower index first" is the keys' plain descending order.
#pragma once
#include "spx_common.h"

namespace {

// float -> uint32 whose unsigned order is the float order (-0 counts as +0, as in a float comparison).  NOT the ord_f32
// of point_dist.h, which maps the raw bits and so keeps -0 below +0: do not unify the two.
__device__ __forceinline__ uint32_t ordered_bits(float s) {
  uint32_t u = __float_as_uint(s + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// key of row (or flat index) `row` >= 0: never 0, so 0 pads a sort and marks an empty place
__device__ __forceinline__ unsigned long long make_key(float score, int row) {
  return ((unsigned long long)ordered_bits(score) << 32) | (unsigned long long)(~(uint32_t)row);
}

__device__ __forceinline__ int row_of(unsigned long long key) { return (int)(~(uint32_t)key); }

// bitonic sort of keys[0, p), descending; p a power of two; called by the whole workgroup after a barrier
__device__ void sort_desc(unsigned long long* keys, int p) {
  for (int k = 2; k <= p; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < p; i += blockDim.x) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long a = keys[i], b = keys[x];
          const bool desc = (i & k) == 0;
          if (desc ? a < b : a > b) {
            keys[i] = b;
            keys[x] = a;
          }
        }
      }
      __syncthreads();
    }
}

}  // namespace
