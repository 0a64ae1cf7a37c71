// point_dist.h — the squared distance and the order-preserving float key that pointnet2.hip (§11) and pointnet2_stack.hip
// (§18) pin together.  The distance must not be contracted into FMAs: each including file sets
// `#pragma clang fp contract(off)` itself BEFORE it includes this header (the pragma of an including file covers the
// inline functions below).
#pragma once
#include "spx_common.h"

// ((dx*dx) + (dy*dy)) + (dz*dz), rounded after each operation
__device__ __forceinline__ float sq_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;   // contraction is off in every including file
}

// float -> uint32 whose unsigned order is the order of the raw bits (-0 below +0).  NOT the ordered_bits of score_keys.h,
// which canonicalises -0 with s + 0.0f: do not unify the two.
__device__ __forceinline__ uint32_t ord_f32(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
