// box_inside.h — the point-in-rotated-box test shared by roiaware_pool3d.hip (§12), roiaware_sparse.hip and
// point_targets.hip (§16), and the RoI-aware cell of a local coordinate that the first two share.
// The semantics are pinned in the header comment of roiaware_pool3d.hip and restated in tests/roiaware_ref.py.  The local
// coordinates must not be contracted into FMAs: every file that includes this header sets `#pragma clang fp contract(off)`
// itself, before its first function (the pragma of an including file covers the inline functions below).
#pragma once
#include "spx_common.h"

constexpr float kGpuMargin = 1e-5f;

struct BoxC {            // per-box constants of the inside test
  float cx, cy, cz, cosa, sina, pad0;
  double hz, lx, ly;     // dz / 2, dx / 2 + margin, dy / 2 + margin (all in double, as the reference compares)
};

// the three limits of a box of size (dx, dy, dz); the enlarged boxes of the target assigner pass d + extra_width (float)
__device__ __forceinline__ void box_limits(BoxC& c, float dx, float dy, float dz) {
  c.hz = (double)dz / 2.0;
  c.lx = (double)dx / 2.0 + (double)kGpuMargin;
  c.ly = (double)dy / 2.0 + (double)kGpuMargin;
}

__device__ __forceinline__ BoxC box_consts(const float* bx) {
  BoxC c;
  c.cx = bx[0];
  c.cy = bx[1];
  c.cz = bx[2];
  const float rz = bx[6];
  c.cosa = (float)cos((double)(-rz));
  c.sina = (float)sin((double)(-rz));
  c.pad0 = 0.f;
  box_limits(c, bx[3], bx[4], bx[5]);
  return c;
}

// the reference's check_pt_in_box3d; local_x / local_y are written only when the z test passes
__device__ __forceinline__ bool in_box(const BoxC& b, float x, float y, float z, float& lx, float& ly) {
  if ((double)fabsf(z - b.cz) > b.hz) return false;
  const float sx = x - b.cx, sy = y - b.cy;
  lx = sx * b.cosa + sy * (-b.sina);   // contraction is off in every including file
  ly = sx * b.sina + sy * b.cosa;
  return (double)fabsf(lx) < b.lx && (double)fabsf(ly) < b.ly;
}

// float -> int as the hardware convert does it: saturating, NaN -> 0
__device__ __forceinline__ int f2i_sat(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.f) return INT32_MAX;
  if (f <= -2147483648.f) return INT32_MIN;
  return (int)f;
}

// the cell of a local coordinate along one axis of a box of size d cut into o cells, clamped to o - 1
__device__ __forceinline__ unsigned cell_axis(float local, float d, int o) {
  const float res = d / (float)o;
  const unsigned u = (unsigned)f2i_sat((local + d / 2.f) / res);
  return u < (unsigned)(o - 1) ? u : (unsigned)(o - 1);
}
