// box_iou.h — the rotated-BEV pair test shared by nms.hip and post_process.hip: intersection area of two rotated
// rectangles, BEV IoU and axis-aligned IoU.  One definition, so that every NMS in the library takes the same
// suppression decision for the same pair of boxes (a decision is an integer result: it must not depend on the caller).
//
// The algorithm follows the reference, quirks included: intersection polygon = {edge/edge crossings with STRICT
// straddle tests} U {corners of one box inside the other with a 1e-2 margin}, vertices sorted by angle around their
// centroid, shoelace area (reference pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:30-235, CPU twin
// src/iou3d_cpu.cpp:30-252).  The argument order matters to the last bit: callers pass (earlier box, later box).
//
// Three departures, no-ops wherever the reference's arithmetic is sound (tests/box_iou_ref.py restates them):
//   - a crossing point is moved onto the rectangle that the two segments' bounding boxes share.  Two edges on one line
//     (boxes flush along an edge, at a heading where the cross products do not cancel exactly) can pass the straddle
//     test by rounding alone, and the point then computed lies anywhere on that line: the reference returns an area that
//     is off by the box's own size.  On the shared rectangle the point is a boundary point of the intersection.
//   - where the two edges are parallel to within kEps, the reference solves the two line equations, dividing
//     differences of coordinate products by a determinant below kEps: in fp32 that is noise as soon as the coordinates
//     exceed the edge lengths.  Here the point is q0 + t (q1 - q0) with t = s1 / (s1 - s5) clamped to [0, 1]: on q.
//   - the IoU is capped at 1.  Corners taken in by the margin can make the polygon larger than either box (boxes a few
//     centimetres in size, near-duplicates), and the ratio then exceeds 1 by anything up to 1 / kEps.  No suppression
//     decision at a threshold below 1 changes.
//
// FMA contraction is off from here to the end of every file that includes this header.  Left to the compiler, the cross
// products contract differently in each kernel the pair test is inlined into: k_nms_mask and k_iou_bev have returned
// IoUs one ulp apart for the same pair, and with them different keep lists at a threshold equal to that IoU
// (tests/test_gpu_box_iou.py).  Every fp32 operation below now rounds once, in source order, in every caller.
#pragma once
#include "spx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr float kEps = 1e-8f;
constexpr float kMargin = 1e-2f;

struct P2 {
  float x, y;
};

__device__ __forceinline__ float cross3(const P2& p1, const P2& p2, const P2& p0) {
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__device__ __forceinline__ bool bbox_overlap(const P2& p1, const P2& p2, const P2& q1, const P2& q2) {
  return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
         fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

__device__ __forceinline__ bool in_box(const float* box, const P2& p) {
  float ca = cosf(-box[6]), sa = sinf(-box[6]);
  float rx = (p.x - box[0]) * ca + (p.y - box[1]) * (-sa);
  float ry = (p.x - box[0]) * sa + (p.y - box[1]) * ca;
  return fabsf(rx) < box[3] / 2 + kMargin && fabsf(ry) < box[4] / 2 + kMargin;
}

// segment p0-p1 x segment q0-q1 (strict straddling), intersection point in *ans
__device__ __forceinline__ bool seg_cross(const P2& p1, const P2& p0, const P2& q1, const P2& q0, P2* ans) {
  if (!bbox_overlap(p0, p1, q0, q1)) return false;
  float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > kEps) {
    ans->x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    ans->y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    // parallel to rounding: the point of q at the clamped parameter (fmaxf first, so that a NaN becomes 0)
    float t = fminf(fmaxf(s1 / (s1 - s5), 0.f), 1.f);
    ans->x = q0.x + t * (q1.x - q0.x);
    ans->y = q0.y + t * (q1.y - q0.y);
  }
  // onto the shared rectangle (not empty: bbox_overlap holds); fmaxf first, so that a NaN goes to the lower end
  ans->x = fminf(fmaxf(ans->x, fmaxf(fminf(p0.x, p1.x), fminf(q0.x, q1.x))), fminf(fmaxf(p0.x, p1.x), fmaxf(q0.x, q1.x)));
  ans->y = fminf(fmaxf(ans->y, fmaxf(fminf(p0.y, p1.y), fminf(q0.y, q1.y))), fminf(fmaxf(p0.y, p1.y), fmaxf(q0.y, q1.y)));
  return true;
}

__device__ void corners_of(const float* b, P2* c) {
  float hx = b[3] / 2, hy = b[4] / 2, ca = cosf(b[6]), sa = sinf(b[6]);
  const float ox[4] = {-hx, hx, hx, -hx}, oy[4] = {-hy, -hy, hy, hy};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // rotate (center + offset) around the center
    float px = b[0] + ox[k], py = b[1] + oy[k];
    c[k].x = (px - b[0]) * ca + (py - b[1]) * (-sa) + b[0];
    c[k].y = (px - b[0]) * sa + (py - b[1]) * ca + b[1];
  }
  c[4] = c[0];
}

__device__ float overlap_area(const float* a, const float* b) {
  P2 ca[5], cb[5], pts[16];
  corners_of(a, ca);
  corners_of(b, cb);
  int cnt = 0;
  float sx = 0.f, sy = 0.f;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 x;
      if (seg_cross(ca[i + 1], ca[i], cb[j + 1], cb[j], &x)) {
        pts[cnt++] = x;
        sx += x.x;
        sy += x.y;
      }
    }
  for (int k = 0; k < 4; ++k) {
    if (in_box(a, cb[k])) {
      sx += cb[k].x;
      sy += cb[k].y;
      pts[cnt++] = cb[k];
    }
    if (in_box(b, ca[k])) {
      sx += ca[k].x;
      sy += ca[k].y;
      pts[cnt++] = ca[k];
    }
  }
  if (cnt == 0) return 0.f;   // (the reference divides by zero here and sums an empty polygon: area 0)
  float cx = sx / cnt, cy = sy / cnt;
  float ang[16];
  for (int i = 0; i < cnt; ++i) ang[i] = atan2f(pts[i].y - cy, pts[i].x - cx);
  // bubble sort ascending by angle, exactly the reference's pass structure (stable w.r.t. ties)
  for (int j = 0; j < cnt - 1; ++j)
    for (int i = 0; i < cnt - j - 1; ++i)
      if (ang[i] > ang[i + 1]) {
        float t = ang[i];
        ang[i] = ang[i + 1];
        ang[i + 1] = t;
        P2 p = pts[i];
        pts[i] = pts[i + 1];
        pts[i + 1] = p;
      }
  float area = 0.f;
  for (int k = 0; k < cnt - 1; ++k) {
    float ax = pts[k].x - pts[0].x, ay = pts[k].y - pts[0].y;
    float bx = pts[k + 1].x - pts[0].x, by = pts[k + 1].y - pts[0].y;
    area += ax * by - ay * bx;
  }
  return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_bev(const float* a, const float* b) {
  float sa = a[3] * a[4], sb = b[3] * b[4];
  float so = overlap_area(a, b);
  return fminf(so / fmaxf(sa + sb - so, kEps), 1.0f);
}

__device__ __forceinline__ float iou_normal(const float* a, const float* b) {
  float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
  float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
  float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
  float inter = w * h;
  return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, kEps);
}

}  // namespace
