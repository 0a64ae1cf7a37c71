// point_targets.hip — target assignment of the point heads for a whole batch in one launch, no host read
// (include/spx.h §16).  Replaces the per-frame loop of the fork's point head and SASA loss (reference
// point_head_vote_sasa_statistic_distillation.py: assign_stack_targets_mask, assign_stack_targets_simple,
// generate_centerness_label; loss_utils.py: PointSASALoss.assign_target): points_in_boxes_gpu once or twice per frame,
// boolean-mask indexing (a count read per mask), PointBinResidualCoder.encode_torch on the compacted rows, a scatter
// back.  Here every point scans its frame's boxes, takes its label from the first box that holds it and writes its own
// rows; outputs have the static shape b * n and nothing is compacted, so the call can be captured in a graph.
//
// Pinned semantics (tests/point_targets_ref.py restates all of it in float32 numpy):
//   - inside test: box_inside.h, the one of spx_points_in_boxes, FMA contraction OFF for this whole file.  The enlarged
//     box of (dx, dy, dz) is (dx + ew0, dy + ew1, dz + ew2) in float, then the same limits.
//   - mode 0 (plain): hit = first enlarged box holding the point; label = class of the hit, else 0.
//     mode 1 (ignore ring): hit = first gt box; label = class of the hit, else -1 when any enlarged box holds the point.
//     mode 2 (ball): hit = first gt box; d = centre - point in float, sqrtf(dx*dx + dy*dy + dz*dz) < radius keeps the
//       class, else -1.  Only the first hit is looked at, as in the reference.
//     class = 1 when num_class == 1, else (int64)box[7].  A point is FOREGROUND when its label is > 0; every float row of
//     a point that is not is zero.  (The reference also fills the rows of a hit whose class truncates to <= 0 with
//     num_class > 1, rows that its losses mask out; zero-padded gt rows are otherwise scanned like any other box.)
//   - box_labels: the hit's 7 box values as stored (not enlarged, sizes not clamped); center_labels: its xyz.
//   - reg_labels: PointBinResidualCoder.encode_torch, use_mean_size False, as torch evaluates it on the CPU in float:
//     g - p; logf(d < 1e-5f ? 1e-5f : d); angle = rem(rz, 2pi_f), shifted = rem(angle + half_f, 2pi_f) with rem the
//     fmodf-based floor remainder; bin = floorf(shifted / apc_f) (IEEE divide); residual = (shifted - (bin * apc_f +
//     half_f)) / apc_f; 2pi_f, apc_f, half_f the float roundings of 2 pi, 2 pi / bins, (2 pi / bins) / 2 taken in
//     double.  One-hot 1.0f at the bin, residual at the bin and 0.0f * residual elsewhere.  A bin outside [0, bins)
//     (torch raises there) writes no 1.  Exactly reproducible except for logf.
//   - centerness: c = p - centre; x' = c.x * cosf(-rz) + c.y * (-sinf(-rz)), y' = c.x * sinf(-rz) + c.y * cosf(-rz);
//     front / back = dx / 2 -+ x' and so on; ratios min / max; powf(prod < 1e-6f ? 1e-6f : prod, 1.f / 3.f).
#include "spx_common.h"

#pragma clang fp contract(off)

#include "box_inside.h"   // after the pragma, which covers its inline functions

namespace {

constexpr int kThreads = 256;   // points per workgroup = boxes staged per LDS chunk
constexpr int kRowLd = 17;      // floats of a point's record in LDS; odd, so a thread-per-row write has no bank conflict
constexpr int kMaxBins = 32;

// a point's record: [0, 7) box, [7, 10) offsets, [10, 13) log sizes, 13 bin residual, 14 bin (int bits, -1: none)
constexpr int kRecOff = 7, kRecLog = 10, kRecRes = 13, kRecBin = 14;

struct TargetArgs {
  const float* pts;
  const float* boxes;
  int n, m, ld;
  float ew[3];
  float radius;
  int num_class, bins;
  float two_pi, apc, half_apc;
  int64_t* cls;
  int32_t* box_idx;
  float* box_labels;
  float* center;
  float* reg;
  float* centerness;
};

// torch.remainder for floats on the CPU: fmod, then the divisor added when the signs differ
__device__ __forceinline__ float floor_rem(float a, float b) {
  float m = fmodf(a, b);
  if (m != 0.f && ((b < 0.f) != (m < 0.f))) m += b;
  return m;
}

// grid (ceil(n / 256), b).  The workgroup stages the frame's boxes 256 at a time (the constants of the gt boxes and / or
// of the enlarged ones, as the mode needs), every thread scans them in ascending index for its own point, and the
// workgroup leaves the chunk loop once no point is still looking.  Each thread then builds its point's record in LDS and
// the workgroup writes the row outputs from there, consecutive threads to consecutive addresses.
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_point_assign(const TargetArgs a) {
  __shared__ BoxC s_box[MODE != 0 ? kThreads : 1];    // gt boxes
  __shared__ BoxC s_grow[MODE != 2 ? kThreads : 1];   // enlarged boxes
  __shared__ float s_row[kThreads * kRowLd];
  const int b = blockIdx.y, tid = threadIdx.x, i0 = blockIdx.x * kThreads, i = i0 + tid;
  const bool live = i < a.n;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float* p = a.pts + ((size_t)b * a.n + i) * 3;
    x = p[0];
    y = p[1];
    z = p[2];
  }
  const float* B = a.boxes + (size_t)b * a.m * a.ld;
  int hit = -1;
  bool grown = false;   // mode 1: some enlarged box holds the point
  for (int base = 0; base < a.m; base += kThreads) {
    const bool looking = live && (hit < 0 || (MODE == 1 && !grown));
    if (!__syncthreads_or(looking)) break;   // also orders the previous chunk's reads before the refill
    const int len = min(kThreads, a.m - base);
    if (tid < len) {
      const float* bx = B + (size_t)(base + tid) * a.ld;
      BoxC c = box_consts(bx);
      if (MODE != 0) s_box[tid] = c;
      if (MODE != 2) {
        box_limits(c, bx[3] + a.ew[0], bx[4] + a.ew[1], bx[5] + a.ew[2]);
        s_grow[tid] = c;
      }
    }
    __syncthreads();
    if (looking) {
      float lx, ly;
      for (int k = 0; k < len; ++k) {
        if (MODE == 1) {
          if (hit < 0 && in_box(s_box[k], x, y, z, lx, ly)) hit = base + k;
          if (!grown && in_box(s_grow[k], x, y, z, lx, ly)) grown = true;
          if (hit >= 0 && grown) break;
        } else if (in_box(MODE == 0 ? s_grow[k] : s_box[k], x, y, z, lx, ly)) {
          hit = base + k;
          break;
        }
      }
    }
  }

  float* rec = s_row + tid * kRowLd;
  int64_t label = 0;
  float g[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (hit >= 0) {
    const float* bx = B + (size_t)hit * a.ld;
    label = a.num_class == 1 ? (int64_t)1 : (int64_t)bx[7];
    if (MODE == 2) {
      const float ex = bx[0] - x, ey = bx[1] - y, ez = bx[2] - z;
      if (!(sqrtf(ex * ex + ey * ey + ez * ez) < a.radius)) label = -1;
    }
    if (label > 0) {
#pragma unroll
      for (int c = 0; c < 7; ++c) g[c] = bx[c];
    }
  } else if (MODE == 1 && grown) {
    label = -1;
  }
  const bool fg = label > 0;
  float off[3] = {0.f, 0.f, 0.f}, lg[3] = {0.f, 0.f, 0.f}, res = 0.f, ctr = 0.f;
  int bin = -1;
  if (fg) {
    if (a.reg != nullptr && a.bins > 0) {
      off[0] = g[0] - x;
      off[1] = g[1] - y;
      off[2] = g[2] - z;
#pragma unroll
      for (int c = 0; c < 3; ++c) lg[c] = logf(g[3 + c] < 1e-5f ? 1e-5f : g[3 + c]);
      const float angle = floor_rem(g[6], a.two_pi);
      const float shifted = floor_rem(angle + a.half_apc, a.two_pi);
      const float cf = floorf(shifted / a.apc);
      res = (shifted - (cf * a.apc + a.half_apc)) / a.apc;
      bin = (cf >= 0.f && cf < (float)a.bins) ? (int)cf : -1;
    }
    if (a.centerness != nullptr) {
      const float cx = x - g[0], cy = y - g[1], cz = z - g[2];
      const float ca = cosf(-g[6]), sa = sinf(-g[6]);
      const float rx = cx * ca + cy * (-sa), ry = cx * sa + cy * ca;
      const float f0 = g[3] / 2.f - rx, f1 = g[3] / 2.f + rx;
      const float l0 = g[4] / 2.f - ry, l1 = g[4] / 2.f + ry;
      const float t0 = g[5] / 2.f - cz, t1 = g[5] / 2.f + cz;
      const float prod = fminf(f0, f1) / fmaxf(f0, f1) * (fminf(l0, l1) / fmaxf(l0, l1)) * (fminf(t0, t1) / fmaxf(t0, t1));
      ctr = powf(prod < 1e-6f ? 1e-6f : prod, 1.f / 3.f);
    }
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) rec[c] = g[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rec[kRecOff + c] = off[c];
    rec[kRecLog + c] = lg[c];
  }
  rec[kRecRes] = res;
  rec[kRecBin] = __int_as_float(bin);

  const size_t row0 = (size_t)b * a.n + i0;
  if (live) {
    a.cls[row0 + tid] = label;
    a.box_idx[row0 + tid] = hit;
    if (a.centerness != nullptr) a.centerness[row0 + tid] = ctr;
  }
  __syncthreads();
  const int cnt = min(kThreads, a.n - i0);
  if (a.box_labels != nullptr) {
    float* o = a.box_labels + row0 * 7;
    for (int e = tid; e < cnt * 7; e += kThreads) {
      const int r = e / 7;
      o[e] = s_row[r * kRowLd + (e - r * 7)];
    }
  }
  if (a.center != nullptr) {
    float* o = a.center + row0 * 3;
    for (int e = tid; e < cnt * 3; e += kThreads) {
      const int r = e / 3;
      o[e] = s_row[r * kRowLd + (e - r * 3)];
    }
  }
  if (a.reg != nullptr && a.bins > 0) {
    const int w = 6 + 2 * a.bins;
    float* o = a.reg + row0 * w;
    for (int e = tid; e < cnt * w; e += kThreads) {
      const int r = e / w, c = e - r * w;
      const float* q = s_row + r * kRowLd;
      const int rb = __float_as_int(q[kRecBin]);
      float v;
      if (c < 6)
        v = q[kRecOff + c];
      else if (c < 6 + a.bins)
        v = c - 6 == rb ? 1.f : 0.f;
      else
        v = c - 6 - a.bins == rb ? q[kRecRes] : 0.f * q[kRecRes];
      o[e] = v;
    }
  }
}

}  // namespace

extern "C" int spx_point_assign_targets(const float* points, const float* gt_boxes, int32_t b, int64_t n, int64_t m,
                                        int32_t ld, const float* extra_width, int32_t mode, float central_radius,
                                        int32_t num_class, int32_t angle_bin_num, int64_t* cls_labels, int32_t* box_idx,
                                        float* box_labels, float* center_labels, float* reg_labels, float* centerness,
                                        spx_stream_t stream) {
  if (b < 0 || n < 0 || m < 0 || ld < 8) return SPX_ERR_INVALID_ARG;
  if (!points || (m > 0 && !gt_boxes) || !extra_width || !cls_labels || !box_idx) return SPX_ERR_INVALID_ARG;
  if (mode < 0 || mode > 2 || angle_bin_num < 0 || angle_bin_num > kMaxBins) return SPX_ERR_UNSUPPORTED;
  if (b == 0 || n == 0) return SPX_OK;
  if (b > 65535 || n >= INT32_MAX - kThreads || m >= INT32_MAX - kThreads ||
      (int64_t)b * n * (6 + 2 * angle_bin_num) >= ((int64_t)1 << 40))
    return SPX_ERR_TOO_LARGE;
  TargetArgs a;
  a.pts = points;
  a.boxes = gt_boxes;
  a.n = (int)n;
  a.m = (int)m;
  a.ld = ld;
  for (int i = 0; i < 3; ++i) a.ew[i] = extra_width[i];
  a.radius = central_radius;
  a.num_class = num_class;
  a.bins = angle_bin_num;
  const double two_pi = 3.141592653589793 * 2.0, apc = angle_bin_num > 0 ? two_pi / (double)angle_bin_num : 0.0;
  a.two_pi = (float)two_pi;
  a.apc = (float)apc;
  a.half_apc = (float)(apc / 2.0);
  a.cls = cls_labels;
  a.box_idx = box_idx;
  a.box_labels = box_labels;
  a.center = center_labels;
  a.reg = reg_labels;
  a.centerness = centerness;
  const dim3 grid((unsigned)((n + kThreads - 1) / kThreads), (unsigned)b), block(kThreads);
  if (mode == 0)
    hipLaunchKernelGGL(k_point_assign<0>, grid, block, 0, spx_s(stream), a);
  else if (mode == 1)
    hipLaunchKernelGGL(k_point_assign<1>, grid, block, 0, spx_s(stream), a);
  else
    hipLaunchKernelGGL(k_point_assign<2>, grid, block, 0, spx_s(stream), a);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
