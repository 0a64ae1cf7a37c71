// center_targets.hip — target assignment of the centre head for a whole batch and every head, two launches, no host
// read (include/spx.h §20).  Replaces CenterHead.assign_targets / assign_target_of_single_head (reference
// pcdet/models/dense_heads/center_head.py:103-219) with gaussian_radius and draw_gaussian_to_heatmap
// (pcdet/models/model_utils/centernet_utils.py:9-69): a Python loop over heads x frames x boxes that moves every frame's
// boxes to the host, reads radius[k].item() per box and builds each Gaussian in numpy.
//
// Launch 1, one workgroup per frame: every box looks up its head and its class within the head, takes its slot (its
// rank among the frame's boxes of that head, in input order) and writes the slot's target_boxes / inds / mask rows and
// a draw record (centre cell, radius, channel) to the workspace; the slots no box takes are zeroed.
// Launch 2, one thread per heatmap element: the element scans the draw records of its frame and head and keeps the
// maximum of the Gaussians whose window covers it, 0 without one.  Every output element is written exactly once, by one
// thread, and max is order independent: no atomics, bitwise reproducible.
//
// Pinned semantics (tests/center_targets_ref.py restates all of it in numpy):
//   - class = (int) of the LAST column; ids outside 1..num_class and classes the table gives to no head own no slot.
//     gt_boxes is never written (the reference rewrites the class column in place while it filters per head).
//   - coord = ((x - range0) / vs0) / stride in float, rounded after every operation; clamped to [0, W - 0.5] /
//     [0, H - 0.5]; cell = (int)coord; inds = cell_y * W + cell_x.
//   - radius = gaussian_radius((dx / vs0) / stride, (dy / vs1) / stride, min_overlap) in float with the reference's
//     operation order (its Python scalars are doubles rounded to float where they meet the tensor) and a correctly
//     rounded sqrt; (int), then max(., min_radius).  A slot whose scaled dx or dy is not > 0 keeps its place with mask 0
//     and zeros and draws nothing.
//   - Gaussian: window [cx - r, cx + r] x [cy - r, cy + r] clipped to the map, exp(-(ddx^2 + ddy^2) / (2 s s)) with
//     s = (2 r + 1) / 6 evaluated in DOUBLE and rounded once to float, as numpy does for the reference; the centre is
//     exactly 1.  The reference's eps * max cut-off never fires (the smallest window value is > exp(-9)).
//   - target_boxes row: coord - (float)cell (2), z, logf(dx, dy, dz), cosf(rz), sinf(rz), then columns 7 .. C - 2.
#include "spx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxHeads = 16;

struct CenterArgs {
  const float* gt;
  int b, m, ld;
  const int32_t* table;   // device [num_class + 1, 2]: head, 1-based class within the head; -1: no head
  int num_class, n_heads;
  int chan_off[kMaxHeads + 1];
  float x0, y0, vs0, vs1, stride;
  int w, h, k;
  float k1n, k1d, k2, kb3, kc3, k4a3;
  int min_radius;
  float* heat;
  float* boxes;
  int64_t* inds;
  int64_t* mask;
  int32_t* cnt;   // ws: [n_heads, b] live slots
  int4* draw;     // ws: [n_heads, b, k] (cell x, cell y, radius or -1, channel)
};

__device__ __forceinline__ float clamp_keep_nan(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

__device__ __forceinline__ int gaussian_radius_int(const CenterArgs& a, float height, float width) {
  const float hw = height + width, wh = width * height;
  const float c1 = wh * a.k1n / a.k1d;
  const float r1 = (hw + sqrtf(hw * hw - 4.f * c1)) / 2.f;
  const float b2 = 2.f * hw, c2 = a.k2 * width * height;
  const float r2 = (b2 + sqrtf(b2 * b2 - 16.f * c2)) / 2.f;
  const float b3 = a.kb3 * hw, c3 = a.kc3 * width * height;
  const float r3 = (b3 + sqrtf(b3 * b3 - a.k4a3 * c3)) / 2.f;
  const float rad = fminf(fminf(r1, r2), r3);
  int r = a.min_radius;
  if (rad >= 1073741824.f)
    r = 1073741824;
  else if (rad > (float)a.min_radius)
    r = (int)rad;   // NaN stays at min_radius
  return r;
}

// grid (b).  The frame's boxes go through in chunks of 256, one box per thread.
__global__ __launch_bounds__(kThreads) void k_center_slots(const CenterArgs a) {
  __shared__ int s_head[kThreads];
  __shared__ int s_base[kMaxHeads];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid < kMaxHeads) s_base[tid] = 0;
  __syncthreads();
  for (int base = 0; base < a.m; base += kThreads) {
    const int i = base + tid, len = min(kThreads, a.m - base);
    const float* row = a.gt + ((size_t)f * a.m + (i < a.m ? i : 0)) * a.ld;
    int head = -1, cls = 0;
    if (i < a.m) {
      const float cv = row[a.ld - 1];
      if (cv >= 1.f && cv < (float)(a.num_class + 1)) {
        const int gc = (int)cv;
        head = a.table[2 * gc];
        cls = a.table[2 * gc + 1];
        if (head < 0 || head >= a.n_heads || cls < 1 || cls > a.chan_off[head + 1] - a.chan_off[head]) head = -1;
      }
    }
    s_head[tid] = head;
    __syncthreads();
    if (head >= 0) {
      int slot = s_base[head];
      for (int j = 0; j < tid; ++j) slot += s_head[j] == head;
      if (slot < a.k) {
        const size_t r = ((size_t)head * a.b + f) * a.k + slot;
        const float cxf = clamp_keep_nan((row[0] - a.x0) / a.vs0 / a.stride, (float)a.w - 0.5f);
        const float cyf = clamp_keep_nan((row[1] - a.y0) / a.vs1 / a.stride, (float)a.h - 0.5f);
        const float sdx = row[3] / a.vs0 / a.stride, sdy = row[4] / a.vs1 / a.stride;
        const bool live = sdx > 0.f && sdy > 0.f && cxf == cxf && cyf == cyf;
        float* o = a.boxes + r * a.ld;
        int4 d = make_int4(0, 0, -1, 0);
        if (live) {
          const int cx = (int)cxf, cy = (int)cyf;
          d = make_int4(cx, cy, gaussian_radius_int(a, sdx, sdy), cls - 1);
          o[0] = cxf - (float)cx;
          o[1] = cyf - (float)cy;
          o[2] = row[2];
          o[3] = logf(row[3]);
          o[4] = logf(row[4]);
          o[5] = logf(row[5]);
          o[6] = cosf(row[6]);
          o[7] = sinf(row[6]);
          for (int c = 8; c < a.ld; ++c) o[c] = row[c - 1];
          a.inds[r] = (int64_t)cy * a.w + cx;
          a.mask[r] = 1;
        } else {
          for (int c = 0; c < a.ld; ++c) o[c] = 0.f;
          a.inds[r] = 0;
          a.mask[r] = 0;
        }
        a.draw[r] = d;
      }
    }
    __syncthreads();
    if (tid < a.n_heads) {
      int c = 0;
      for (int j = 0; j < len; ++j) c += s_head[j] == tid;
      s_base[tid] += c;
    }
    __syncthreads();
  }
  if (tid < a.n_heads) a.cnt[tid * a.b + f] = min(s_base[tid], a.k);
  for (int e = tid; e < a.n_heads * a.k; e += kThreads) {
    const int head = e / a.k, slot = e - head * a.k;
    if (slot < s_base[head]) continue;
    const size_t r = ((size_t)head * a.b + f) * a.k + slot;
    float* o = a.boxes + r * a.ld;
    for (int c = 0; c < a.ld; ++c) o[c] = 0.f;
    a.inds[r] = 0;
    a.mask[r] = 0;
    a.draw[r] = make_int4(0, 0, -1, 0);
  }
}

// grid (ceil(h * w / 256), b * total channels): blockIdx.y = frame * total + global channel.
__global__ __launch_bounds__(kThreads) void k_center_heatmap(const CenterArgs a) {
  __shared__ int4 s_draw[kThreads];
  const int total = a.chan_off[a.n_heads];
  const int f = blockIdx.y / total, gc = blockIdx.y - f * total, tid = threadIdx.x;
  int head = 0;
  while (head + 1 < a.n_heads && gc >= a.chan_off[head + 1]) ++head;
  const int ch = gc - a.chan_off[head], n_ch = a.chan_off[head + 1] - a.chan_off[head];
  const int hw = a.h * a.w, p = blockIdx.x * kThreads + tid;
  const int py = p / a.w, px = p - py * a.w;
  const size_t list = ((size_t)head * a.b + f) * a.k;
  const int cnt = a.cnt[head * a.b + f];
  float v = 0.f;
  for (int base = 0; base < cnt; base += kThreads) {
    const int len = min(kThreads, cnt - base);
    __syncthreads();
    if (tid < len) {
      int4 d = a.draw[list + base + tid];
      if (d.w != ch) d.z = -1;
      s_draw[tid] = d;
    }
    __syncthreads();
    if (p < hw) {
      for (int j = 0; j < len; ++j) {
        const int4 d = s_draw[j];
        const int ddx = px - d.x, ddy = py - d.y;
        if (abs(ddx) <= d.z && abs(ddy) <= d.z) {
          const double sigma = (double)(2 * (int64_t)d.z + 1) / 6.0;
          const double g = exp(-(double)((int64_t)ddx * ddx + (int64_t)ddy * ddy) / (2.0 * sigma * sigma));
          v = fmaxf(v, (float)g);
        }
      }
    }
  }
  if (p < hw) a.heat[(size_t)a.b * hw * a.chan_off[head] + ((size_t)f * n_ch + ch) * hw + p] = v;
}

size_t cnt_bytes(int64_t b, int64_t n_heads) { return spx_align((size_t)(b * n_heads) * sizeof(int32_t)); }

}  // namespace

extern "C" size_t spx_center_assign_targets_ws_bytes(int32_t b, int32_t n_heads, int64_t num_max_objs) {
  if (b <= 0 || n_heads <= 0 || num_max_objs <= 0) return 0;
  return cnt_bytes(b, n_heads) + (size_t)b * n_heads * num_max_objs * sizeof(int4);
}

extern "C" int spx_center_assign_targets(const float* gt_boxes, int32_t b, int64_t m, int32_t ld,
                                         const int32_t* class_to_head_slot, int32_t num_class, int32_t n_heads,
                                         const int32_t* head_channels, const float* range_lo2, const float* voxel_size2,
                                         float feature_map_stride, int32_t w, int32_t h, int64_t num_max_objs,
                                         double gaussian_overlap, int32_t min_radius, float* heatmaps,
                                         float* target_boxes, int64_t* inds, int64_t* masks, void* ws, size_t ws_bytes,
                                         spx_stream_t stream) {
  if (b < 0 || m < 0 || ld < 8 || num_class < 0 || n_heads < 1 || w < 1 || h < 1 || num_max_objs < 1)
    return SPX_ERR_INVALID_ARG;
  if (!class_to_head_slot || !head_channels || !range_lo2 || !voxel_size2 || (m > 0 && !gt_boxes) || !heatmaps ||
      !target_boxes || !inds || !masks)
    return SPX_ERR_INVALID_ARG;
  if (n_heads > kMaxHeads) return SPX_ERR_UNSUPPORTED;
  CenterArgs a;
  a.chan_off[0] = 0;
  for (int i = 0; i < n_heads; ++i) {
    if (head_channels[i] < 1 || head_channels[i] > 65535) return SPX_ERR_INVALID_ARG;
    a.chan_off[i + 1] = a.chan_off[i] + head_channels[i];
  }
  for (int i = n_heads; i < kMaxHeads; ++i) a.chan_off[i + 1] = a.chan_off[n_heads];
  const int64_t total = a.chan_off[n_heads], hw = (int64_t)w * h;
  if (b == 0) return SPX_OK;
  if (b > 65535 || b * total > 65535 || m >= INT32_MAX - kThreads || hw >= INT32_MAX - kThreads ||
      num_max_objs * n_heads >= INT32_MAX || (int64_t)b * total * hw >= ((int64_t)1 << 40) ||
      (int64_t)b * n_heads * num_max_objs * ld >= ((int64_t)1 << 40))
    return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < spx_center_assign_targets_ws_bytes(b, n_heads, num_max_objs)) return SPX_ERR_WORKSPACE;
  a.gt = gt_boxes;
  a.b = b;
  a.m = (int)m;
  a.ld = ld;
  a.table = class_to_head_slot;
  a.num_class = num_class;
  a.n_heads = n_heads;
  a.x0 = range_lo2[0];
  a.y0 = range_lo2[1];
  a.vs0 = voxel_size2[0];
  a.vs1 = voxel_size2[1];
  a.stride = feature_map_stride;
  a.w = w;
  a.h = h;
  a.k = (int)num_max_objs;
  // gaussian_radius' Python scalars: doubles, rounded to float where they meet the float tensor
  const double mo = gaussian_overlap;
  a.k1n = (float)(1 - mo);
  a.k1d = (float)(1 + mo);
  a.k2 = (float)(1 - mo);
  a.kb3 = (float)(-2 * mo);
  a.kc3 = (float)(mo - 1);
  a.k4a3 = (float)(4 * (4 * mo));
  a.min_radius = min_radius;
  a.heat = heatmaps;
  a.boxes = target_boxes;
  a.inds = inds;
  a.mask = masks;
  a.cnt = reinterpret_cast<int32_t*>(ws);
  a.draw = reinterpret_cast<int4*>(reinterpret_cast<char*>(ws) + cnt_bytes(b, n_heads));
  hipLaunchKernelGGL(k_center_slots, dim3((unsigned)b), dim3(kThreads), 0, spx_s(stream), a);
  SPX_CHECK_LAUNCH();
  const dim3 grid((unsigned)((hw + kThreads - 1) / kThreads), (unsigned)(b * total));
  hipLaunchKernelGGL(k_center_heatmap, grid, dim3(kThreads), 0, spx_s(stream), a);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
