// proposal_targets.hip — RoI / GT matching and fg / bg sampling of the second stage for the whole batch
// (include/spx.h §26).
//
// Replaces ProposalTargetLayer.sample_rois_for_rcnn, subsample_rois, sample_bg_inds and get_max_iou_with_same_class
// (reference pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:64-228): a Python loop over frames and, with
// SAMPLE_ROI_BY_EACH_CLASS, over classes, each with an IoU launch, nonzero / numel / item host reads and numpy and
// CPU-torch random numbers.  Here the random draws are inputs (fg_keys, slot_u) and two launches serve the batch:
//   k_pair_iou   one thread per (frame, RoI, GT row): the 3-D IoU with box_iou.h's overlap_area, 0 for a pair of
//                different classes when sampling by class;
//   k_sample     one block per frame: trailing zero GT rows trimmed, per-RoI maximum (ties: lowest GT row), the fg / hard
//                / easy candidate lists in ascending RoI order, the fg ranks by counting smaller (key, index) pairs, and
//                one output slot per thread.
// Integer atomics only (one LDS atomicMax for the trim), no host read, every output a pure function of the inputs.
#include "spx_common.h"
#include "box_iou.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = 2048;               // RoIs per frame: five LDS arrays of kMaxR words = 40 KiB

// iou3d_nms_utils.boxes_iou3d_gpu for one pair, the tensor expression's operations in its order (contraction is off)
__device__ __forceinline__ float iou3d_pair(const float* a, const float* b) {
  const float a_max = a[2] + a[5] / 2, a_min = a[2] - a[5] / 2, b_max = b[2] + b[5] / 2, b_min = b[2] - b[5] / 2;
  const float bev = overlap_area(a, b);
  const float hgt = fmaxf(fminf(a_max, b_max) - fmaxf(a_min, b_min), 0.f);
  const float o3 = bev * hgt;
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  return o3 / fmaxf(va + vb - o3, 1e-6f);
}

__global__ void k_pair_iou(const float* __restrict__ rois, const int64_t* __restrict__ roi_labels,
                           const float* __restrict__ gt, int64_t total, int r, int roi_stride, int gmax, int gt_stride,
                           int by_class, float* __restrict__ iou) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int g = (int)(t % gmax);
  const int64_t br = t / gmax;             // frame * r + roi
  const int64_t b = br / r;
  const float* pg = gt + (b * gmax + g) * gt_stride;
  float v = 0.f;
  if (!by_class || roi_labels[br] == (int64_t)pg[gt_stride - 1]) {
    float a7[7], b7[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      a7[j] = rois[br * roi_stride + j];
      b7[j] = pg[j];
    }
    v = iou3d_pair(a7, b7);
  }
  iou[t] = v;
}

__global__ __launch_bounds__(kThreads) void k_sample(const float* __restrict__ iou, const int64_t* __restrict__ roi_labels,
                                                     const float* __restrict__ gt, int r, int gmax, int gt_stride, int m,
                                                     int fg_per_image, float reg_fg, float cls_fg, float bg_lo,
                                                     double hard_ratio, int by_class, const float* __restrict__ fg_keys,
                                                     const float* __restrict__ slot_u, int64_t* __restrict__ sampled,
                                                     float* __restrict__ roi_ious, int64_t* __restrict__ gt_inds) {
  __shared__ float ovl[kMaxR];
  __shared__ int asg[kMaxR];
  __shared__ int fg_list[kMaxR], hard_list[kMaxR], easy_list[kMaxR];
  __shared__ int cnt[3][kThreads + 1];
  __shared__ int k_last;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* gtb = gt + (int64_t)b * gmax * gt_stride;
  const int64_t* lab = roi_labels + (int64_t)b * r;
  const float* ioub = iou + (int64_t)b * r * gmax;

  // trailing GT rows whose sum is 0 are dropped; row 0 always stays, interior zero rows stay
  if (tid == 0) k_last = 0;
  __syncthreads();
  for (int g = tid; g < gmax; g += kThreads) {
    float s = 0.f;
    for (int j = 0; j < gt_stride; ++j) s += gtb[(int64_t)g * gt_stride + j];
    if (s != 0.f) atomicMax(&k_last, g);
  }
  __syncthreads();
  const int n_gt = k_last + 1;
  const float fg_thresh = fminf(reg_fg, cls_fg);

  // each thread owns the contiguous RoIs [lo, hi): lists come out in ascending RoI order
  const int per = (r + kThreads - 1) / kThreads;
  const int lo = min(tid * per, r), hi = min(lo + per, r);
  int n3[3] = {0, 0, 0};
  for (int i = lo; i < hi; ++i) {
    float best = -1.f;
    int arg = 0;
    bool any = false;
    for (int g = 0; g < n_gt; ++g) {
      if (by_class && lab[i] != (int64_t)gtb[(int64_t)g * gt_stride + gt_stride - 1]) continue;
      const float v = ioub[(int64_t)i * gmax + g];
      if (!any || v > best) {
        best = v;
        arg = g;
        any = true;
      }
    }
    if (!any) best = 0.f;                  // no GT of this class: overlap 0, assignment 0
    ovl[i] = best;
    asg[i] = arg;
    n3[0] += best >= fg_thresh;
    n3[1] += best < reg_fg && best >= bg_lo;
    n3[2] += best < bg_lo;
  }
  for (int q = 0; q < 3; ++q) cnt[q][tid] = n3[q];
  __syncthreads();
  if (tid < 3) {                           // exclusive scan of 256 counts, one list per thread
    int run = 0;
    for (int i = 0; i < kThreads; ++i) {
      const int v = cnt[tid][i];
      cnt[tid][i] = run;
      run += v;
    }
    cnt[tid][kThreads] = run;
  }
  __syncthreads();
  {
    int p0 = cnt[0][tid], p1 = cnt[1][tid], p2 = cnt[2][tid];
    for (int i = lo; i < hi; ++i) {
      const float v = ovl[i];
      if (v >= fg_thresh) fg_list[p0++] = i;
      if (v < reg_fg && v >= bg_lo) hard_list[p1++] = i;
      if (v < bg_lo) easy_list[p2++] = i;
    }
  }
  __syncthreads();
  const int n_fg = cnt[0][kThreads], n_hard = cnt[1][kThreads], n_easy = cnt[2][kThreads];
  const int n_bg = n_hard + n_easy;

  // slot layout: [0, n_take) fg without replacement (only when bg exists), then hard bg, then easy bg
  int n_take = 0, n_hard_slots = 0;
  const bool fg_only = n_fg > 0 && n_bg == 0;
  if (!fg_only) {
    n_take = n_bg > 0 ? min(fg_per_image, n_fg) : 0;
    const int bg_slots = m - n_take;
    if (n_hard > 0 && n_easy > 0)
      n_hard_slots = min((int)((double)bg_slots * hard_ratio), n_hard);
    else if (n_hard > 0)
      n_hard_slots = bg_slots;
    if (n_hard_slots < 0) n_hard_slots = 0;
  }
  int64_t* sb = sampled + (int64_t)b * m;

  // fg without replacement: ascending (key, RoI index); the rank is the number of smaller pairs
  if (n_take > 0) {
    const float* keys = fg_keys + (int64_t)b * r;
    for (int p = tid; p < n_fg; p += kThreads) {
      const int i = fg_list[p];
      const float ki = keys[i];
      int rank = 0;
      for (int q = 0; q < n_fg; ++q) {
        const int j = fg_list[q];
        const float kj = keys[j];
        rank += (kj < ki) || (kj == ki && j < i);
      }
      if (rank < n_take) sb[rank] = i;
    }
  }
  __syncthreads();
  for (int s = tid; s < m; s += kThreads) {
    int pick;
    if (s < n_take) {
      pick = (int)sb[s];                   // written above by this block (ranks of distinct finite keys are distinct)
      if (pick < 0 || pick >= r) pick = 0; // NaN keys leave a rank unwritten: stay inside the frame
    } else {
      const int* list;
      int n;
      if (fg_only) {
        list = fg_list;
        n = n_fg;
      } else if (s < n_take + n_hard_slots) {
        list = hard_list;
        n = n_hard;
      } else {
        list = easy_list;
        n = n_easy;
      }
      if (n <= 0) {
        pick = 0;                          // no candidate of any kind (NaN overlaps only)
      } else {
        const double v = floor((double)slot_u[(int64_t)b * m + s] * n);
        int q = v >= 0.0 ? (v < (double)n ? (int)v : n - 1) : 0;   // min(floor(u n), n - 1); a NaN or negative draw: 0
        pick = list[q];
      }
    }
    sb[s] = pick;
    roi_ious[(int64_t)b * m + s] = ovl[pick];
    gt_inds[(int64_t)b * m + s] = asg[pick];
  }
}

}  // namespace

extern "C" size_t spx_proposal_sample_ws_bytes(int32_t batch, int32_t r, int32_t gmax) {
  if (batch < 1 || r < 1 || gmax < 1) return 0;
  return spx_align((size_t)batch * r * gmax * sizeof(float));
}

extern "C" int spx_proposal_sample(const float* rois, const int64_t* roi_labels, const float* gt_boxes, int32_t batch,
                                   int32_t r, int32_t roi_stride, int32_t gmax, int32_t gt_stride, int32_t m,
                                   int32_t fg_per_image, float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh_lo,
                                   double hard_bg_ratio, int by_class, const float* fg_keys, const float* slot_u,
                                   int64_t* sampled_inds, float* roi_ious, int64_t* gt_inds, void* ws, size_t ws_bytes,
                                   spx_stream_t stream) {
  if (batch < 0 || r < 1 || roi_stride < 7 || gmax < 1 || gt_stride < 8 || m < 1 || fg_per_image < 0 || fg_per_image > m)
    return SPX_ERR_INVALID_ARG;
  if (!(hard_bg_ratio >= 0.0 && hard_bg_ratio <= 1.0)) return SPX_ERR_INVALID_ARG;
  if (batch == 0) return SPX_OK;
  if (!rois || !roi_labels || !gt_boxes || !fg_keys || !slot_u || !sampled_inds || !roi_ious || !gt_inds)
    return SPX_ERR_INVALID_ARG;
  if (r > kMaxR) return SPX_ERR_TOO_LARGE;
  const int64_t total = (int64_t)batch * r * gmax;
  if (total >= (int64_t(1) << 31)) return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < spx_proposal_sample_ws_bytes(batch, r, gmax)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  float* iou = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(k_pair_iou, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, s, rois, roi_labels, gt_boxes, total,
                     r, roi_stride, gmax, gt_stride, by_class, iou);
  hipLaunchKernelGGL(k_sample, dim3((unsigned)batch), dim3(kThreads), 0, s, iou, roi_labels, gt_boxes, r, gmax, gt_stride,
                     m, fg_per_image, reg_fg_thresh, cls_fg_thresh, cls_bg_thresh_lo, hard_bg_ratio, by_class, fg_keys,
                     slot_u, sampled_inds, roi_ious, gt_inds);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
