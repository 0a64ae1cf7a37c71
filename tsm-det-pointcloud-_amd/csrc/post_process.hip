// post_process.hip — batched post-processing of a point head's predictions with no host read (include/spx.h §15):
// score threshold, ordering, pre-max, greedy rotated-BEV NMS, post-max for every frame (and class) of a batch in two
// launches, into outputs of static capacity with the live count on the device; and the recall record of the kept boxes
// against the ground truth.  Replaces the per-frame, per-class mask / nonzero / topk / NMS / .item() chain of
// Detector3DTemplate.post_processing + model_nms_utils.multi_thresh (reference detector3d_template.py:207-349,
// model_nms_utils.py) and generate_recall_record (:501-542).
//
// Launch 1, one workgroup per (frame, class): the members' 64-bit keys (score as an ordered uint, ~row) are compacted
//   into LDS, sorted descending by a bitonic network (equal scores: lower row first), cut at pre_max, reduced by the
//   greedy NMS below, cut at post_max; the survivors' keys go to the workspace.
// Launch 2, one workgroup per frame: the survivors of all classes are sorted again, reduced by one more NMS and written
//   out with the padding.  In agnostic mode launch 1 has one "class" and launch 2 only writes.
//
// Greedy NMS over a sorted list, 64 boxes per step, no n x n mask: the chunk's 64 x 64 tile of pair tests among the
// boxes still alive is taken by ballots (one wave per row), every thread resolves the chunk's greedy order from the 64
// row masks, and each later live box is then tested against the chunk's kept boxes until the first one suppresses it.
// The pair test is box_iou.h's, with (earlier, later) argument order, as in nms.hip.
#include "post_nms.h"

namespace {

// grid (b, n_thresh): members of one class of one frame -> up to post_cap survivor keys in score order
template <bool NORMAL>
__global__ __launch_bounds__(kThreads) void k_class_nms(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                        const float* __restrict__ boxes, int n, Thresh th, int per_class,
                                                        float nms_thresh, int pre_max, int post_cap,
                                                        unsigned long long* __restrict__ surv, int32_t* __restrict__ scnt) {
  __shared__ NmsLds s;
  const int t = threadIdx.x, b = blockIdx.x, c = blockIdx.y, slot = b * gridDim.y + c;
  const int64_t row0 = (int64_t)b * n;
  if (t == 0) s.cnt = 0;
  __syncthreads();
  const float thr = th.v[c];
  for (int r = t; r < n; r += blockDim.x) {
    const float sc = scores[row0 + r];
    if (sc >= thr && (!per_class || labels[row0 + r] == c + 1)) s.keys[atomicAdd(&s.cnt, 1)] = make_key(sc, r);
  }
  __syncthreads();
  const int cnt = s.cnt;
  if (cnt == 0) {
    if (t == 0) scnt[slot] = 0;
    return;
  }
  const int p = pow2_at_least(cnt);
  for (int i = cnt + t; i < p; i += blockDim.x) s.keys[i] = 0ull;
  __syncthreads();
  sort_desc(s.keys, p);
  const int m = min(cnt, pre_max);
  greedy_nms<NORMAL>(boxes + row0 * 7, 7, s, m, nms_thresh);
  const int total = kept_prefix(s, m);
  for (int j = t; j < m; j += blockDim.x) {
    const int rank = kept_rank(s, j);
    if (rank >= 0 && rank < post_cap) surv[(int64_t)slot * post_cap + rank] = s.keys[j];
  }
  if (t == 0) scnt[slot] = min(total, post_cap);
}

// 3-D IoU with the roundings of iou3d_nms_utils.boxes_iou3d_gpu (every product and sum rounded on its own, as the
// tensor expression does): BEV overlap x height overlap / max(vol_a + vol_b - overlap, 1e-6)
__device__ float iou_3d(const float* a, const float* b) {
  const float a_max = a[2] + a[5] / 2, a_min = a[2] - a[5] / 2;      // x / 2 is exact: contraction cannot change these
  const float b_max = b[2] + b[5] / 2, b_min = b[2] - b[5] / 2;
  const float overlap_bev = overlap_area(a, b);
  const float overlap_h = fmaxf(__fsub_rn(fminf(a_max, b_max), fmaxf(a_min, b_min)), 0.f);
  const float overlap_3d = __fmul_rn(overlap_bev, overlap_h);
  const float vol_a = __fmul_rn(__fmul_rn(a[3], a[4]), a[5]), vol_b = __fmul_rn(__fmul_rn(b[3], b[4]), b[5]);
  return __fdiv_rn(overlap_3d, fmaxf(__fsub_rn(__fadd_rn(vol_a, vol_b), overlap_3d), 1e-6f));
}

// grid (b), one wave per gt box, lanes over the frame's kept boxes
__global__ __launch_bounds__(kThreads) void k_recall(const float* __restrict__ out_boxes, const int32_t* __restrict__ count,
                                                     int cap, const float* __restrict__ gt, int g, int gt_ld, Thresh th,
                                                     int n_thresh, int32_t* __restrict__ recalled,
                                                     int32_t* __restrict__ num_gt) {
  __shared__ int s_last;
  __shared__ int s_rec[kMaxThresh];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6, b = blockIdx.x;
  const float* fgt = gt + (int64_t)b * g * gt_ld;
  if (t == 0) {
    int k = g - 1;
    while (k > 0) {      // trailing rows that sum to 0 are padding; row 0 always counts
      float sum = 0.f;
      for (int q = 0; q < gt_ld; ++q) sum += fgt[(int64_t)k * gt_ld + q];
      if (sum != 0.f) break;
      --k;
    }
    s_last = k;
  }
  if (t < kMaxThresh) s_rec[t] = 0;
  __syncthreads();
  const int ng = g > 0 ? s_last + 1 : 0;
  const int live = min(max(count[b], 0), cap);
  const float* fb = out_boxes + (int64_t)b * cap * 7;
  for (int gi = wave; gi < ng && live > 0; gi += nw) {
    float gbox[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) gbox[q] = fgt[(int64_t)gi * gt_ld + q];
    float best = -INFINITY;
    bool nan = false;        // torch.max returns NaN when it meets one
    for (int i = lane; i < live; i += 64) {
      const float v = iou_3d(fb + (int64_t)i * 7, gbox);
      nan |= v != v;
      best = fmaxf(best, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
    const bool any_nan = __ballot(nan) != 0ull;
    if (lane < n_thresh && !any_nan && best > th.v[lane]) atomicAdd(&s_rec[lane], 1);
  }
  __syncthreads();
  if (t < n_thresh) recalled[b * n_thresh + t] = s_rec[t];
  if (t == 0) num_gt[b] = ng;
}

static inline int64_t out_cap(int64_t n, int32_t n_thresh, int64_t post_max, int per_class) {
  const int64_t lim = per_class ? (int64_t)n_thresh * (post_max < n ? post_max : n) : post_max;
  return lim < n ? lim : n;
}

}  // namespace

extern "C" int64_t spx_point_post_process_capacity(int64_t n, int32_t n_thresh, int64_t post_max, int per_class) {
  if (n < 0 || n_thresh < 1 || post_max < 1) return 0;
  return out_cap(n, n_thresh, post_max, per_class);
}

extern "C" size_t spx_point_post_process_ws_bytes(int32_t b, int64_t n, int32_t n_thresh, int64_t post_max) {
  if (b < 1 || n < 1 || n_thresh < 1 || post_max < 1) return spx_align(1);
  const int64_t post_cap = post_max < n ? post_max : n;
  return spx_align((size_t)b * n_thresh * post_cap * 8) + spx_align((size_t)b * n_thresh * 4);
}

extern "C" int spx_point_post_process(const float* scores, const int32_t* labels, const float* boxes, int32_t b, int64_t n,
                                      const float* thresholds, int32_t n_thresh, float nms_thresh, int64_t pre_max,
                                      int64_t post_max, int axis_aligned, int per_class, int64_t* sel, int32_t* count,
                                      float* out_boxes, float* out_scores, int64_t* out_labels, void* ws, size_t ws_bytes,
                                      spx_stream_t stream) {
  if (!scores || !labels || !boxes || !thresholds || !sel || !count || !out_boxes || !out_scores || !out_labels)
    return SPX_ERR_INVALID_ARG;
  if (b < 0 || n < 0 || n_thresh < 1 || pre_max < 1 || post_max < 1) return SPX_ERR_INVALID_ARG;
  if (!per_class && n_thresh != 1) return SPX_ERR_INVALID_ARG;
  if (n_thresh > kMaxThresh) return SPX_ERR_UNSUPPORTED;
  if (n > kMaxN) return SPX_ERR_TOO_LARGE;
  if (b == 0) return SPX_OK;
  hipStream_t s = spx_s(stream);
  if (n == 0) {     // capacity 0: only the counts exist
    spx_fill_async(count, 0, (size_t)b * sizeof(int32_t), s);
    SPX_CHECK_LAUNCH();
    return SPX_OK;
  }
  if (!ws || ws_bytes < spx_point_post_process_ws_bytes(b, n, n_thresh, post_max)) return SPX_ERR_WORKSPACE;
  const int post_cap = (int)(post_max < n ? post_max : n);
  const int pre = (int)(pre_max < n ? pre_max : n);
  const int cap = (int)out_cap(n, n_thresh, post_max, per_class);
  unsigned long long* surv = reinterpret_cast<unsigned long long*>(ws);
  int32_t* scnt = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + spx_align((size_t)b * n_thresh * post_cap * 8));
  Thresh th;
  for (int i = 0; i < kMaxThresh; ++i) th.v[i] = i < n_thresh ? thresholds[i] : 0.f;
  const dim3 g1((unsigned)b, (unsigned)n_thresh), g2((unsigned)b), blk(kThreads);
  const int pc = per_class ? 1 : 0;
  if (axis_aligned) {
    hipLaunchKernelGGL((k_class_nms<true>), g1, blk, 0, s, scores, labels, boxes, (int)n, th, pc, nms_thresh, pre, post_cap,
                       surv, scnt);
    hipLaunchKernelGGL((k_frame_out<true>), g2, blk, 0, s, scores, labels, boxes, 7, (int)n, (int)n_thresh, nms_thresh,
                       post_cap, pc, surv, scnt, cap, sel, count, out_boxes, out_scores, out_labels);
  } else {
    hipLaunchKernelGGL((k_class_nms<false>), g1, blk, 0, s, scores, labels, boxes, (int)n, th, pc, nms_thresh, pre, post_cap,
                       surv, scnt);
    hipLaunchKernelGGL((k_frame_out<false>), g2, blk, 0, s, scores, labels, boxes, 7, (int)n, (int)n_thresh, nms_thresh,
                       post_cap, pc, surv, scnt, cap, sel, count, out_boxes, out_scores, out_labels);
  }
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_recall_count(const float* out_boxes, const int32_t* count, int32_t b, int64_t cap, const float* gt_boxes,
                                int64_t g, int32_t gt_ld, const float* thresholds, int32_t n_thresh, int32_t* recalled,
                                int32_t* num_gt, spx_stream_t stream) {
  if (!count || !thresholds || !recalled || !num_gt || (!out_boxes && cap > 0) || (!gt_boxes && g > 0))
    return SPX_ERR_INVALID_ARG;
  if (b < 0 || cap < 0 || g < 0 || gt_ld < 7 || n_thresh < 1) return SPX_ERR_INVALID_ARG;
  if (n_thresh > kMaxThresh) return SPX_ERR_UNSUPPORTED;
  if (cap > kMaxN * (int64_t)kMaxThresh || g >= (int64_t(1) << 24)) return SPX_ERR_TOO_LARGE;
  if (b == 0) return SPX_OK;
  Thresh th;
  for (int i = 0; i < kMaxThresh; ++i) th.v[i] = i < n_thresh ? thresholds[i] : 0.f;
  hipLaunchKernelGGL(k_recall, dim3((unsigned)b), dim3(kThreads), 0, spx_s(stream), out_boxes, count, (int)cap, gt_boxes,
                     (int)g, (int)gt_ld, th, (int)n_thresh, recalled, num_gt);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
