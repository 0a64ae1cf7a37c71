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
#include "box_iou.h"

namespace {

constexpr int kMaxN = 4096;       // candidates per frame: the keys of one frame fit a 32 KiB LDS array
constexpr int kThreads = 1024;
constexpr int kMaxThresh = 8;

struct Thresh {
  float v[kMaxThresh];
};

struct NmsLds {
  unsigned long long keys[kMaxN];
  unsigned long long remv[64];    // bit j of word w: sorted position 64 w + j is suppressed (or, past a chunk, not kept)
  unsigned long long diag[64];
  float cbox[64 * 7];
  int wpre[65];
  int cnt;
};

// float -> uint32 whose unsigned order is the float order (-0 counts as +0, as in a float comparison)
__device__ __forceinline__ uint32_t ordered_bits(float s) {
  uint32_t u = __float_as_uint(s + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// key of a member row: never 0, so 0 pads the sort
__device__ __forceinline__ unsigned long long make_key(float score, int row) {
  return ((unsigned long long)ordered_bits(score) << 32) | (unsigned long long)(~(uint32_t)row);
}

__device__ __forceinline__ int row_of(unsigned long long key) { return (int)(~(uint32_t)key); }

__device__ __forceinline__ int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

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

template <bool NORMAL>
__device__ __forceinline__ bool suppresses(const float* earlier, const float* later, float thresh) {
  const float v = NORMAL ? iou_normal(earlier, later) : iou_bev(earlier, later);
  return v > thresh;
}

// Greedy NMS over the sorted positions [0, m) of s.keys (rows of the frame whose boxes start at fb).  On return
// (after a barrier) bit j of ~s.remv[w] says that position 64 w + j is kept (bits at or past m in the last word are set
// too: mask them).
template <bool NORMAL>
__device__ void greedy_nms(const float* __restrict__ fb, NmsLds& s, int m, float thresh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = blockDim.x >> 6;
  for (int w = t; w < 64; w += blockDim.x) s.remv[w] = 0ull;
  __syncthreads();
  const int nchunks = (m + 63) >> 6;
  for (int c = 0; c < nchunks; ++c) {
    const int base = c << 6;
    const int size = min(64, m - base);
    unsigned long long alive = ~s.remv[c];
    if (size < 64) alive &= (1ull << size) - 1ull;
    for (int e = t; e < size * 7; e += blockDim.x)
      s.cbox[e] = fb[(int64_t)row_of(s.keys[base + e / 7]) * 7 + e % 7];
    __syncthreads();
    // the chunk's own tile: row i (one wave each), column = lane; only pairs of live boxes
    for (int i = wave; i < size; i += nw) {
      bool hit = false;
      if (lane > i && lane < size && ((alive >> i) & 1ull) && ((alive >> lane) & 1ull))
        hit = suppresses<NORMAL>(s.cbox + i * 7, s.cbox + lane * 7, thresh);
      const unsigned long long row_mask = __ballot(hit);
      if (lane == 0) s.diag[i] = row_mask;
    }
    __syncthreads();
    unsigned long long kept = 0ull;      // the same in every thread
    for (int i = 0; i < size; ++i)
      if ((alive >> i) & 1ull) {
        kept |= 1ull << i;
        alive &= ~s.diag[i];
      }
    if (t == 0) s.remv[c] = ~kept;
    // later boxes against the chunk's kept ones; a wave owns 64 consecutive positions = one word of remv
    for (int jb = base + 64 + (wave << 6); jb < m; jb += blockDim.x) {
      const int j = jb + lane;
      bool hit = false;
      if (j < m && !((s.remv[jb >> 6] >> lane) & 1ull)) {
        float me[7];
        const float* src = fb + (int64_t)row_of(s.keys[j]) * 7;
#pragma unroll
        for (int q = 0; q < 7; ++q) me[q] = src[q];
        unsigned long long kk = kept;
        while (kk) {
          const int i = __ffsll(kk) - 1;
          kk &= kk - 1ull;
          if (suppresses<NORMAL>(s.cbox + i * 7, me, thresh)) {
            hit = true;
            break;
          }
        }
      }
      const unsigned long long word = __ballot(hit);
      if (lane == 0 && word) s.remv[jb >> 6] |= word;
    }
    __syncthreads();
  }
}

// ranks of the kept positions: s.wpre[w] = kept positions before word w; returns the total (after a barrier)
__device__ int kept_prefix(NmsLds& s, int m) {
  const int nchunks = (m + 63) >> 6;
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int w = 0; w < nchunks; ++w) {
      s.wpre[w] = acc;
      unsigned long long k = ~s.remv[w];
      const int size = min(64, m - (w << 6));
      if (size < 64) k &= (1ull << size) - 1ull;
      acc += __popcll(k);
    }
    s.wpre[nchunks] = acc;
  }
  __syncthreads();
  return s.wpre[nchunks];
}

// rank of kept position j among the kept ones, or -1
__device__ __forceinline__ int kept_rank(const NmsLds& s, int j) {
  const unsigned long long k = ~s.remv[j >> 6];
  if (!((k >> (j & 63)) & 1ull)) return -1;
  return s.wpre[j >> 6] + __popcll(k & ((1ull << (j & 63)) - 1ull));
}

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
  greedy_nms<NORMAL>(boxes + row0 * 7, s, m, nms_thresh);
  const int total = kept_prefix(s, m);
  for (int j = t; j < m; j += blockDim.x) {
    const int rank = kept_rank(s, j);
    if (rank >= 0 && rank < post_cap) surv[(int64_t)slot * post_cap + rank] = s.keys[j];
  }
  if (t == 0) scnt[slot] = min(total, post_cap);
}

// grid (b): the classes' survivors -> final order, one more NMS (final_nms) -> the padded outputs
template <bool NORMAL>
__global__ __launch_bounds__(kThreads) void k_frame_out(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                        const float* __restrict__ boxes, int n, int n_thresh,
                                                        float nms_thresh, int post_cap, int final_nms,
                                                        const unsigned long long* __restrict__ surv,
                                                        const int32_t* __restrict__ scnt, int cap, int64_t* __restrict__ sel,
                                                        int32_t* __restrict__ count, float* __restrict__ out_boxes,
                                                        float* __restrict__ out_scores, int64_t* __restrict__ out_labels) {
  __shared__ NmsLds s;
  __shared__ int coff[kMaxThresh + 1];
  const int t = threadIdx.x, b = blockIdx.x;
  const int64_t row0 = (int64_t)b * n;
  if (t == 0) {
    int acc = 0;
    for (int c = 0; c < n_thresh; ++c) {
      coff[c] = acc;
      acc += scnt[b * n_thresh + c];
    }
    coff[n_thresh] = acc;
  }
  __syncthreads();
  const int m = min(coff[n_thresh], kMaxN);   // <= n: the classes' rows are disjoint
  for (int c = 0; c < n_thresh; ++c) {
    const int len = coff[c + 1] - coff[c];
    for (int i = t; i < len && coff[c] + i < m; i += blockDim.x)
      s.keys[coff[c] + i] = surv[(int64_t)(b * n_thresh + c) * post_cap + i];
  }
  int total = 0;
  if (m > 0) {
    if (final_nms) {
      const int p = pow2_at_least(m);
      for (int i = m + t; i < p; i += blockDim.x) s.keys[i] = 0ull;
      __syncthreads();
      sort_desc(s.keys, p);
      greedy_nms<NORMAL>(boxes + row0 * 7, s, m, nms_thresh);
    } else {
      for (int w = t; w < 64; w += blockDim.x) s.remv[w] = 0ull;
      __syncthreads();
    }
    total = min(kept_prefix(s, m), cap);
    for (int j = t; j < m; j += blockDim.x) {
      const int rank = kept_rank(s, j);
      if (rank < 0 || rank >= cap) continue;
      const int64_t row = row0 + row_of(s.keys[j]), o = (int64_t)b * cap + rank;
      sel[o] = row;
#pragma unroll
      for (int q = 0; q < 7; ++q) out_boxes[o * 7 + q] = boxes[row * 7 + q];
      out_scores[o] = scores[row];
      out_labels[o] = (int64_t)labels[row];
    }
  }
  for (int r = total + t; r < cap; r += blockDim.x) {
    const int64_t o = (int64_t)b * cap + r;
    sel[o] = -1;
#pragma unroll
    for (int q = 0; q < 7; ++q) out_boxes[o * 7 + q] = 0.f;
    out_scores[o] = 0.f;
    out_labels[o] = 0;
  }
  if (t == 0) count[b] = total;
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
    hipLaunchKernelGGL((k_frame_out<true>), g2, blk, 0, s, scores, labels, boxes, (int)n, (int)n_thresh, nms_thresh,
                       post_cap, pc, surv, scnt, cap, sel, count, out_boxes, out_scores, out_labels);
  } else {
    hipLaunchKernelGGL((k_class_nms<false>), g1, blk, 0, s, scores, labels, boxes, (int)n, th, pc, nms_thresh, pre, post_cap,
                       surv, scnt);
    hipLaunchKernelGGL((k_frame_out<false>), g2, blk, 0, s, scores, labels, boxes, (int)n, (int)n_thresh, nms_thresh,
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
