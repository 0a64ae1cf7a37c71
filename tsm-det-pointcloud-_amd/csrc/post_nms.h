// post_nms.h — what the two post-processing files share (post_process.hip §15, dense_post_process.hip §29): the 64-bit
// candidate keys and the LDS bitonic sort (score_keys.h), the single-workgroup greedy NMS over a sorted list and the
// per-frame output kernel.  Boxes are read by a row stride `ld` (>= 7 floats).
#pragma once
#include "box_iou.h"
#include "score_keys.h"

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

__device__ __forceinline__ int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
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
__device__ void greedy_nms(const float* __restrict__ fb, int ld, NmsLds& s, int m, float thresh) {
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
      s.cbox[e] = fb[(int64_t)row_of(s.keys[base + e / 7]) * ld + e % 7];
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
        const float* src = fb + (int64_t)row_of(s.keys[j]) * ld;
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

// grid (b): the classes' survivors -> final order, one more NMS (final_nms) -> the padded outputs
template <bool NORMAL>
__global__ __launch_bounds__(kThreads) void k_frame_out(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                        const float* __restrict__ boxes, int ld, int n, int n_thresh,
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
      greedy_nms<NORMAL>(boxes + row0 * ld, ld, s, m, nms_thresh);
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
      for (int q = 0; q < 7; ++q) out_boxes[o * 7 + q] = boxes[row * ld + q];
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

}  // namespace
