// center_decode.hip — the K best heatmap cells of every frame of a centre head, decoded to boxes with the centre-range
// and score masks, with no host read and no float atomics (include/spx.h §21).  Replaces, for one head and the whole
// batch, the eager chain of CenterHead.generate_predicted_boxes / centernet_utils.decode_bbox_from_heatmap (reference
// pcdet/models/dense_heads/center_head.py:288-321, pcdet/models/model_utils/centernet_utils.py:118-216): a sigmoid and
// an exp over full maps, torch.topk per class and over C x K, six permute + gather passes and the masks.
//
// Selection is a tournament over 64-bit keys (value as an ordered uint, ~flat index): the keys are pairwise distinct,
// "value descending, lower flat index first" is their plain descending order, and the K largest of a frame lie in the
// union of the K largest of its parts.  One kernel does every round: a workgroup of 1024 threads holds up to 8192 keys
// in registers (8 per thread), finds the K-th largest by a radix select over 11-bit digits (LDS histogram, integer
// atomics; it stops as soon as the digit's bin is taken whole, after three digits when the values are distinct) and
// compacts the K keys at or above it.
//   round 0: ceil(C H W / 8192) workgroups per frame read the heatmap and write K keys each to the workspace;
//   middle rounds (only when more than floor(8192 / K) lists are left): each workgroup merges floor(8192 / K) lists;
//   last round, one workgroup per frame: merges the remaining lists, sorts the K keys in LDS (bitonic), gathers the
//     regression maps at the selected cells, decodes and writes every output row, and counts the kept rows.
// LAUNCHES: 1 when C H W <= 8192; 2 when ceil(C H W / 8192) <= floor(8192 / K) — both yamls (3 x 200 x 176 and
// 3 x 188 x 188 give 13 lists, K = 500 merges 16); 3 for upstream Waymo's 3 x 468 x 468 (81 lists -> 6 -> 1).
// The order in which the LDS atomics append to a list varies between runs; a list is only ever read as a set, and the
// final order comes from the sort of distinct keys, so the outputs are bit-identical from call to call.
// Gather indices are the positions the keys were built from (< C H W) whatever bits the heatmap holds (NaN, inf).
#include "spx_common.h"

#pragma clang fp contract(off)

#include "score_keys.h"   // make_key, row_of (here: the flat heatmap index), sort_desc

namespace {

constexpr int kThreads = 1024;
constexpr int kPer = 8;                      // keys per thread
constexpr int kSlice = kThreads * kPer;      // keys per workgroup
constexpr int kBins = 2048;                  // 11-bit digits; 64 lanes x 32 bins in the scan
constexpr int kMaxK = 1024;

struct DecodeArgs {
  const float* hm;
  const float* center;
  const float* center_z;
  const float* dim;
  const float* rot;
  const float* vel;     // nullable
  int c, h, w, k;
  int n;                // c * h * w
  float stride, vs0, vs1, x0, y0;
  float lim[6];
  float score_thresh;
  int has_thresh, raw;
  float* boxes;
  float* scores;
  int32_t* labels;
  int64_t* cells;
  uint8_t* keep;
  int32_t* count;
};

struct SelLds {
  unsigned long long list[kMaxK];
  int hist[kBins];
  int n_valid, cnt, sel_bin, sel_rem, sel_cnt, kept;
};

// hist[bin] += 1 for every lane with `on`.  Heatmap values crowd into a few bins of the leading digits, where one
// atomic per lane would serialise on one address: the bins of the first two leading lanes are added once per wave.
__device__ __forceinline__ void hist_add(int* hist, int bin, bool on) {
  const int lane = threadIdx.x & 63;
  unsigned long long rem = __ballot(on);
  for (int it = 0; it < 2 && rem; ++it) {
    const int leader = __ffsll(rem) - 1;
    const int lb = __shfl(bin, leader, 64);
    const unsigned long long same = __ballot(on && bin == lb);
    if (lane == leader) atomicAdd(&hist[lb], __popcll(same));
    if (bin == lb) on = false;
    rem &= ~same;
  }
  if (on) atomicAdd(&hist[bin], 1);
}

// The min(k_top, live) largest of the workgroup's keys (0 = empty place) -> s.list[0, returned count), in no
// particular order.  Called by all threads.
__device__ int select_top(const unsigned long long (&key)[kPer], int k_top, SelLds& s) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int nv = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) nv += key[e] != 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off, 64);
  if (t == 0) {
    s.n_valid = 0;
    s.cnt = 0;
  }
  __syncthreads();
  if (lane == 0) atomicAdd(&s.n_valid, nv);
  __syncthreads();
  unsigned long long lo = 1ull;      // keys >= lo are taken
  if (s.n_valid > k_top) {
    unsigned long long prefix = 0ull;   // the digits fixed so far = key >> hi_shift of the K-th largest key
    int hi_shift = 64, r = k_top;       // r: how many keys are still to take among those that match the prefix
    for (int shift = 53;;) {
      const int width = hi_shift - shift;
      const unsigned mask = (1u << width) - 1u;
      for (int i = t; i < kBins; i += kThreads) s.hist[i] = 0;
      __syncthreads();
#pragma unroll
      for (int e = 0; e < kPer; ++e) {
        const bool on = key[e] != 0ull && (hi_shift == 64 || (key[e] >> hi_shift) == prefix);
        hist_add(s.hist, (int)((unsigned)(key[e] >> shift) & mask), on);
      }
      __syncthreads();
      if (wave == 0) {                  // lane 0 owns the 32 highest bins
        const int base = (63 - lane) * 32;
        int sum = 0;
        for (int j = 0; j < 32; ++j) sum += s.hist[base + j];
        int inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int v = __shfl_up(inc, off, 64);
          if (lane >= off) inc += v;
        }
        const int exc = inc - sum;
        if (exc < r && inc >= r) {      // exactly one lane: the matching keys number more than r >= 1
          int need = r - exc;
          for (int j = 31; j >= 0; --j) {
            const int c = s.hist[base + j];
            if (c >= need) {
              s.sel_bin = base + j;
              s.sel_rem = need;
              s.sel_cnt = c;
              break;
            }
            need -= c;
          }
        }
      }
      __syncthreads();
      prefix = (prefix << width) | (unsigned long long)s.sel_bin;
      r = s.sel_rem;
      hi_shift = shift;
      if (s.sel_cnt == r || shift == 0) break;    // the bin is taken whole (distinct keys: always at shift 0)
      shift = shift >= 11 ? shift - 11 : 0;
    }
    lo = prefix << hi_shift;
  }
#pragma unroll
  for (int e = 0; e < kPer; ++e)
    if (key[e] != 0ull && key[e] >= lo) {
      const int pos = atomicAdd(&s.cnt, 1);
      if (pos < kMaxK) s.list[pos] = key[e];
    }
  __syncthreads();
  return min(s.cnt, k_top);
}

// One output row from one selected key (or, without one, a row of zeros that is not kept).
__device__ __forceinline__ bool decode_row(const DecodeArgs& a, int f, int j, bool have, unsigned long long key) {
  const int64_t o = (int64_t)f * a.k + j;
  const int ncol = a.vel ? 9 : 7;
  float* box = a.boxes + o * ncol;
  if (!have) {
    for (int q = 0; q < ncol; ++q) box[q] = 0.f;
    a.scores[o] = 0.f;
    a.labels[o] = 0;
    a.cells[o] = 0;
    a.keep[o] = 0;
    return false;
  }
  const int hw = a.h * a.w;
  const int idx = row_of(key);                  // < n by construction
  const int cls = idx / hw, cell = idx - cls * hw;
  const int y = cell / a.w, x = cell - y * a.w;
  const float v = a.hm[(int64_t)f * a.n + idx];
  const int64_t r2 = (int64_t)f * 2 * hw + cell;      // the cell in a two-channel map
  const float cx = a.center[r2], cy = a.center[r2 + hw];
  const float xs = ((float)x + cx) * a.stride * a.vs0 + a.x0;
  const float ys = ((float)y + cy) * a.stride * a.vs1 + a.y0;
  const float z = a.center_z[(int64_t)f * hw + cell];
  const int64_t d3 = (int64_t)f * 3 * hw + cell;
  float d0 = a.dim[d3], d1 = a.dim[d3 + hw], d2 = a.dim[d3 + 2 * hw];
  float score = v;
  if (a.raw) {
    d0 = expf(d0);
    d1 = expf(d1);
    d2 = expf(d2);
    score = 1.f / (1.f + expf(-v));
  }
  const float angle = atan2f(a.rot[r2 + hw], a.rot[r2]);
  box[0] = xs;
  box[1] = ys;
  box[2] = z;
  box[3] = d0;
  box[4] = d1;
  box[5] = d2;
  box[6] = angle;
  if (a.vel) {
    box[7] = a.vel[r2];
    box[8] = a.vel[r2 + hw];
  }
  bool keep = xs >= a.lim[0] && ys >= a.lim[1] && z >= a.lim[2] && xs <= a.lim[3] && ys <= a.lim[4] && z <= a.lim[5];
  if (a.has_thresh) keep = keep && score > a.score_thresh;
  a.scores[o] = score;
  a.labels[o] = cls;
  a.cells[o] = cell;
  a.keep[o] = keep ? 1 : 0;
  return keep;
}

// grid (groups, b).  FIRST: group g reads heatmap elements [g * 8192, (g + 1) * 8192) of its frame; otherwise lists
// [g * fan, (g + 1) * fan) of the n_in lists of src, k keys each (0 = empty).  LAST (one group per frame): sort, decode,
// write the outputs; otherwise the group's list goes to dst[(frame * gridDim.x + g) * k ...], padded with 0.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kThreads) void k_center_select(const DecodeArgs a, const unsigned long long* __restrict__ src,
                                                            int n_in, int fan, unsigned long long* __restrict__ dst) {
  __shared__ SelLds s;
  const int t = threadIdx.x, g = blockIdx.x, f = blockIdx.y;
  unsigned long long key[kPer];
  if (FIRST) {
    const float* fh = a.hm + (int64_t)f * a.n;
    const int64_t base = (int64_t)g * kSlice;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int64_t i = base + e * kThreads + t;
      key[e] = i < a.n ? make_key(fh[i], (int)i) : 0ull;
    }
  } else {
    const int first = g * fan;
    const int total = (min(first + fan, n_in) - first) * a.k;      // <= fan * k <= 8192
    const unsigned long long* fs = src + ((int64_t)f * n_in + first) * a.k;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int i = e * kThreads + t;
      key[e] = i < total ? fs[i] : 0ull;
    }
  }
  const int cnt = select_top(key, a.k, s);
  if (!LAST) {
    unsigned long long* out = dst + ((int64_t)f * gridDim.x + g) * a.k;
    for (int j = t; j < a.k; j += kThreads) out[j] = j < cnt ? s.list[j] : 0ull;
    return;
  }
  int p = 1;
  while (p < cnt) p <<= 1;
  for (int i = cnt + t; i < p; i += kThreads) s.list[i] = 0ull;
  if (t == 0) s.kept = 0;
  __syncthreads();
  sort_desc(s.list, p);
  int kept = 0;
  for (int j = t; j < a.k; j += kThreads) kept += decode_row(a, f, j, j < cnt, j < cnt ? s.list[j] : 0ull) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
  if ((t & 63) == 0 && kept) atomicAdd(&s.kept, kept);
  __syncthreads();
  if (t == 0) a.count[f] = s.kept;
}

inline int64_t n_first(int64_t n) { return (n + kSlice - 1) / kSlice; }

}  // namespace

extern "C" size_t spx_center_decode_ws_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t k) {
  if (b < 1 || c < 1 || h < 1 || w < 1 || k < 1 || k > kMaxK) return spx_align(1);
  const int64_t n = (int64_t)c * h * w, fan = kSlice / k;
  int64_t lists = 0, cur = n_first(n);
  if (cur > 1) {
    lists = cur;
    while (cur > fan) {
      cur = (cur + fan - 1) / fan;
      lists += cur;
    }
  }
  return spx_align((size_t)(lists * b * k * 8 + 1));
}

extern "C" int spx_center_decode(const float* hm, const float* center, const float* center_z, const float* dim,
                                 const float* rot, const float* vel, int32_t b, int32_t c, int32_t h, int32_t w,
                                 int32_t k, float feature_map_stride, const float* voxel_size2, const float* range_lo2,
                                 const float* post_center_limit_range6, float score_thresh, int has_score_thresh, int raw,
                                 float* boxes, float* scores, int32_t* labels, int64_t* cells, uint8_t* keep,
                                 int32_t* count, void* ws, size_t ws_bytes, spx_stream_t stream) {
  if (!hm || !center || !center_z || !dim || !rot || !voxel_size2 || !range_lo2 || !post_center_limit_range6 || !boxes ||
      !scores || !labels || !cells || !keep || !count)
    return SPX_ERR_INVALID_ARG;
  if (b < 0 || c < 1 || h < 1 || w < 1 || k < 1 || (int64_t)k > (int64_t)h * w) return SPX_ERR_INVALID_ARG;
  if (k > kMaxK) return SPX_ERR_TOO_LARGE;
  const int64_t n = (int64_t)c * h * w;
  if (n >= ((int64_t)1 << 31) || b > 65535) return SPX_ERR_TOO_LARGE;
  if (b == 0) return SPX_OK;
  if (!ws || ws_bytes < spx_center_decode_ws_bytes(b, c, h, w, k)) return SPX_ERR_WORKSPACE;
  DecodeArgs a;
  a.hm = hm;
  a.center = center;
  a.center_z = center_z;
  a.dim = dim;
  a.rot = rot;
  a.vel = vel;
  a.c = c;
  a.h = h;
  a.w = w;
  a.k = k;
  a.n = (int)n;
  a.stride = feature_map_stride;
  a.vs0 = voxel_size2[0];
  a.vs1 = voxel_size2[1];
  a.x0 = range_lo2[0];
  a.y0 = range_lo2[1];
  for (int i = 0; i < 6; ++i) a.lim[i] = post_center_limit_range6[i];
  a.score_thresh = score_thresh;
  a.has_thresh = has_score_thresh ? 1 : 0;
  a.raw = raw ? 1 : 0;
  a.boxes = boxes;
  a.scores = scores;
  a.labels = labels;
  a.cells = cells;
  a.keep = keep;
  a.count = count;
  hipStream_t s = spx_s(stream);
  const dim3 blk(kThreads);
  const int fan = kSlice / k;
  int cur = (int)n_first(n);
  if (cur == 1) {
    hipLaunchKernelGGL((k_center_select<true, true>), dim3(1, (unsigned)b), blk, 0, s, a, nullptr, 0, 0, nullptr);
    SPX_CHECK_LAUNCH();
    return SPX_OK;
  }
  unsigned long long* lists = reinterpret_cast<unsigned long long*>(ws);
  hipLaunchKernelGGL((k_center_select<true, false>), dim3((unsigned)cur, (unsigned)b), blk, 0, s, a, nullptr, 0, 0, lists);
  SPX_CHECK_LAUNCH();
  while (cur > fan) {
    const int next = (cur + fan - 1) / fan;
    unsigned long long* out = lists + (int64_t)cur * b * k;
    hipLaunchKernelGGL((k_center_select<false, false>), dim3((unsigned)next, (unsigned)b), blk, 0, s, a, lists, cur, fan,
                       out);
    SPX_CHECK_LAUNCH();
    lists = out;
    cur = next;
  }
  hipLaunchKernelGGL((k_center_select<false, true>), dim3(1, (unsigned)b), blk, 0, s, a, lists, cur, fan, nullptr);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
