// dense_post_process.hip — threshold + top-K + NMS over dense (B, N, .) predictions with no host read (include/spx.h
// §29): the anchors of AnchorHeadSingle (2e5 .. 3e5 per frame) and the proposal stage of the RoI heads.  Replaces the
// per-frame mask / nonzero / topk / NMS / count read of Detector3DTemplate.post_processing (reference
// detector3d_template.py:207-349, model_nms_utils.py) and the topk + per-frame NMS of RoIHeadTemplate.proposal_layer
// (reference roi_head_template.py:45-95) where n is beyond the 4096 rows of §15.
//
// Every stage is a launch of its own and the kernel boundary is the only hand-off between workgroups; the launch count
// depends on the arguments alone.  A (frame, class) pair is a SLOT; a row belongs to at most one slot.
//   select: an exact radix select over the slot's 64-bit keys (ordered score bits, then the row reversed, so keys are
//     unique and "equal scores lower row first" is the key order): per pass one histogram launch over all rows (LDS
//     histograms, integer atomics) and one scan launch per slot that fixes the next digit of the pre_max-th largest key;
//     then one compaction launch (key >= cut: exactly min(members, pre_max) rows, positions by an integer atomic, the
//     order is restored next) and one LDS bitonic sort per slot.
//   nms: the upper triangle of the slot's suppression bit matrix by the whole grid: up to 4096 workgroups of 256 threads
//     stride over the 64 x 64 tiles (the slot runs fastest in the tile index; only tiles below the slot's live count do
//     any work) and share a tile's live pairs among their threads; then one workgroup per slot walks the matrix
//     greedily 64 rows a step and stops at post_max kept boxes, so it loads at most post_max mask rows.
//   out: §15's per-frame kernel (post_nms.h): the classes' survivors sorted again, one more NMS, padded outputs.
#include <atomic>

#include "post_nms.h"
#include "spx_common.h"

namespace {

constexpr int kMaxPre = 16384;            // keys of one slot in LDS: 128 KiB
constexpr int kDigitBits = 11;
constexpr int kBins = 1 << kDigitBits;
constexpr int kHistThreads = 1024;
constexpr int kRowsPerBlock = 8192;       // rows of one frame a histogram / compaction workgroup reads
constexpr int kMaskBlocks = 4096;         // workgroups of the pair-test launch at most
constexpr int kMaxDevices = 64;
constexpr int kMaskThreads = 256;         // threads of a pair-test workgroup

struct SlotState {
  unsigned long long prefix;   // digits fixed so far; after the last pass the cut key (0: every member is taken)
  int32_t need;                // rank still looked for among the keys that share the prefix
  int32_t all;                 // the slot has fewer than pre members: all of them are taken
  int32_t total;               // members (set by the first scan)
  int32_t pos;                 // compaction cursor
};

struct Member {
  int c;
  unsigned long long key;
};

// the slot (class index) and select key of row r of its frame, or false where the row is no member of any slot
__device__ __forceinline__ bool member_of(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                          int64_t row, int r, const Thresh& th, int has_thresh, int per_class,
                                          int n_thresh, int rb, Member* out) {
  const float sc = scores[row];
  int c = 0;
  if (per_class) {
    c = labels[row] - 1;
    if (c < 0 || c >= n_thresh) return false;
  }
  if (!(sc == sc)) return false;                      // a NaN is never a member
  if (has_thresh) {
    float thr = th.v[0];
#pragma unroll
    for (int q = 1; q < kMaxThresh; ++q) thr = c == q ? th.v[q] : thr;
    if (!(sc >= thr)) return false;
  }
  const unsigned long long rmask = (1ull << rb) - 1ull;
  out->c = c;
  out->key = ((unsigned long long)ordered_bits(sc) << rb) | (rmask - (unsigned long long)r);
  return true;
}

// grid (ceil(n / kRowsPerBlock), b); dynamic LDS n_thresh * kBins ints.  Digit `bits` wide at `shift` of every member key
// that shares its slot's prefix -> hist [slot, kBins]
__global__ __launch_bounds__(kHistThreads) void k_hist(const float* __restrict__ scores, const int32_t* __restrict__ labels,
                                                       int n, Thresh th, int has_thresh, int per_class, int n_thresh,
                                                       int rb, int shift, int bits, const SlotState* __restrict__ st,
                                                       int32_t* __restrict__ hist) {
  extern __shared__ int32_t lh[];
  const int t = threadIdx.x, f = blockIdx.y;
  for (int i = t; i < n_thresh * kBins; i += blockDim.x) lh[i] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock;
  const int64_t r1 = min((int64_t)n, r0 + kRowsPerBlock);
  for (int64_t r = r0 + t; r < r1; r += blockDim.x) {
    Member m;
    if (!member_of(scores, labels, (int64_t)f * n + r, (int)r, th, has_thresh, per_class, n_thresh, rb, &m)) continue;
    const SlotState s = st[f * n_thresh + m.c];
    if (s.all || (m.key >> (shift + bits)) != s.prefix) continue;
    atomicAdd(&lh[m.c * kBins + (int)((m.key >> shift) & ((1ull << bits) - 1ull))], 1);
  }
  __syncthreads();
  for (int i = t; i < n_thresh * kBins; i += blockDim.x) {
    const int v = lh[i];
    if (v) atomicAdd(&hist[((int64_t)f * n_thresh + i / kBins) * kBins + i % kBins], v);
  }
}

// grid (slots), 256 threads: the digit of the need-th largest key among those that share the prefix
__global__ __launch_bounds__(256) void k_scan(const int32_t* __restrict__ hist, SlotState* __restrict__ st, int first,
                                              int pre, int bits) {
  __shared__ int32_t part[2][256];
  const int t = threadIdx.x, slot = blockIdx.x;
  SlotState s = st[slot];
  if (first) {
    s.prefix = 0ull;
    s.need = pre;
    s.all = 0;
    s.total = 0;
    s.pos = 0;
  }
  if (s.all) return;                                  // uniform over the workgroup
  const int32_t* h = hist + (int64_t)slot * kBins;
  constexpr int kPer = kBins / 256;
  // thread t owns the bins [hi - kPer + 1, hi], hi descending with t: sums from the top
  const int hi = kBins - 1 - t * kPer;
  int mine = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) mine += h[hi - q];
  part[0][t] = mine;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < 256; off <<= 1) {           // inclusive scan over t
    const int v = part[cur][t] + (t >= off ? part[cur][t - off] : 0);
    part[cur ^ 1][t] = v;
    cur ^= 1;
    __syncthreads();
  }
  const int incl = part[cur][t], excl = incl - mine, total = part[cur][255];
  if (first && total < s.need) {                      // fewer members than pre: take all of them (uniform)
    if (t == 0) {
      s.all = 1;
      s.total = total;
      st[slot] = s;
    }
    return;
  }
  if (excl < s.need && s.need <= incl) {              // exactly one thread (total >= need >= 1)
    int acc = excl, d = hi - kPer + 1;
    for (int q = 0; q < kPer; ++q) {
      const int v = h[hi - q];
      if (acc + v >= s.need) {
        d = hi - q;
        break;
      }
      acc += v;
    }
    s.prefix = (s.prefix << bits) | (unsigned long long)d;
    s.need -= acc;
    if (first) s.total = total;
    st[slot] = s;
  }
}

// grid as k_hist: member keys at or above the slot's cut -> cbuf [slot, pre], any order
__global__ __launch_bounds__(kHistThreads) void k_compact(const float* __restrict__ scores,
                                                          const int32_t* __restrict__ labels, int n, Thresh th,
                                                          int has_thresh, int per_class, int n_thresh, int rb, int pre,
                                                          SlotState* __restrict__ st,
                                                          unsigned long long* __restrict__ cbuf) {
  const int t = threadIdx.x, f = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock;
  const int64_t r1 = min((int64_t)n, r0 + kRowsPerBlock);
  for (int64_t r = r0 + t; r < r1; r += blockDim.x) {
    Member m;
    if (!member_of(scores, labels, (int64_t)f * n + r, (int)r, th, has_thresh, per_class, n_thresh, rb, &m)) continue;
    const int slot = f * n_thresh + m.c;
    const unsigned long long cut = st[slot].all ? 0ull : st[slot].prefix;
    if (m.key < cut) continue;
    const int p = atomicAdd(&st[slot].pos, 1);
    if (p < pre) cbuf[(int64_t)slot * pre + p] = m.key;
  }
}

// grid (slots), dynamic LDS p * 8 bytes (p = pre rounded up to a power of two): the slot's keys in order -> skeys
// [slot, pre] in §15's key format (0 past the count), scnt [slot], and, where asked for, cand [slot, cand_ld] rows of the
// batch (-1 past the count)
__global__ __launch_bounds__(kThreads) void k_sort(const SlotState* __restrict__ st,
                                                   const unsigned long long* __restrict__ cbuf, int n, int n_thresh,
                                                   int rb, int pre, int p, unsigned long long* __restrict__ skeys,
                                                   int32_t* __restrict__ scnt, int64_t* __restrict__ cand, int cand_ld) {
  extern __shared__ unsigned long long sk[];
  const int t = threadIdx.x, slot = blockIdx.x;
  const SlotState s = st[slot];
  const int cnt = max(0, min(min(s.all ? s.total : pre, s.pos), pre));
  p = min(p, pow2_at_least(cnt));                     // the launch reserves LDS for pre keys; few members sort faster
  for (int i = t; i < p; i += blockDim.x) sk[i] = i < cnt ? cbuf[(int64_t)slot * pre + i] : 0ull;
  __syncthreads();
  sort_desc(sk, p);
  const unsigned long long rmask = (1ull << rb) - 1ull;
  const int64_t row0 = (int64_t)(slot / n_thresh) * n;
  const int last = max(pre, cand ? cand_ld : 0);
  for (int i = t; i < last; i += blockDim.x) {
    int r = -1;
    unsigned long long key = 0ull;
    if (i < cnt) {
      const unsigned long long k = sk[i];
      r = (int)(rmask - (k & rmask));
      key = ((k >> rb) << 32) | (unsigned long long)(~(uint32_t)r);
    }
    if (i < pre) skeys[(int64_t)slot * pre + i] = key;
    if (cand && i < cand_ld) cand[(int64_t)slot * cand_ld + i] = r < 0 ? -1 : row0 + r;
  }
  if (t == 0) scnt[slot] = cnt;
}

// grid (up to kMaskBlocks), kMaskThreads threads: tile (rt, ct) of slot s, ct >= rt, both below the slot's live tiles: word ct
// of mask row i = 64 rt + r has bit j set where sorted box i suppresses the later box 64 ct + j.  The tile's live pairs
// are spread over the whole workgroup (a rotated pair test is long and latency bound: few live rows must not mean few
// busy lanes); a hit sets its bit by an integer OR in LDS.  mask [slot, pre, words].
template <bool NORMAL>
__global__ __launch_bounds__(kMaskThreads) void k_pair_mask(const float* __restrict__ boxes, int ld, int n, int n_thresh,
                                                        int slots, int pre, int words, float thresh,
                                                        const unsigned long long* __restrict__ skeys,
                                                        const int32_t* __restrict__ scnt,
                                                        unsigned long long* __restrict__ mask) {
  __shared__ float rbox[64 * 7];
  __shared__ float cbox[64 * 7];
  __shared__ unsigned long long bitsw[64];
  const int t = threadIdx.x;
  const int64_t tiles = (int64_t)slots * words * words;
  for (int64_t idx = blockIdx.x; idx < tiles; idx += gridDim.x) {
    const int s = (int)(idx % slots);                 // the slot runs fastest: a tile's slots go to different workgroups
    const int rem = (int)(idx / slots);
    const int rt = rem / words, ct = rem % words;
    const int m = max(0, min(scnt[s], pre));
    const int live = (m + 63) >> 6;
    if (ct < rt || ct >= live) continue;              // uniform over the workgroup
    const float* fb = boxes + (int64_t)(s / n_thresh) * n * ld;
    const unsigned long long* keys = skeys + (int64_t)s * pre;
    const int i0 = rt << 6, j0 = ct << 6;
    const int mr = min(64, m - i0), mc = min(64, m - j0);
    if (t < 64) {
      if (t < mr) {
        const float* src = fb + (int64_t)row_of(keys[i0 + t]) * ld;
#pragma unroll
        for (int q = 0; q < 7; ++q) rbox[t * 7 + q] = src[q];
      }
      bitsw[t] = 0ull;
    } else if (t < 128 && t - 64 < mc) {
      const float* src = fb + (int64_t)row_of(keys[j0 + t - 64]) * ld;
#pragma unroll
      for (int q = 0; q < 7; ++q) cbox[(t - 64) * 7 + q] = src[q];
    }
    __syncthreads();
    for (int p = t; p < mr * mc; p += blockDim.x) {
      const int i = p / mc, j = p - i * mc;
      if (j0 + j > i0 + i && suppresses<NORMAL>(rbox + i * 7, cbox + j * 7, thresh)) atomicOr(&bitsw[i], 1ull << j);
    }
    __syncthreads();
    if (t < mr) mask[((int64_t)s * pre + i0 + t) * words + ct] = bitsw[t];
    __syncthreads();
  }
}

// grid (slots), 256 threads: greedy walk over the bit matrix, 64 sorted positions a step, until post_cap boxes are kept
// -> surv [slot, post_cap] keys in order, kcnt [slot]
__global__ __launch_bounds__(256) void k_reduce(const unsigned long long* __restrict__ skeys,
                                                const int32_t* __restrict__ scnt,
                                                const unsigned long long* __restrict__ mask, int pre, int words,
                                                int post_cap, unsigned long long* __restrict__ surv,
                                                int32_t* __restrict__ kcnt) {
  __shared__ unsigned long long remv[kMaxPre / 64];
  __shared__ unsigned long long diag[64];
  const int t = threadIdx.x, slot = blockIdx.x;
  const int m = max(0, min(scnt[slot], pre));
  const int live = (m + 63) >> 6;
  const unsigned long long* keys = skeys + (int64_t)slot * pre;
  const unsigned long long* mk = mask + (int64_t)slot * pre * words;
  for (int w = t; w < live; w += blockDim.x) remv[w] = 0ull;
  __syncthreads();
  int total = 0;                                      // the same in every thread
  for (int c = 0; c < live && total < post_cap; ++c) {
    const int base = c << 6;
    const int size = min(64, m - base);
    if (t < size) diag[t] = mk[(int64_t)(base + t) * words + c];
    __syncthreads();
    unsigned long long alive = ~remv[c];
    if (size < 64) alive &= (1ull << size) - 1ull;
    unsigned long long kept = 0ull;
    int k = total;
    for (int i = 0; i < size && k < post_cap; ++i)
      if ((alive >> i) & 1ull) {
        kept |= 1ull << i;
        alive &= ~diag[i];
        ++k;
      }
    // the kept boxes in order go out; the words of later chunks take their mask rows
    if (t < size && ((kept >> t) & 1ull))
      surv[(int64_t)slot * post_cap + total + __popcll(kept & ((1ull << t) - 1ull))] = keys[base + t];
    total = k;
    if (total < post_cap)
      for (int w = c + 1 + t; w < live; w += blockDim.x) {
        unsigned long long acc = 0ull, kk = kept;
        while (kk) {
          const int i = __ffsll(kk) - 1;
          kk &= kk - 1ull;
          acc |= mk[(int64_t)(base + i) * words + w];
        }
        remv[w] |= acc;
      }
    __syncthreads();
  }
  if (t == 0) kcnt[slot] = total;
}

struct Plan {
  int rb, passes, pre, p, slots, words, post_cap;
  size_t off_state, off_hist, off_cbuf, off_skeys, off_scnt, off_mask, off_surv, off_kcnt, bytes;
};

int bits_for(int64_t n) {          // bits that hold every row 0 .. n - 1, at least 1
  int rb = 1;
  while (((int64_t)1 << rb) < n) ++rb;
  return rb;
}

Plan make_plan(int32_t b, int64_t n, int32_t n_thresh, int64_t pre_max, int64_t post_max, bool nms) {
  Plan pl;
  pl.rb = bits_for(n);
  pl.passes = (32 + pl.rb + kDigitBits - 1) / kDigitBits;
  pl.pre = (int)(pre_max < n ? pre_max : n);
  pl.p = 1;
  while (pl.p < pl.pre) pl.p <<= 1;
  pl.slots = b * n_thresh;
  pl.words = (pl.pre + 63) / 64;
  pl.post_cap = (int)(post_max < pl.pre ? post_max : pl.pre);
  size_t o = 0;
  pl.off_state = o, o += spx_align((size_t)pl.slots * sizeof(SlotState));
  pl.off_hist = o, o += spx_align((size_t)pl.passes * pl.slots * kBins * 4);
  pl.off_cbuf = o, o += spx_align((size_t)pl.slots * pl.pre * 8);
  pl.off_skeys = o, o += spx_align((size_t)pl.slots * pl.pre * 8);
  pl.off_scnt = o, o += spx_align((size_t)pl.slots * 4);
  pl.off_mask = pl.off_surv = pl.off_kcnt = o;
  if (nms) {
    pl.off_mask = o, o += spx_align((size_t)pl.slots * pl.pre * pl.words * 8);
    pl.off_surv = o, o += spx_align((size_t)pl.slots * pl.post_cap * 8);
    pl.off_kcnt = o, o += spx_align((size_t)pl.slots * 4);
  }
  pl.bytes = o;
  return pl;
}

int check_common(int32_t b, int64_t n, int32_t n_thresh, int64_t pre_max, int per_class) {
  if (b < 0 || n < 0 || n_thresh < 1 || pre_max < 1) return SPX_ERR_INVALID_ARG;
  if (!per_class && n_thresh != 1) return SPX_ERR_INVALID_ARG;
  if (n_thresh > kMaxThresh) return SPX_ERR_UNSUPPORTED;
  if (pre_max > kMaxPre || b > 65535 || (int64_t)b * n >= ((int64_t)1 << 31)) return SPX_ERR_TOO_LARGE;
  return SPX_OK;
}

// the selection launches: 1 fill, 2 per pass, compaction, sort
int run_select(const float* scores, const int32_t* labels, int32_t b, int64_t n, const float* thresholds, int32_t n_thresh,
               int per_class, const Plan& pl, char* ws, int32_t* scnt, int64_t* cand, int cand_ld, hipStream_t s) {
  // the sort takes up to 128 KiB of dynamic LDS: the attribute belongs to the device's copy of the kernel, so it is
  // raised once per device (two threads that race here only raise it twice)
  static std::atomic<int> raised[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return SPX_ERR_LAUNCH;
  if (dev < 0 || dev >= kMaxDevices || !raised[dev].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kMaxPre * 8) != hipSuccess)
      return SPX_ERR_LAUNCH;
    if (dev >= 0 && dev < kMaxDevices) raised[dev].store(1, std::memory_order_release);
  }
  Thresh th;
  for (int i = 0; i < kMaxThresh; ++i) th.v[i] = (thresholds && i < n_thresh) ? thresholds[i] : 0.f;
  const int has_thresh = thresholds ? 1 : 0, pc = per_class ? 1 : 0;
  SlotState* st = reinterpret_cast<SlotState*>(ws + pl.off_state);
  int32_t* hist = reinterpret_cast<int32_t*>(ws + pl.off_hist);
  unsigned long long* cbuf = reinterpret_cast<unsigned long long*>(ws + pl.off_cbuf);
  unsigned long long* skeys = reinterpret_cast<unsigned long long*>(ws + pl.off_skeys);
  spx_fill_async(ws + pl.off_state, 0, pl.off_cbuf - pl.off_state, s);      // slot states and every pass's histogram
  const dim3 grows((unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)b);
  int left = 32 + pl.rb;
  for (int pass = 0; pass < pl.passes; ++pass) {
    const int bits = left < kDigitBits ? left : kDigitBits;
    left -= bits;
    int32_t* h = hist + (size_t)pass * pl.slots * kBins;
    hipLaunchKernelGGL(k_hist, grows, dim3(kHistThreads), (size_t)n_thresh * kBins * 4, s, scores, labels, (int)n, th,
                       has_thresh, pc, (int)n_thresh, pl.rb, left, bits, st, h);
    hipLaunchKernelGGL(k_scan, dim3((unsigned)pl.slots), dim3(256), 0, s, h, st, pass == 0 ? 1 : 0, pl.pre, bits);
  }
  hipLaunchKernelGGL(k_compact, grows, dim3(kHistThreads), 0, s, scores, labels, (int)n, th, has_thresh, pc,
                     (int)n_thresh, pl.rb, pl.pre, st, cbuf);
  hipLaunchKernelGGL(k_sort, dim3((unsigned)pl.slots), dim3(kThreads), (size_t)pl.p * 8, s, st, cbuf, (int)n,
                     (int)n_thresh, pl.rb, pl.pre, pl.p, skeys, scnt, cand, cand_ld);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

}  // namespace

extern "C" size_t spx_dense_select_ws_bytes(int32_t b, int64_t n, int32_t n_thresh, int64_t pre_max) {
  if (b < 1 || n < 1 || n_thresh < 1 || n_thresh > kMaxThresh || pre_max < 1 || pre_max > kMaxPre) return spx_align(1);
  return make_plan(b, n, n_thresh, pre_max, 1, false).bytes;
}

extern "C" int spx_dense_select(const float* scores, const int32_t* labels, int32_t b, int64_t n, const float* thresholds,
                                int32_t n_thresh, int64_t pre_max, int per_class, int64_t* cand, int32_t* cand_count,
                                void* ws, size_t ws_bytes, spx_stream_t stream) {
  if (!scores || !labels || !cand || !cand_count) return SPX_ERR_INVALID_ARG;
  const int rc = check_common(b, n, n_thresh, pre_max, per_class);
  if (rc != SPX_OK) return rc;
  if ((int64_t)b * n == 0) return SPX_OK;
  if (!ws || ws_bytes < spx_dense_select_ws_bytes(b, n, n_thresh, pre_max)) return SPX_ERR_WORKSPACE;
  const Plan pl = make_plan(b, n, n_thresh, pre_max, 1, false);
  hipStream_t s = spx_s(stream);
  char* w = static_cast<char*>(ws);
  return run_select(scores, labels, b, n, thresholds, n_thresh, per_class, pl, w, cand_count, cand, (int)pre_max, s);
}

extern "C" size_t spx_dense_post_process_ws_bytes(int32_t b, int64_t n, int32_t n_thresh, int64_t pre_max,
                                                  int64_t post_max) {
  if (b < 1 || n < 1 || n_thresh < 1 || n_thresh > kMaxThresh || pre_max < 1 || pre_max > kMaxPre || post_max < 1)
    return spx_align(1);
  return make_plan(b, n, n_thresh, pre_max, post_max, true).bytes;
}

extern "C" int spx_dense_post_process(const float* scores, const int32_t* labels, const float* boxes, int32_t box_ld,
                                      int32_t b, int64_t n, const float* thresholds, int32_t n_thresh, float nms_thresh,
                                      int64_t pre_max, int64_t post_max, int axis_aligned, int per_class, int64_t* sel,
                                      int32_t* count, float* out_boxes, float* out_scores, int64_t* out_labels, void* ws,
                                      size_t ws_bytes, spx_stream_t stream) {
  if (!scores || !labels || !boxes || !sel || !count || !out_boxes || !out_scores || !out_labels)
    return SPX_ERR_INVALID_ARG;
  if (post_max < 1 || box_ld < 7) return SPX_ERR_INVALID_ARG;
  const int rc = check_common(b, n, n_thresh, pre_max, per_class);
  if (rc != SPX_OK) return rc;
  if (b == 0) return SPX_OK;
  hipStream_t s = spx_s(stream);
  if (n == 0) {     // capacity 0: only the counts exist
    spx_fill_async(count, 0, (size_t)b * sizeof(int32_t), s);
    SPX_CHECK_LAUNCH();
    return SPX_OK;
  }
  const Plan pl = make_plan(b, n, n_thresh, pre_max, post_max, true);
  if ((int64_t)n_thresh * pl.post_cap > kMaxN) return SPX_ERR_TOO_LARGE;      // the final stage is one workgroup
  if (!ws || ws_bytes < pl.bytes) return SPX_ERR_WORKSPACE;
  char* w = static_cast<char*>(ws);
  int32_t* scnt = reinterpret_cast<int32_t*>(w + pl.off_scnt);
  const int r2 = run_select(scores, labels, b, n, thresholds, n_thresh, per_class, pl, w, scnt, nullptr, 0, s);
  if (r2 != SPX_OK) return r2;
  const unsigned long long* skeys = reinterpret_cast<unsigned long long*>(w + pl.off_skeys);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(w + pl.off_mask);
  unsigned long long* surv = reinterpret_cast<unsigned long long*>(w + pl.off_surv);
  int32_t* kcnt = reinterpret_cast<int32_t*>(w + pl.off_kcnt);
  const int64_t tiles = (int64_t)pl.slots * pl.words * pl.words;
  const dim3 gmask((unsigned)(tiles < kMaskBlocks ? tiles : kMaskBlocks)), gslots((unsigned)pl.slots), gb((unsigned)b);
  const int cap = (int)spx_point_post_process_capacity(n, n_thresh, post_max, per_class);
  const int pc = per_class ? 1 : 0;
  if (axis_aligned) {
    hipLaunchKernelGGL((k_pair_mask<true>), gmask, dim3(kMaskThreads), 0, s, boxes, (int)box_ld, (int)n, (int)n_thresh, pl.slots,
                       pl.pre, pl.words, nms_thresh, skeys, scnt, mask);
    hipLaunchKernelGGL(k_reduce, gslots, dim3(256), 0, s, skeys, scnt, mask, pl.pre, pl.words, pl.post_cap, surv, kcnt);
    hipLaunchKernelGGL((k_frame_out<true>), gb, dim3(kThreads), 0, s, scores, labels, boxes, (int)box_ld, (int)n,
                       (int)n_thresh, nms_thresh, pl.post_cap, pc, surv, kcnt, cap, sel, count, out_boxes, out_scores,
                       out_labels);
  } else {
    hipLaunchKernelGGL((k_pair_mask<false>), gmask, dim3(kMaskThreads), 0, s, boxes, (int)box_ld, (int)n, (int)n_thresh, pl.slots,
                       pl.pre, pl.words, nms_thresh, skeys, scnt, mask);
    hipLaunchKernelGGL(k_reduce, gslots, dim3(256), 0, s, skeys, scnt, mask, pl.pre, pl.words, pl.post_cap, surv, kcnt);
    hipLaunchKernelGGL((k_frame_out<false>), gb, dim3(kThreads), 0, s, scores, labels, boxes, (int)box_ld, (int)n,
                       (int)n_thresh, nms_thresh, pl.post_cap, pc, surv, kcnt, cap, sel, count, out_boxes, out_scores,
                       out_labels);
  }
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
