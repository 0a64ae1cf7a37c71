// dyn_pillar_vfe.hip — DynamicPillarVFE: sort-free, sync-free pillarisation and one fused last-layer PFNLayerV2, forward
// and parameter gradients (include/spx.h §24).
//
// Restates DynamicPillarVFE.forward + PFNLayerV2.forward (reference pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py)
// for NUM_FILTERS of length 1 with USE_NORM.  Every in-range point is kept: there is no per-pillar or per-frame cap and no
// [M, T, C] buffer, a pillar is a RAGGED list of point rows.
//
// Pillarisation (spx_dynamic_pillarize), ten launches, launch shapes from host values only:
//   clear the bitmap ; mark every kept point's cell in a bitmap laid out in key order ((b X + cx) Y + cy) ; popcount per
//   256 words ; ranks of the words + coords of the set bits (rank order IS torch.unique's order; every block sums the block
//   sums before it, no single-block scan) ; rank of every point + integer-atomic count per pillar ; block sums of count
//   over 1 024 rows ; offsets (again every block sums the block sums before it) ; bucket (slot = what the count atomic
//   returned) ; order the buckets.  The atomic hands out slots in arrival order, so every bucket is then put into
//   ascending point order, which makes the result independent of that order (bitwise reproducible):
//     m <= 64      one wave per pillar ranks its elements with m shuffles,
//     m <= 2 048   one block ranks the bucket in LDS (m^2 / 256 LDS reads per thread),
//     m >  2 048   one block re-derives the bucket by a compacting scan over point_to_pillar, 2 048 points per step:
//                  O(n / 256) per thread whatever m is, and there are at most n / 2 048 such pillars.
//   Nothing is serial in the size of a pillar.
//
// PFN layer.  The core — the 13 fixed feature slots and their slot -> weight-column table, the S1 / G statistics, the
// BatchNorm fold and the closed-form weight gradient — is pfn_layer.h, shared with pillar_vfe.hip; the derivations are
// there.  Tiles are 256 consecutive positions of `order`, so the points of a pillar are contiguous and a pillar may span
// any number of tiles.  There are no padding rows: N is the number of kept points.
// Training forward, five launches:
//   1. k_mean: per pillar the mean of xyz, a double sum in a fixed order over `order` (one wave per pillar);
//   2. k_stats: S1 = sum f and G = sum f f^T over the kept points, tile i to block i mod 1 024, one partial per block;
//   3. k_stats_final: fixed-order sum of the partials, N = *d_num_points, then pfn_layer.h's per-channel statistics;
//      the running statistics and the counter move only when N >= 2 (torch raises below two samples; here the status
//      word says so);
//   4. k_fwd: a wave walks 64 consecutive positions, lane = channel: z = (w.f) * scale + shift in double, ReLU, running max
//      and the winning point row per pillar segment.  A pillar wholly inside the 64 positions is written at once; a segment
//      cut by the chunk's edge goes to one of the chunk's two partial slots (head / tail);
//   5. k_fwd_combine: one thread per (pillar, channel) joins the partials of a pillar that spans chunks, in position order
//      (strict >, so ties keep the lowest position), and writes exact zeros to dead rows.
// Eval forward: launches 1, 4, 5 with scale / shift folded from the running statistics.  The [N, 64] activations are
// never written.  Backward, two launches: k_bwd_gather takes A, d_beta, d_gamma of pfn_layer.h's dW formula (every selected
// row is a real point), pfn_k_bwd_final applies it.
//
// Integer atomics only (bitmap OR, count, the large-pillar list; nothing that is kept depends on their order), no float
// atomics, no host read, every floating sum in double in a fixed order.  Rows at or beyond min(*d_num_pillars, cap) and
// positions at or beyond *d_num_points are never dereferenced.
#include "block_ops.h"
#include "pfn_layer.h"

namespace {

constexpr int kBlock = 256;
constexpr int kStatPart = 1024;               // partial-writing blocks of k_stats
constexpr int kMaxPart = 256;                 // partial-writing blocks of k_bwd_gather
constexpr int kSmall = 64;                    // bucket sizes: one wave / one block in LDS / compacting scan
constexpr int kMedium = 2048;
constexpr int kScanRows = 4 * kBlock;         // rows of `count` per block of the offset scan
constexpr int kBwdRows = 16;                  // pillars per tile of k_bwd_gather

// ------------------------------------------------------------------------------------------------ block helpers
// sum of a[0 .. b) by the whole block (integers: the order does not matter)
__device__ __forceinline__ uint32_t block_sum_before(const uint32_t* __restrict__ a, int64_t b, uint32_t* wsum) {
  uint32_t s = 0;
  for (int64_t j = threadIdx.x; j < b; j += kBlock) s += a[j];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if (spx_lane() == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  const uint32_t r = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int64_t live_rows(const int64_t* d_n, int64_t cap) {
  int64_t v = *d_n;
  if (v < 0) v = 0;
  return v < cap ? v : cap;
}

// ------------------------------------------------------------------------------------------------ pillarisation
struct PGeo {
  float lo[2], vs[2];
  int32_t gx, gy;
  int batch;
};

// floor((p - lo) / vs) in fp32, the subtraction and the division rounded separately; -1 outside [0, n) and for NaN
__device__ __forceinline__ int cell_of(float p, float lo, float vs, int n) {
  const float f = floorf(__fdiv_rn(__fsub_rn(p, lo), vs));
  if (!(f >= 0.f) || !(f < (float)n)) return -1;
  return (int)f;
}

__global__ __launch_bounds__(kBlock) void k_mark(const float* __restrict__ pts, int64_t n, int stride, int batch_col,
                                                 int xyz_col, PGeo g, uint64_t* __restrict__ bits,
                                                 int32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ p = pts + i * stride;
  int32_t key = -1;
  const int cx = cell_of(p[xyz_col], g.lo[0], g.vs[0], g.gx);
  const int cy = cell_of(p[xyz_col + 1], g.lo[1], g.vs[1], g.gy);
  const float bf = batch_col >= 0 ? p[batch_col] : 0.f;
  if (cx >= 0 && cy >= 0 && bf >= 0.f && bf < (float)g.batch) key = ((int)bf * g.gx + cx) * g.gy + cy;
  keys[i] = key;
  if (key < 0) return;
  // A cell next to the sensor holds hundreds of points and its 64-cell word thousands: same-address atomics, which the L2
  // serialises.  Bits only ever go from 0 to 1, so a look that bypasses the L1 may miss a bit (one atomic too many) but
  // never invents one.
  unsigned long long* word = reinterpret_cast<unsigned long long*>(&bits[key >> 6]);
  const unsigned long long bit = 1ull << (key & 63);
  if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0ull) atomicOr(word, bit);
}

// popcount of 256 words per block; the same grid clears count and the counter of the large-pillar list (both are first
// touched later in the stream)
__global__ __launch_bounds__(kBlock) void k_blocksum(const uint64_t* __restrict__ bits, int64_t nwords,
                                                     uint32_t* __restrict__ blocksum, int32_t* __restrict__ count,
                                                     int32_t* __restrict__ n_big, int64_t cap) {
  __shared__ uint32_t wsum[4];
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t s = w < nwords ? (uint32_t)__popcll(bits[w]) : 0u;
  uint32_t total;
  spx_block_excl_scan(s, &total, wsum);
  if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
  for (int64_t r = w; r < cap; r += (int64_t)gridDim.x * kBlock) count[r] = 0;
  if (w == 0) *n_big = 0;
}

__global__ __launch_bounds__(kBlock) void k_expand(const uint64_t* __restrict__ bits, int64_t nwords,
                                                   const uint32_t* __restrict__ blocksum, uint32_t* __restrict__ prefix,
                                                   PGeo g, int32_t* __restrict__ coords, int64_t cap,
                                                   int64_t* __restrict__ d_num_pillars, int32_t* status) {
  __shared__ uint32_t wsum[4];
  const uint32_t base = block_sum_before(blocksum, blockIdx.x, wsum);
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  uint64_t m = w < nwords ? bits[w] : 0ull;
  uint32_t total;
  uint32_t run = base + spx_block_excl_scan((uint32_t)__popcll(m), &total, wsum);
  if (w < nwords) prefix[w] = run;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const int64_t np = (int64_t)base + total;
    *d_num_pillars = np;
    if (status && np > cap) atomicMin(status, (int32_t)SPX_ERR_CAPACITY);
  }
  while (m != 0ull) {
    const int bit = __ffsll((unsigned long long)m) - 1;
    m &= m - 1ull;
    if ((int64_t)run < cap) {
      const uint32_t key = (uint32_t)(w * 64 + bit);
      const uint32_t cy = key % (uint32_t)g.gy, t = key / (uint32_t)g.gy;
      const uint32_t cx = t % (uint32_t)g.gx, b = t / (uint32_t)g.gx;
      reinterpret_cast<int4*>(coords)[run] = make_int4((int)b, 0, (int)cy, (int)cx);
    }
    ++run;
  }
}

// keys[i] becomes the point's slot inside its bucket: what the count atomic returned (arrival order)
__global__ __launch_bounds__(kBlock) void k_rank(int32_t* __restrict__ keys, int64_t n, const uint64_t* __restrict__ bits,
                                                 const uint32_t* __restrict__ prefix, int64_t cap,
                                                 int32_t* __restrict__ inv, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t key = keys[i];
  int32_t rk = -1;
  if (key >= 0) {
    const uint64_t w = bits[key >> 6];
    const int64_t r = (int64_t)prefix[key >> 6] + __popcll(w & ((1ull << (key & 63)) - 1ull));
    if (r < cap) {
      rk = (int32_t)r;
      keys[i] = atomicAdd(&count[rk], 1);
    }
  }
  inv[i] = rk;
}

// rows [0, cap] in blocks of 1 024; row cap counts 0.  count of a dead row is 0, so no live count is needed.
__global__ __launch_bounds__(kBlock) void k_count_blocksum(const int32_t* __restrict__ count, int64_t cap,
                                                           uint32_t* __restrict__ cblock) {
  __shared__ uint32_t wsum[4];
  const int64_t r0 = (int64_t)blockIdx.x * kScanRows + threadIdx.x * 4;
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (r0 + j < cap) s += (uint32_t)count[r0 + j];
  uint32_t total;
  spx_block_excl_scan(s, &total, wsum);
  if (threadIdx.x == 0) cblock[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_offsets(const int32_t* __restrict__ count, int64_t cap,
                                                    const uint32_t* __restrict__ cblock, int32_t* __restrict__ offset,
                                                    int64_t* __restrict__ d_num_points) {
  __shared__ uint32_t wsum[4];
  const uint32_t base = block_sum_before(cblock, blockIdx.x, wsum);
  const int64_t r0 = (int64_t)blockIdx.x * kScanRows + threadIdx.x * 4;
  uint32_t c[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = r0 + j < cap ? (uint32_t)count[r0 + j] : 0u;
    s += c[j];
  }
  uint32_t run = base + spx_block_excl_scan(s, nullptr, wsum);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (r0 + j <= cap) offset[r0 + j] = (int32_t)run;
    if (r0 + j == cap) *d_num_points = (int64_t)run;
    run += c[j];
  }
}

__global__ __launch_bounds__(kBlock) void k_bucket(const int32_t* __restrict__ inv, int64_t n,
                                                   const int32_t* __restrict__ offset, const int32_t* __restrict__ slot,
                                                   int32_t* __restrict__ order) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t rk = inv[i];
  if (rk < 0) return;
  order[offset[rk] + slot[i]] = (int32_t)i;
}

// one wave per pillar with 2 <= m <= 64 points: rank by counting, m shuffles.  A larger pillar goes onto the list of
// k_order_big (in arrival order, which no result depends on): such pillars sit next to each other in key order, and the
// list spreads them over that launch's blocks.
__global__ __launch_bounds__(kBlock) void k_order_small(const int32_t* __restrict__ count, const int32_t* __restrict__ offset,
                                                        const int64_t* __restrict__ d_np, int64_t cap,
                                                        int32_t* __restrict__ order, int32_t* __restrict__ n_big,
                                                        int32_t* __restrict__ big) {
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= live_rows(d_np, cap)) return;
  const int m = count[p];
  const int lane = spx_lane();
  if (m > kSmall) {
    if (lane == 0) big[atomicAdd(n_big, 1)] = (int32_t)p;
    return;
  }
  if (m < 2) return;
  int32_t* __restrict__ b = order + offset[p];
  const int32_t v = lane < m ? b[lane] : 0x7fffffff;
  int rank = 0;
  for (int j = 0; j < m; ++j) rank += __shfl(v, j, 64) < v ? 1 : 0;
  if (lane < m) b[rank] = v;
}

// the listed pillars (more than 64 points), entry e to block e mod gridDim
__global__ __launch_bounds__(kBlock) void k_order_big(const int32_t* __restrict__ count, const int32_t* __restrict__ offset,
                                                      const int32_t* __restrict__ inv, int64_t n,
                                                      const int32_t* __restrict__ n_big, const int32_t* __restrict__ big,
                                                      int64_t cap, int32_t* __restrict__ order) {
  __shared__ int32_t s_v[kMedium];
  __shared__ uint32_t wsum[4];
  int64_t entries = *n_big;
  if (entries > cap) entries = cap;
  for (int64_t e0 = blockIdx.x; e0 < entries; e0 += gridDim.x) {
    const int64_t p = big[e0];
    if (p < 0 || p >= cap) continue;
    const int m = count[p];
    const int32_t off = offset[p];
    if (m <= kMedium) {
      for (int e = threadIdx.x; e < m; e += kBlock) s_v[e] = order[off + e];
      __syncthreads();
      for (int e = threadIdx.x; e < m; e += kBlock) {
        const int32_t v = s_v[e];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += s_v[j] < v ? 1 : 0;
        order[off + rank] = v;
      }
      __syncthreads();
    } else {
      uint32_t base = 0;
      for (int64_t i0 = 0; i0 < n; i0 += 8 * kBlock) {
        const int64_t b = i0 + threadIdx.x * 8;
        uint32_t mask = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (b + u < n && inv[b + u] == (int32_t)p) mask |= 1u << u;
        uint32_t total;
        uint32_t dst = base + spx_block_excl_scan((uint32_t)__popc(mask), &total, wsum);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if ((mask >> u) & 1u) {
            if (dst < (uint32_t)m) order[off + dst] = (int32_t)(b + u);
            ++dst;
          }
        base += total;
      }
    }
  }
}

struct PWs {
  uint64_t* bits;
  uint32_t *blocksum, *prefix, *cblock;
  int32_t *keys, *n_big;        // keys: the cell key, then the slot inside the bucket, then the large-pillar list
  int64_t nwords, nblk, ncb;
  size_t total;
};

PWs p_layout(void* ws, int64_t n, int64_t cells, int64_t cap) {
  PWs r;
  r.nwords = (cells + 63) / 64;
  r.nblk = (r.nwords + kBlock - 1) / kBlock;
  r.ncb = (cap + 1 + kScanRows - 1) / kScanRows;
  char* p = reinterpret_cast<char*>(ws);
  size_t o = 0;
  r.bits = reinterpret_cast<uint64_t*>(p + o);
  o += spx_align((size_t)r.nwords * 8);
  r.blocksum = reinterpret_cast<uint32_t*>(p + o);
  o += spx_align((size_t)r.nblk * 4);
  r.prefix = reinterpret_cast<uint32_t*>(p + o);
  o += spx_align((size_t)r.nwords * 4);
  r.cblock = reinterpret_cast<uint32_t*>(p + o);
  o += spx_align((size_t)r.ncb * 4);
  r.keys = reinterpret_cast<int32_t*>(p + o);
  o += spx_align((size_t)(n > cap ? n : cap) * 4);
  r.n_big = reinterpret_cast<int32_t*>(p + o);
  o += spx_align(4);
  r.total = o;
  return r;
}

// ---------------------------------------------------------------------------------------------------- PFN layer
struct Geo {
  float vx, vy, ox, oy, oz;
  int c;
  int col[kSlots];                // slot -> weight column, -1 absent
  int c_in;
};

struct In {
  const float* pts;               // [n, stride]
  int stride, xyz_col;
  const int32_t *coords, *inv, *offset, *order;
  const int64_t *d_np, *d_npts;
  int64_t n, cap;
};

__device__ __forceinline__ int64_t kept_points(const In& in) {
  int64_t v = *in.d_npts;
  if (v < 0) v = 0;
  return v < in.n ? v : in.n;
}

// the 13 feature slots of point row i in pillar p (both already checked)
__device__ __forceinline__ void features(const In& in, const Geo& g, const double* __restrict__ pmean, int64_t i, int64_t p,
                                         double* f) {
  const float* __restrict__ pt = in.pts + i * in.stride + in.xyz_col;
  const double dx = pt[0], dy = pt[1], dz = pt[2];
  const int32_t* __restrict__ cd = in.coords + p * 4;
  const float cx = centre32(cd[3], g.vx, g.ox);
  const float cy = centre32(cd[2], g.vy, g.oy);
  f[0] = dx;
  f[1] = dy;
  f[2] = dz;
  f[3] = dx - pmean[p * 3 + 0];
  f[4] = dy - pmean[p * 3 + 1];
  f[5] = dz - pmean[p * 3 + 2];
  f[6] = dx - (double)cx;
  f[7] = dy - (double)cy;
  f[8] = dz - (double)g.oz;
  f[9] = sqrt(dx * dx + dy * dy + dz * dz);
#pragma unroll
  for (int j = 0; j < 3; ++j) f[10 + j] = 3 + j < g.c ? (double)pt[3 + j] : 0.0;
}

// one wave per pillar: lane l adds positions l, l + 64, ... in that order, then an xor butterfly
__global__ __launch_bounds__(kBlock) void k_mean(In in, double* __restrict__ pmean) {
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= live_rows(in.d_np, in.cap)) return;
  const int64_t npts = kept_points(in);
  int64_t b = in.offset[p], e = in.offset[p + 1];
  if (b < 0) b = 0;
  if (e > npts) e = npts;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t j = b + spx_lane(); j < e; j += 64) {
    const int64_t i = in.order[j];
    if (i < 0 || i >= in.n) continue;
    const float* __restrict__ pt = in.pts + i * in.stride + in.xyz_col;
    sx += (double)pt[0];
    sy += (double)pt[1];
    sz += (double)pt[2];
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sx += __shfl_xor(sx, d, 64);
    sy += __shfl_xor(sy, d, 64);
    sz += __shfl_xor(sz, d, 64);
  }
  if (spx_lane() == 0) {
    const double m = e > b ? (double)(e - b) : 1.0;
    pmean[p * 3 + 0] = sx / m;
    pmean[p * 3 + 1] = sy / m;
    pmean[p * 3 + 2] = sz / m;
  }
}

// Features of positions [pos0, pos0 + 256) of `order` into fs[t * 13 + slot]; s_pil[t] = the pillar (-1: no point),
// s_row[t] = the point row, s_beg / s_end[t] = the pillar's position range.  Thread t builds position pos0 + t.
__device__ __forceinline__ void build_tile(const In& in, const Geo& g, const double* __restrict__ pmean, int64_t pos0,
                                           int64_t npts, int64_t live, double* fs, int32_t* s_pil, int32_t* s_row,
                                           int32_t* s_beg, int32_t* s_end) {
  const int t = threadIdx.x;
  const int64_t pos = pos0 + t;
  int64_t i = -1, p = -1;
  if (pos < npts) {
    i = in.order[pos];
    if (i >= 0 && i < in.n) p = in.inv[i];
    if (p < 0 || p >= live) p = -1;
  }
  double* __restrict__ f = fs + t * kSlots;
  if (p >= 0) {
    features(in, g, pmean, i, p, f);
    s_beg[t] = in.offset[p];
    s_end[t] = in.offset[p + 1];
  } else {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) f[k] = 0.0;
    s_beg[t] = s_end[t] = 0;
  }
  s_pil[t] = (int32_t)p;
  s_row[t] = (int32_t)i;
}

#define SPX_DPV_TILE_LDS                         \
  __shared__ double fs[kBlock * kSlots];         \
  __shared__ int32_t s_pil[kBlock], s_row[kBlock], s_beg[kBlock], s_end[kBlock]

__global__ __launch_bounds__(kBlock) void k_stats(In in, Geo g, const double* __restrict__ pmean, double* __restrict__ part) {
  SPX_DPV_TILE_LDS;
  const int64_t npts = kept_points(in), live = live_rows(in.d_np, in.cap);
  const int e = threadIdx.x;
  const bool gram = e < kG;
  const int i = gram ? e / kSlots : 0, j = gram ? e % kSlots : (e < kStat ? e - kG : 0);
  double acc = 0.0;
  for (int64_t tile = blockIdx.x; tile * kBlock < npts; tile += gridDim.x) {
    build_tile(in, g, pmean, tile * kBlock, npts, live, fs, s_pil, s_row, s_beg, s_end);
    __syncthreads();
    if (e < kStat) {
      // four running sums over the positions t mod 4 (the LDS reads of one sum would wait for each other), joined in a
      // fixed order: the result depends on the tile's point count alone
      const int64_t left = npts - tile * kBlock;
      const int cnt = left < kBlock ? (int)left : kBlock;
      const double* __restrict__ f = fs;
      double a[4] = {0.0, 0.0, 0.0, 0.0};
      int t = 0;
      for (; t + 4 <= cnt; t += 4, f += 4 * kSlots) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = gram ? fma(f[u * kSlots + i], f[u * kSlots + j], a[u]) : a[u] + f[u * kSlots + j];
      }
      for (; t < cnt; ++t, f += kSlots) a[0] = gram ? fma(f[i], f[j], a[0]) : a[0] + f[j];
      acc += (a[0] + a[1]) + (a[2] + a[3]);
    }
    __syncthreads();
  }
  if (e < kStat) part[(int64_t)blockIdx.x * kStat + e] = acc;
}

__global__ __launch_bounds__(kBlock) void k_stats_final(In in, Geo g, BN bn, const double* __restrict__ part, int n_part,
                                                        double* __restrict__ stats, double* __restrict__ ss,
                                                        float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                        int32_t* status) {
  __shared__ double s[kStat];
  const int e = threadIdx.x;
  if (e < kStat) {
    double a = 0.0;
#pragma unroll 8
    for (int b = 0; b < n_part; ++b) a += part[(int64_t)b * kStat + e];   // in block order; unrolled so the loads overlap
    s[e] = a;
    stats[e] = a;
  }
  __syncthreads();
  const double n = (double)kept_points(in);
  const bool enough = n >= 2.0;   // torch raises below two samples; here: no running update, the status word says so
  if (e == 0) {
    stats[kOffN] = n;
    stats[kOffN + 1] = 0.0;
    if (enough) {
      if (bn.nbt) bn.nbt[0] += 1;
    } else if (status) {
      atomicMin(status, (int32_t)SPX_ERR_BATCH_STATS);
    }
  }
  if (e >= kCout) return;
  stats_channel(bn, g, s, n, enough, e, stats, ss, save_mean, save_invstd);
}

// ss: the folded scale / shift of k_stats_final, or nullptr: fold the running statistics here (eval)
// pv / pa: per 64-position chunk two partial slots (0: the segment holding the chunk's first position, 1: its last)
__global__ __launch_bounds__(kBlock) void k_fwd(In in, Geo g, BN bn, const double* __restrict__ pmean,
                                                const double* __restrict__ ss, float* __restrict__ out,
                                                int32_t* __restrict__ arg, double* __restrict__ pv, int32_t* __restrict__ pa) {
  SPX_DPV_TILE_LDS;
  const int64_t npts = kept_points(in), live = live_rows(in.d_np, in.cap);
  const int64_t pos0 = (int64_t)blockIdx.x * kBlock;
  if (pos0 >= npts) return;
  build_tile(in, g, pmean, pos0, npts, live, fs, s_pil, s_row, s_beg, s_end);
  const int q = threadIdx.x >> 6, ch = threadIdx.x & 63;
  double w[kSlots];
  load_w(bn.weight, g, ch, w);
  double scale, shift;
  fold_scale_shift(bn, ss, ch, scale, shift);
  __syncthreads();
  const int tb = q * 64;
  const int64_t cstart = pos0 + tb;
  const int64_t left = npts - cstart;
  const int cvalid = left < 64 ? (int)left : 64;
  const int64_t chunk = cstart >> 6;
  int t = 0;
  while (t < cvalid) {
    const int p = s_pil[tb + t];
    const int64_t pb = s_beg[tb + t], pe = s_end[tb + t];
    int64_t t1 = pe - cstart;
    if (t1 > cvalid) t1 = cvalid;
    if (p < 0 || t1 <= t) {       // not a point of a live pillar (cannot happen with consistent inputs): skip it
      ++t;
      continue;
    }
    double best = -1.0;
    int a = -1;
    const double* __restrict__ f = fs + (tb + t) * kSlots;
    for (int u = t; u < (int)t1; ++u, f += kSlots) {
      const double z = fma(dot13(w, f), scale, shift);
      const double r = z > 0.0 ? z : 0.0;
      if (r > best) {             // strict: ties keep the lowest position
        best = r;
        a = s_row[tb + u];
      }
    }
    if (pb >= cstart && pe <= cstart + 64) {
      out[(int64_t)p * kCout + ch] = (float)best;
      arg[(int64_t)p * kCout + ch] = a;
    } else {
      if (t == 0) {
        pv[(chunk * 2 + 0) * kCout + ch] = best;
        pa[(chunk * 2 + 0) * kCout + ch] = a;
      }
      if (t1 == 64) {
        pv[(chunk * 2 + 1) * kCout + ch] = best;
        pa[(chunk * 2 + 1) * kCout + ch] = a;
      }
    }
    t = (int)t1;
  }
}

__global__ __launch_bounds__(kBlock) void k_fwd_combine(In in, const double* __restrict__ pv, const int32_t* __restrict__ pa,
                                                        float* __restrict__ out, int32_t* __restrict__ arg) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int ch = threadIdx.x & 63;
  if (row >= in.cap) return;
  if (row >= live_rows(in.d_np, in.cap)) {    // a dead row: exact zeros, nothing read
    out[row * kCout + ch] = 0.f;
    arg[row * kCout + ch] = -1;
    return;
  }
  const int64_t npts = kept_points(in);
  int64_t b = in.offset[row], e = in.offset[row + 1];
  if (e > npts) e = npts;
  if (b < 0 || e <= b) {                      // an empty live row cannot come from spx_dynamic_pillarize
    out[row * kCout + ch] = 0.f;
    arg[row * kCout + ch] = -1;
    return;
  }
  const int64_t k0 = b >> 6, k1 = (e - 1) >> 6;
  if (k0 == k1) return;                       // written by k_fwd
  double best = pv[(k0 * 2 + 1) * kCout + ch];
  int32_t a = pa[(k0 * 2 + 1) * kCout + ch];
  for (int64_t k = k0 + 1; k <= k1; ++k) {
    const double v = pv[(k * 2) * kCout + ch];
    if (v > best) {
      best = v;
      a = pa[(k * 2) * kCout + ch];
    }
  }
  out[row * kCout + ch] = (float)best;
  arg[row * kCout + ch] = a;
}

// ------------------------------------------------------------------------------------------------------ backward
__global__ __launch_bounds__(kBlock) void k_bwd_gather(In in, Geo g, BN bn, Bwd<int32_t> b, const double* __restrict__ pmean,
                                                       double* __restrict__ part) {
  __shared__ double red[3 * kAcc * kCout];
  const int64_t live = live_rows(in.d_np, in.cap);
  const int q = threadIdx.x >> 6, ch = threadIdx.x & 63;
  double w[kSlots];
  load_w(bn.weight, g, ch, w);
  double mean, invstd;
  mean_invstd(bn, b, ch, mean, invstd);
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  for (int64_t tile = blockIdx.x; tile * kBwdRows < live; tile += gridDim.x) {
#pragma unroll
    for (int h = 0; h < kBwdRows / 4; ++h) {
      const int64_t row = tile * kBwdRows + q + 4 * h;
      if (row >= live) continue;
      if (!(b.out[row * kCout + ch] > 0.f)) continue;
      const int64_t i = b.arg[row * kCout + ch];
      if (i < 0 || i >= in.n) continue;
      const double gr = (double)b.d_out[row * kCout + ch];
      double f[kSlots];
      features(in, g, pmean, i, row, f);
      const double xhat = (dot13(w, f) - mean) * invstd;
#pragma unroll
      for (int k = 0; k < kSlots; ++k) acc[2 + k] = fma(gr, f[k], acc[2 + k]);
      acc[0] += gr;
      acc[1] = fma(gr, xhat, acc[1]);
    }
  }
  // the four pillar lanes of a channel, added in the order q = 0, 1, 2, 3
  if (q > 0) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) red[((q - 1) * kAcc + k) * kCout + ch] = acc[k];
  }
  __syncthreads();
  if (q == 0) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
      double v = acc[k];
      for (int r = 0; r < 3; ++r) v += red[(r * kAcc + k) * kCout + ch];
      part[((int64_t)blockIdx.x * kAcc + k) * kCout + ch] = v;
    }
  }
}

// Shared argument checks; fills the geometry and (make_cols) the slot -> column table.
inline int make_geo(int64_t n, int stride, int xyz_col, int32_t c, int64_t cap, int32_t c_in, int32_t c_out,
                    const float* geom5, int use_absolute_xyz, int with_distance, Geo* g) {
  if (n < 0 || cap <= 0 || !geom5 || c < 3 || c > 6 || stride <= 0 || xyz_col < 0 || xyz_col + c > stride)
    return SPX_ERR_INVALID_ARG;
  const int rc = make_cols(c, c_in, c_out, use_absolute_xyz, with_distance, g->col);
  if (rc != SPX_OK) return rc;
  if (n >= (1ll << 31) || cap >= (1ll << 31) / kCout) return SPX_ERR_TOO_LARGE;
  g->vx = geom5[0];
  g->vy = geom5[1];
  g->ox = geom5[2];
  g->oy = geom5[3];
  g->oz = geom5[4];
  g->c = c;
  g->c_in = c_in;
  return SPX_OK;
}

struct VWs {
  double *part, *ss, *pv;
  int32_t* pa;
  size_t total;
};

VWs v_layout(void* ws, int64_t n) {
  VWs r;
  const size_t chunks = (size_t)((n > 0 ? n : 1) + 63) / 64;
  const size_t np_fwd = (size_t)kStatPart * kStat * 8, np_bwd = (size_t)kMaxPart * kAcc * kCout * 8;
  char* p = reinterpret_cast<char*>(ws);
  size_t o = 0;
  r.part = reinterpret_cast<double*>(p + o);
  o += spx_align(np_fwd > np_bwd ? np_fwd : np_bwd);
  r.ss = reinterpret_cast<double*>(p + o);
  o += spx_align(2 * kCout * 8);
  r.pv = reinterpret_cast<double*>(p + o);
  o += spx_align(chunks * 2 * kCout * 8);
  r.pa = reinterpret_cast<int32_t*>(p + o);
  o += spx_align(chunks * 2 * kCout * 4);
  r.total = o;
  return r;
}

}  // namespace

extern "C" size_t spx_dynamic_pillarize_ws_bytes(int64_t n_points, int batch, const int32_t* grid2, int64_t cap) {
  if (!grid2 || batch <= 0 || cap <= 0 || n_points < 0 || grid2[0] <= 0 || grid2[1] <= 0) return 0;
  return p_layout(nullptr, n_points, (int64_t)batch * grid2[0] * grid2[1], cap).total;
}

extern "C" int spx_dynamic_pillarize(const float* points, int64_t n_points, int stride, int batch_col, int xyz_col,
                                     const float* range_lo2, const float* voxel_size2, const int32_t* grid2, int batch,
                                     int32_t* coords, int32_t* point_to_pillar, int32_t* count, int32_t* offset,
                                     int32_t* order, int64_t* d_num_pillars, int64_t* d_num_points, int64_t cap,
                                     int32_t* d_status, void* ws, size_t ws_bytes, spx_stream_t stream) {
  if ((!points && n_points > 0) || !range_lo2 || !voxel_size2 || !grid2 || !coords || !point_to_pillar || !count ||
      !offset || !order || !d_num_pillars || !d_num_points || n_points < 0 || stride <= 0 || xyz_col < 0 ||
      xyz_col + 2 > stride || batch_col >= stride || batch <= 0 || cap <= 0)
    return SPX_ERR_INVALID_ARG;
  for (int j = 0; j < 2; ++j)
    if (grid2[j] <= 0 || !(voxel_size2[j] > 0.f)) return SPX_ERR_INVALID_ARG;
  if (n_points >= (int64_t(1) << 31) || cap >= (int64_t(1) << 31) - 1) return SPX_ERR_TOO_LARGE;
  const int64_t cells = (int64_t)batch * grid2[0] * grid2[1];
  if (cells >= (int64_t(1) << 31)) return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < spx_dynamic_pillarize_ws_bytes(n_points, batch, grid2, cap)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  PWs w = p_layout(ws, n_points, cells, cap);
  PGeo g;
  for (int j = 0; j < 2; ++j) {
    g.lo[j] = range_lo2[j];
    g.vs[j] = voxel_size2[j];
  }
  g.gx = grid2[0];
  g.gy = grid2[1];
  g.batch = batch;
  const unsigned nbp = (unsigned)((n_points + kBlock - 1) / kBlock);
  spx_fill_async(w.bits, 0, (size_t)w.nwords * 8, s);
  if (n_points > 0)
    hipLaunchKernelGGL(k_mark, dim3(nbp), dim3(kBlock), 0, s, points, n_points, stride, batch_col, xyz_col, g, w.bits, w.keys);
  hipLaunchKernelGGL(k_blocksum, dim3((unsigned)w.nblk), dim3(kBlock), 0, s, w.bits, w.nwords, w.blocksum, count, w.n_big,
                     cap);
  hipLaunchKernelGGL(k_expand, dim3((unsigned)w.nblk), dim3(kBlock), 0, s, w.bits, w.nwords, w.blocksum, w.prefix, g, coords,
                     cap, d_num_pillars, d_status);
  if (n_points > 0)
    hipLaunchKernelGGL(k_rank, dim3(nbp), dim3(kBlock), 0, s, w.keys, n_points, w.bits, w.prefix, cap, point_to_pillar, count);
  hipLaunchKernelGGL(k_count_blocksum, dim3((unsigned)w.ncb), dim3(kBlock), 0, s, count, cap, w.cblock);
  hipLaunchKernelGGL(k_offsets, dim3((unsigned)w.ncb), dim3(kBlock), 0, s, count, cap, w.cblock, offset, d_num_points);
  if (n_points > 0) {
    hipLaunchKernelGGL(k_bucket, dim3(nbp), dim3(kBlock), 0, s, point_to_pillar, n_points, offset, w.keys, order);
    hipLaunchKernelGGL(k_order_small, dim3((unsigned)((cap + 3) / 4)), dim3(kBlock), 0, s, count, offset, d_num_pillars, cap,
                       order, w.n_big, w.keys);
    int64_t nb = (cap + kSmall) / (kSmall + 1);     // at most n / 65 pillars are listed
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_order_big, dim3((unsigned)nb), dim3(kBlock), 0, s, count, offset, point_to_pillar, n_points, w.n_big,
                       w.keys, cap, order);
  }
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_dynamic_pillar_vfe_stats_len(void) { return kStatsLen; }

extern "C" size_t spx_dynamic_pillar_vfe_ws_bytes(int64_t n_points) {
  return v_layout(nullptr, n_points < 0 ? 0 : n_points).total;
}

extern "C" int spx_dynamic_pillar_vfe_fwd(const float* points, int64_t n_points, int stride, int xyz_col, int32_t c,
                                          const int32_t* coords, const int32_t* point_to_pillar, const int32_t* offset,
                                          const int32_t* order, int64_t cap, const int64_t* d_num_pillars,
                                          const int64_t* d_num_points, const float* weight, int32_t c_in, int32_t c_out,
                                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                                          int64_t* num_batches_tracked, float momentum, float eps, const float* geom5,
                                          int use_absolute_xyz, int with_distance, int training, float* out, int32_t* arg,
                                          double* pillar_mean, float* save_mean, float* save_invstd, double* stats,
                                          int32_t* d_status, void* ws, size_t ws_bytes, spx_stream_t stream) {
  Geo g;
  const int rc = make_geo(n_points, stride, xyz_col, c, cap, c_in, c_out, geom5, use_absolute_xyz, with_distance, &g);
  if (rc != SPX_OK) return rc;
  if (!weight || !gamma || !beta || !coords || !offset || !d_num_pillars || !d_num_points || !out || !arg || !pillar_mean)
    return SPX_ERR_INVALID_ARG;
  if (n_points > 0 && (!points || !point_to_pillar || !order)) return SPX_ERR_INVALID_ARG;
  if (training && (!save_mean || !save_invstd || !stats)) return SPX_ERR_INVALID_ARG;
  if (!training && (!running_mean || !running_var)) return SPX_ERR_INVALID_ARG;
  if ((running_mean == nullptr) != (running_var == nullptr)) return SPX_ERR_INVALID_ARG;
  if (!ws || ws_bytes < spx_dynamic_pillar_vfe_ws_bytes(n_points)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  VWs w = v_layout(ws, n_points);
  In in{points, stride, xyz_col, coords, point_to_pillar, offset, order, d_num_pillars, d_num_points, n_points, cap};
  BN bn{weight, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps};
  const unsigned row_blocks = (unsigned)((cap + 3) / 4);
  if (n_points > 0) hipLaunchKernelGGL(k_mean, dim3(row_blocks), dim3(kBlock), 0, s, in, pillar_mean);
  const double* ss = nullptr;
  if (training) {
    // tile i always goes to block i % kStatPart: a call at static capacity adds the same numbers in the same order
    const int np = n_points > 0 ? kStatPart : 0;
    if (np > 0) hipLaunchKernelGGL(k_stats, dim3((unsigned)np), dim3(kBlock), 0, s, in, g, pillar_mean, w.part);
    hipLaunchKernelGGL(k_stats_final, dim3(1), dim3(kBlock), 0, s, in, g, bn, w.part, np, stats, w.ss, save_mean, save_invstd,
                       d_status);
    ss = w.ss;
  }
  if (n_points > 0)
    hipLaunchKernelGGL(k_fwd, dim3((unsigned)((n_points + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, in, g, bn, pillar_mean,
                       ss, out, arg, w.pv, w.pa);
  hipLaunchKernelGGL(k_fwd_combine, dim3(row_blocks), dim3(kBlock), 0, s, in, w.pv, w.pa, out, arg);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_dynamic_pillar_vfe_bwd(const float* points, int64_t n_points, int stride, int xyz_col, int32_t c,
                                          const int32_t* coords, int64_t cap, const int64_t* d_num_pillars,
                                          const float* weight, int32_t c_in, int32_t c_out, const float* gamma,
                                          const float* running_mean, const float* running_var, float eps,
                                          const float* geom5, int use_absolute_xyz, int with_distance, int training,
                                          const float* out, const int32_t* arg, const float* d_out,
                                          const double* pillar_mean, const double* stats, float* d_weight, float* d_gamma,
                                          float* d_beta, void* ws, size_t ws_bytes, spx_stream_t stream) {
  Geo g;
  const int rc = make_geo(n_points, stride, xyz_col, c, cap, c_in, c_out, geom5, use_absolute_xyz, with_distance, &g);
  if (rc != SPX_OK) return rc;
  if (!weight || !gamma || !d_weight || !d_gamma || !d_beta || !coords || !d_num_pillars || !out || !arg || !d_out ||
      !pillar_mean)
    return SPX_ERR_INVALID_ARG;
  if (n_points > 0 && !points) return SPX_ERR_INVALID_ARG;
  if (training ? !stats : (!running_mean || !running_var)) return SPX_ERR_INVALID_ARG;
  if (!ws || ws_bytes < spx_dynamic_pillar_vfe_ws_bytes(n_points)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  VWs w = v_layout(ws, n_points);
  In in{points, stride, xyz_col, coords, nullptr, nullptr, nullptr, d_num_pillars, nullptr, n_points, cap};
  BN bn{weight, gamma, nullptr, const_cast<float*>(running_mean), const_cast<float*>(running_var), nullptr, 0.f, eps};
  Bwd<int32_t> b{out, d_out, arg, stats, training};
  int np = 0;                     // no points: the gradients are zeros, from pfn_k_bwd_final alone
  if (n_points > 0) {
    np = kMaxPart;
    hipLaunchKernelGGL(k_bwd_gather, dim3((unsigned)np), dim3(kBlock), 0, s, in, g, bn, b, pillar_mean, w.part);
  }
  hipLaunchKernelGGL((pfn_k_bwd_final<Geo, int32_t>), dim3(1), dim3(kBlock), 0, s, g, bn, b, w.part, np, d_weight, d_gamma,
                     d_beta);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
