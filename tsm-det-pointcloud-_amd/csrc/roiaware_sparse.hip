// roiaware_sparse.hip — batched RoI-aware pooling that writes only the live cells (include/spx.h §30), and the ragged
// points-in-boxes.  Replaces the per-frame loop of PartA2FCHead.roiaware_pool (reference
// pcdet/models/roi_heads/partA2_head.py:104-204): two RoIAwarePool3d calls per frame over dense (N, o, o, o, C) grids,
// sum(-1).nonzero() (a host read) and the gather of the few non-empty cells.
//
// Semantics: those of the header comment of roiaware_pool3d.hip, verbatim (the inside test of box_inside.h, contraction
// off, the cell index rule, the first max_pts - 1 points per cell in ascending point index, max with strict `>` in list
// order, avg = the list-order sum divided by the count, the backward's `grad * (1 / fmaxf(count, 1))`), extended to a
// batch: RoI row r = b * N + n sees only the points of frame b, which are the rows [start_b, start_b + frame_cnt[b]) of
// `points` (start_b = the sum of the earlier counts).  tests/roiaware_sparse_ref.py restates all of it in float32 numpy.
//   - emitted cells: a cell that keeps at least one point AND whose four averaged part values have a non-zero float32
//     sum ((a0 + a1) + a2) + a3 — the reference's pooled_part_features.sum(-1).nonzero().  Defined for non-negative part
//     values, where the order of the adds cannot change whether the sum is zero.
//   - row order: ascending (r, x, y, z) = ascending (r, linear cell), the row-major order of nonzero().
//   - fake_sparse_idx: fewer than 3 emitted cells in the whole batch -> one row (r, 0, 0, 0) per RoI with that cell's
//     pooled values (zeros when it is empty), n_rows = B * N, faked = 1.  Decided on the device by the scan launch.
//   - static capacity: rows at and past n_rows are dead: features 0, cnt 0, arg -1, coords -1 (no kernel of the library
//     reads a dead row: consumers take n_rows as their live count).  n_rows > rows: SPX_ERR_CAPACITY in the status word,
//     the rows past the capacity are dropped (row_of_cell -1, so no gradient either).
// Launches: collect (one workgroup per RoI), scan (one workgroup), emit (one workgroup per RoI, a wave per emitted row,
// its lanes over the 4 + C channels so each listed point row is read coalesced, plus the workgroups that fill the dead
// rows); backward: one launch per feature tensor, one thread per (point, channel) walking its frame's RoIs in ascending
// r from 0.0f.  Integer atomics only (the per-cell counters), no float atomics, no host read, bitwise reproducible.
#include "spx_common.h"

#pragma clang fp contract(off)

#include "box_inside.h"   // BoxC, box_consts, in_box, cell_axis: after the pragma, which covers them

namespace {

constexpr int kPibThreads = 256;     // points_in_boxes_stack: points per workgroup = boxes staged per LDS chunk
constexpr int kColThreads = 1024;    // collection: one workgroup per RoI
constexpr int kColWaves = kColThreads / SPX_WAVE;
constexpr int kLdsCells = 8192;      // cell counters live in LDS up to this many cells per RoI, else in vox_cnt
constexpr int kEmitThreads = 256;
constexpr int kEmitWaves = kEmitThreads / SPX_WAVE;
constexpr int kMaxFrames = 256;      // every thread sums the earlier frames' counts
constexpr int64_t kMaxRois = 1 << 20;   // the single-workgroup scan walks them 1024 at a time

// The rows of frame b: [start, start + len), clamped into [0, np] and to pf rows whatever the counts hold.  ok = the
// counts were non-negative, fit into np and the frame into pf.
__device__ __forceinline__ void frame_span(const int32_t* __restrict__ frame_cnt, int b, int np, int pf, int& start,
                                           int& len, bool& ok) {
  int64_t s = 0;
  bool good = true;
  for (int i = 0; i < b; ++i) {
    const int c = frame_cnt[i];
    good = good && c >= 0;
    s += c > 0 ? c : 0;
  }
  const int c = frame_cnt[b];
  good = good && c >= 0 && s + (c > 0 ? c : 0) <= (int64_t)np;
  start = (int)(s < (int64_t)np ? s : (int64_t)np);
  int l = c > 0 ? c : 0;
  l = min(l, np - start);
  good = good && l <= pf;
  len = min(l, pf);
  ok = good;
}

// exclusive scan of x over the 1024 threads of a collection workgroup; tot = the workgroup's sum (s_w: kColWaves words)
__device__ __forceinline__ int scan_1024(int x, int lane, int w, int32_t* s_w, int& tot) {
  int inc = x;
#pragma unroll
  for (int d = 1; d < SPX_WAVE; d <<= 1) {
    const int y = __shfl_up(inc, d);
    if (lane >= d) inc += y;
  }
  __syncthreads();
  if (lane == SPX_WAVE - 1) s_w[w] = inc;
  __syncthreads();
  int wpre = 0;
  tot = 0;
#pragma unroll
  for (int i = 0; i < kColWaves; ++i) {
    const int c = s_w[i];
    wpre += i < w ? c : 0;
    tot += c;
  }
  return wpre + inc - x;
}

// ------------------------------------------------------------------------------------------- ragged points in boxes
// grid ceil(p / 256); a workgroup's points may lie in several frames: it walks the frames between its lowest and its
// highest, staging each frame's boxes 256 at a time; a thread scans the chunks of its own frame only, in ascending k,
// stopping at its first hit.  A frame index outside [0, b) gives -1.
__global__ __launch_bounds__(kPibThreads) void k_pib_stack(const float* __restrict__ pts, const float* __restrict__ boxes,
                                                           int np, int nb, int t, int32_t* __restrict__ box_idx) {
  __shared__ BoxC s_box[kPibThreads];
  __shared__ int s_lo, s_hi;
  const int i = blockIdx.x * kPibThreads + threadIdx.x;
  const bool live = i < np;
  float x = 0.f, y = 0.f, z = 0.f;
  int f = -1;
  if (live) {
    const float* p = pts + (size_t)i * 4;
    const float fb = p[0];
    if (fb >= 0.f && fb < (float)nb) f = (int)fb;
    x = p[1];
    y = p[2];
    z = p[3];
  }
  if (threadIdx.x == 0) {
    s_lo = INT32_MAX;
    s_hi = -1;
  }
  __syncthreads();
  if (f >= 0) {
    atomicMin(&s_lo, f);
    atomicMax(&s_hi, f);
  }
  __syncthreads();
  const int lo = s_lo, hi = s_hi;
  int hit = -1;
  for (int fr = lo; fr <= hi; ++fr) {
    const float* B = boxes + (size_t)fr * t * 7;
    for (int base = 0; base < t; base += kPibThreads) {
      if (!__syncthreads_or(f == fr && hit < 0)) break;   // also orders the previous chunk's reads before the refill
      const int len = min(kPibThreads, t - base);
      if ((int)threadIdx.x < len) s_box[threadIdx.x] = box_consts(B + (size_t)(base + threadIdx.x) * 7);
      __syncthreads();
      if (f == fr && hit < 0) {
        for (int k = 0; k < len; ++k) {
          float lx, ly;
          if (in_box(s_box[k], x, y, z, lx, ly)) {
            hit = base + k;
            break;
          }
        }
      }
    }
  }
  if (live) box_idx[i] = hit;
}

// ------------------------------------------------------------------------------------------- collection
// One workgroup per RoI r of frame b = r / n_per.  Over the frame's rows, by LOCAL index q = p - start: pt_cell[r, q]
// (cell of each kept point, else -1), vox_cnt[r, :] (kept per cell), off[r, :] (exclusive scan of vox_cnt),
// sorted[r, off[v] .. off[v] + vox_cnt[v]) = the kept points of cell v as GLOBAL rows in ascending order, loc[r, v] = the
// rank of cell v among the RoI's emitted cells (-1: not emitted) and n_emit[r].  rank[r, q] is scratch.  Counters: LDS
// when V <= kLdsCells, else vox_cnt itself.
__global__ __launch_bounds__(kColThreads) void k_sp_collect(
    const float* __restrict__ rois, const float* __restrict__ pts, const int32_t* __restrict__ frame_cnt,
    const float* __restrict__ part, int n_per, int np, int pf, int ox, int oy, int oz, int cap,
    int32_t* __restrict__ pt_cell, int32_t* __restrict__ vox_cnt, int32_t* __restrict__ off, int32_t* __restrict__ rank,
    int32_t* __restrict__ sorted, int32_t* __restrict__ loc, int32_t* __restrict__ n_emit, int32_t* d_status) {
  extern __shared__ int32_t s_dyn[];
  __shared__ int32_t s_code[kColThreads], s_pt[kColThreads], s_w[kColWaves];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (SPX_WAVE - 1), w = tid / SPX_WAVE;
  const int V = ox * oy * oz;
  const size_t rp = (size_t)r * pf, rv = (size_t)r * V;
  int32_t* cnt = V <= kLdsCells ? s_dyn : vox_cnt + rv;
  for (int v = tid; v < V; v += kColThreads) cnt[v] = 0;

  int start, len;
  bool ok;
  frame_span(frame_cnt, r / n_per, np, pf, start, len, ok);
  if (!ok && tid == 0 && d_status) atomicMin(d_status, (int32_t)SPX_ERR_CAPACITY);

  const float* R = rois + (size_t)r * 7;
  const BoxC bc = box_consts(R);
  const float dx = R[3], dy = R[4], dz = R[5];

  for (int base = 0; base < len; base += kColThreads) {
    __syncthreads();   // counters zeroed / previous chunk's walk done
    const int p = base + tid;
    int code = -1;
    if (p < len) {
      const float* q = pts + (size_t)(start + p) * 4 + 1;
      float lx, ly;
      if (in_box(bc, q[0], q[1], q[2], lx, ly)) {
        const float lz = q[2] - bc.cz;
        code = (int)((cell_axis(lx, dx, ox) * (unsigned)oy + cell_axis(ly, dy, oy)) * (unsigned)oz +
                     cell_axis(lz, dz, oz));
      } else {
        pt_cell[rp + p] = -1;
      }
    }
    const uint64_t bal = __ballot(code >= 0);
    if (lane == 0) s_w[w] = __popcll(bal);
    __syncthreads();
    int pre = 0, total = 0;
#pragma unroll
    for (int i = 0; i < kColWaves; ++i) {
      const int c = s_w[i];
      pre += i < w ? c : 0;
      total += c;
    }
    if (code >= 0) {
      const int pos = pre + __popcll(bal & ((1ull << lane) - 1));
      s_code[pos] = code;
      s_pt[pos] = p;
    }
    __syncthreads();
    if (w == 0) {   // wave 0 ranks the compacted chunk, 64 entries at a time, in index order
      for (int j0 = 0; j0 < total; j0 += SPX_WAVE) {
        const int n = min(SPX_WAVE, total - j0);
        const bool v = lane < n;
        const int c = v ? s_code[j0 + lane] : -1, q = v ? s_pt[j0 + lane] : 0;
        int below = 0, last = lane;
        for (int j = 0; j < n; ++j) {
          const int cj = __builtin_amdgcn_readlane(c, j);
          if (cj == c) {
            below += j < lane ? 1 : 0;
            last = j > lane ? j : last;
          }
        }
        int old = 0;
        if (v && last == lane) old = atomicAdd(cnt + c, below + 1);   // the group's last lane adds the group size
        old = __shfl(old, last);
        if (v) {
          const int k = old + below;
          const bool keep = k < cap;
          pt_cell[rp + q] = keep ? c : -1;
          if (keep) rank[rp + q] = k;
        }
      }
    }
  }
  __syncthreads();

  // cap the counters, write vox_cnt, exclusive scan into off
  int carry = 0;
  for (int v0 = 0; v0 < V; v0 += kColThreads) {
    const int v = v0 + tid;
    int x = 0;
    if (v < V) {
      x = min(cnt[v], cap);
      vox_cnt[rv + v] = x;
    }
    int tot;
    const int ex = scan_1024(x, lane, w, s_w, tot);
    if (v < V) off[rv + v] = carry + ex;
    carry += tot;
  }
  __syncthreads();
  for (int p = tid; p < len; p += kColThreads) {
    const int c = pt_cell[rp + p];
    if (c >= 0) sorted[rp + off[rv + c] + rank[rp + p]] = start + p;
  }
  __syncthreads();

  // which cells are emitted: the part averages as the avg pool forms them, their sum, and each emitted cell's rank
  carry = 0;
  for (int v0 = 0; v0 < V; v0 += kColThreads) {
    const int v = v0 + tid;
    int e = 0;
    if (v < V) {
      const int n = vox_cnt[rv + v];
      if (n > 0) {
        const int32_t* L = sorted + rp + off[rv + v];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int k = 0; k < n; ++k) {
          const float* f = part + (size_t)L[k] * 4;
          s0 += f[0];
          s1 += f[1];
          s2 += f[2];
          s3 += f[3];
        }
        const float fn = (float)n;
        const float sum = ((s0 / fn + s1 / fn) + s2 / fn) + s3 / fn;
        e = sum != 0.f ? 1 : 0;
      }
    }
    int tot;
    const int ex = scan_1024(e, lane, w, s_w, tot);
    if (v < V) loc[rv + v] = e ? carry + ex : -1;
    carry += tot;
  }
  if (tid == 0) n_emit[r] = carry;
}

// ------------------------------------------------------------------------------------------- scan
// One workgroup: base[r] = the emitted cells of the RoIs before r, the total, the fake decision and n_rows.
__global__ __launch_bounds__(kColThreads) void k_sp_scan(const int32_t* __restrict__ n_emit, int n,
                                                         int32_t* __restrict__ base, int64_t* __restrict__ n_rows,
                                                         int32_t* __restrict__ faked) {
  __shared__ int32_t s_w[kColWaves];
  const int tid = threadIdx.x, lane = tid & (SPX_WAVE - 1), w = tid / SPX_WAVE;
  int carry = 0;
  for (int r0 = 0; r0 < n; r0 += kColThreads) {
    const int r = r0 + tid;
    const int x = r < n ? n_emit[r] : 0;
    int tot;
    const int ex = scan_1024(x, lane, w, s_w, tot);
    if (r < n) base[r] = carry + ex;
    carry += tot;
  }
  if (tid == 0) {
    const bool fake = carry < 3;
    *faked = fake ? 1 : 0;
    *n_rows = fake ? (int64_t)n : (int64_t)carry;
  }
}

// ------------------------------------------------------------------------------------------- emit
// Workgroups [0, n): RoI r.  Each wave takes 64 cells at a time, turns their ranks into rows (base[r] + rank; the fake
// branch: cell 0 -> row r), writes row_of_cell, and then handles the emitted ones among them one after the other: lane j
// of the wave owns channel j of the 4 part (avg) + c rpn (max) channels, so a listed point's row is one coalesced read.
// Workgroups [n, gridDim): the dead rows [min(n_rows, rows), rows).
__global__ __launch_bounds__(kEmitThreads) void k_sp_emit(
    const float* __restrict__ part, const float* __restrict__ rpn, const int32_t* __restrict__ vox_cnt,
    const int32_t* __restrict__ off, const int32_t* __restrict__ sorted, const int32_t* __restrict__ loc,
    const int32_t* __restrict__ base, const int64_t* __restrict__ n_rows, const int32_t* __restrict__ faked, int n,
    int pf, int ox, int oy, int oz, int c, int64_t rows, int32_t* __restrict__ row_of_cell, int32_t* __restrict__ coords,
    float* __restrict__ out_part, float* __restrict__ out_rpn, int32_t* __restrict__ arg, int32_t* __restrict__ out_cnt,
    int32_t* d_status) {
  const int tid = threadIdx.x, lane = tid & (SPX_WAVE - 1), w = tid / SPX_WAVE;
  const int V = ox * oy * oz, W = c + 4;
  const int64_t total = *n_rows;
  if ((int)blockIdx.x >= n) {   // dead rows
    const int64_t live = total < rows ? total : rows;
    const int64_t cells = (rows - live) * W;
    const int64_t stride = (int64_t)(gridDim.x - n) * kEmitThreads;
    for (int64_t e = (int64_t)(blockIdx.x - n) * kEmitThreads + tid; e < cells; e += stride) {
      const int64_t row = live + e / W;
      const int j = (int)(e % W);
      if (j < 4) {
        out_part[row * 4 + j] = 0.f;
        coords[row * 4 + j] = -1;
        if (j == 0) out_cnt[row] = 0;
      } else {
        out_rpn[row * c + (j - 4)] = 0.f;
        arg[row * c + (j - 4)] = -1;
      }
    }
    return;
  }
  const int r = blockIdx.x;
  if (r == 0 && tid == 0 && total > rows && d_status) atomicMin(d_status, (int32_t)SPX_ERR_CAPACITY);
  const bool fake = *faked != 0;
  const size_t rp = (size_t)r * pf, rv = (size_t)r * V;
  const int64_t b0 = fake ? 0 : (int64_t)base[r];
  for (int c0 = w * SPX_WAVE; c0 < V; c0 += kEmitWaves * SPX_WAVE) {
    const int v = c0 + lane;
    int64_t row = -1;
    if (v < V) {
      if (fake) {
        row = v == 0 ? (int64_t)r : -1;
      } else {
        const int l = loc[rv + v];
        row = l >= 0 ? b0 + l : -1;
      }
      if (row >= rows) row = -1;
      row_of_cell[rv + v] = (int32_t)row;
    }
    uint64_t bal = __ballot(row >= 0);
    while (bal) {
      const int j = __ffsll((unsigned long long)bal) - 1;
      bal &= bal - 1;
      const int64_t orow = __shfl((int)row, j);
      const int cell = c0 + j;
      const int cn = vox_cnt[rv + cell];
      const int32_t* L = sorted + rp + off[rv + cell];
      for (int j0 = 0; j0 < W; j0 += SPX_WAVE) {
        const int ch = j0 + lane;
        if (ch >= W) break;
        const bool is_part = ch < 4;
        const float* src = is_part ? part + ch : rpn + (ch - 4);
        const int ld = is_part ? 4 : c;
        float s = 0.f, best = -INFINITY;
        int am = -1;
        for (int k = 0; k < cn; ++k) {
          const int p = L[k];
          const float f = src[(size_t)p * ld];
          s += f;
          if (f > best) {
            best = f;
            am = p;
          }
        }
        if (is_part) {
          out_part[orow * 4 + ch] = cn > 0 ? s / (float)cn : 0.f;
        } else {
          out_rpn[orow * c + (ch - 4)] = am != -1 ? best : 0.f;
          arg[orow * c + (ch - 4)] = am;
        }
      }
      if (lane == 0) {
        const int x = cell / (oy * oz), yz = cell - x * (oy * oz);
        int32_t* co = coords + orow * 4;
        co[0] = r;
        co[1] = x;
        co[2] = yz / oz;
        co[3] = yz % oz;
        out_cnt[orow] = cn;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- backward
// one thread per (point, channel): the RoIs of the point's frame in ascending order, from 0.0f
template <bool MAX>
__global__ __launch_bounds__(256) void k_sp_bwd(const float* __restrict__ grad, const int32_t* __restrict__ arg,
                                                const int32_t* __restrict__ out_cnt,
                                                const int32_t* __restrict__ row_of_cell,
                                                const int32_t* __restrict__ pt_cell,
                                                const int32_t* __restrict__ frame_cnt, int nb, int n_per, int np, int pf,
                                                int V, int c, int64_t rows, float* __restrict__ grad_in) {
  constexpr int U = 8;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)np * c) return;
  const int p = (int)(e / c), ch = (int)(e - (int64_t)p * c);
  // the frame whose span holds p (frame_span's clamps, so pt_cell is read only where the collection wrote it)
  int b = -1, q = 0;
  int64_t s = 0;
  for (int i = 0; i < nb; ++i) {
    const int ci = frame_cnt[i];
    const int64_t cc = ci > 0 ? ci : 0;
    const int64_t st = s < (int64_t)np ? s : (int64_t)np;
    int64_t l = cc < (int64_t)np - st ? cc : (int64_t)np - st;
    l = l < pf ? l : pf;
    if ((int64_t)p >= st && (int64_t)p < st + l) {
      b = i;
      q = (int)(p - st);
      break;
    }
    s += cc;
  }
  float acc = 0.f;
  if (b >= 0) {
    const int r_lo = b * n_per, r_hi = r_lo + n_per;
    for (int r0 = r_lo; r0 < r_hi; r0 += U) {
      int cell[U];
#pragma unroll
      for (int u = 0; u < U; ++u) cell[u] = r0 + u < r_hi ? pt_cell[(size_t)(r0 + u) * pf + q] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (cell[u] < 0) continue;
        const int64_t row = row_of_cell[(size_t)(r0 + u) * V + cell[u]];
        if (row < 0 || row >= rows) continue;
        const size_t o = (size_t)row * c + ch;
        if (MAX) {
          if (arg[o] == p) acc += grad[o];
        } else {
          acc += grad[o] * (1.f / fmaxf((float)out_cnt[row], 1.f));
        }
      }
    }
  }
  grad_in[e] = acc;
}

struct SparseWs {
  size_t pt_cell, rank, sorted, vox_cnt, off, loc, n_emit, base, total;
};

SparseWs sparse_ws_layout(int64_t n, int64_t pf, int64_t V) {
  SparseWs l;
  const size_t a = spx_align((size_t)n * pf * 4), b = spx_align((size_t)n * V * 4), c = spx_align((size_t)n * 4);
  l.pt_cell = 0;
  l.rank = l.pt_cell + a;
  l.sorted = l.rank + a;
  l.vox_cnt = l.sorted + a;
  l.off = l.vox_cnt + b;
  l.loc = l.off + b;
  l.n_emit = l.loc + b;
  l.base = l.n_emit + c;
  l.total = l.base + c;
  return l;
}

bool pool_dims_ok(int32_t ox, int32_t oy, int32_t oz) {
  return ox >= 1 && oy >= 1 && oz >= 1 && ox < 256 && oy < 256 && oz < 256;
}

// the limits of §30; n = b * n_per RoI rows
int sparse_limits(int32_t b, int64_t n_per, int64_t np, int64_t pf, int64_t V) {
  if (b > kMaxFrames) return SPX_ERR_TOO_LARGE;
  const int64_t n = (int64_t)b * n_per;
  if (n_per >= INT32_MAX || n > kMaxRois || np >= INT32_MAX / 4 || pf >= INT32_MAX / 4 || n * (pf > 0 ? pf : 1) >= INT32_MAX ||
      n * V >= INT32_MAX)
    return SPX_ERR_TOO_LARGE;
  return SPX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int spx_points_in_boxes_stack(const float* points, const float* boxes, int32_t b, int64_t np, int64_t t,
                                         int32_t* box_idx, spx_stream_t stream) {
  if (b < 0 || np < 0 || t < 0) return SPX_ERR_INVALID_ARG;
  if (np == 0) return SPX_OK;
  if (!points || !box_idx || (b > 0 && t > 0 && !boxes)) return SPX_ERR_INVALID_ARG;
  if (np >= INT32_MAX / 4 || t >= INT32_MAX / 7 || b > 65535 || (int64_t)b * t * 7 >= ((int64_t)1 << 40))
    return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_pib_stack, dim3((unsigned)((np + kPibThreads - 1) / kPibThreads)), dim3(kPibThreads), 0,
                     spx_s(stream), points, boxes, (int)np, (int)b, (int)t, box_idx);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_roiaware_sparse_ws_bytes(int32_t b, int64_t n_per, int64_t pf, int32_t ox, int32_t oy, int32_t oz) {
  if (b <= 0 || n_per <= 0 || pf < 0 || !pool_dims_ok(ox, oy, oz)) return 0;
  return sparse_ws_layout((int64_t)b * n_per, pf, (int64_t)ox * oy * oz).total;
}

extern "C" int spx_roiaware_sparse_collect(const float* rois, const float* points, const int32_t* frame_cnt,
                                           const float* part, int32_t b, int64_t n_per, int64_t np, int64_t pf,
                                           int32_t ox, int32_t oy, int32_t oz, int32_t max_pts, int64_t* n_rows,
                                           int32_t* faked, int32_t* d_status, void* ws, size_t ws_bytes,
                                           spx_stream_t stream) {
  if (b < 0 || n_per < 0 || np < 0 || pf < 0 || !pool_dims_ok(ox, oy, oz) || max_pts < 1 || !n_rows || !faked)
    return SPX_ERR_INVALID_ARG;
  hipStream_t s = spx_s(stream);
  const int64_t n = (int64_t)b * n_per, V = (int64_t)ox * oy * oz;
  if (n == 0) {   // no RoI: no row, nothing faked
    spx_fill_async(n_rows, 0, 8, s);
    spx_fill_async(faked, 0, 4, s);
    SPX_CHECK_LAUNCH();
    return SPX_OK;
  }
  if (!rois || !frame_cnt || (np > 0 && (!points || !part))) return SPX_ERR_INVALID_ARG;
  const int lim = sparse_limits(b, n_per, np, pf, V);
  if (lim != SPX_OK) return lim;
  const SparseWs l = sparse_ws_layout(n, pf, V);
  if (!ws || ws_bytes < l.total) return SPX_ERR_WORKSPACE;
  char* Wp = (char*)ws;
  const size_t lds = V <= kLdsCells ? (size_t)V * 4 : 0;
  hipLaunchKernelGGL(k_sp_collect, dim3((unsigned)n), dim3(kColThreads), lds, s, rois, points, frame_cnt, part,
                     (int)n_per, (int)np, (int)pf, ox, oy, oz, max_pts - 1, (int32_t*)(Wp + l.pt_cell),
                     (int32_t*)(Wp + l.vox_cnt), (int32_t*)(Wp + l.off), (int32_t*)(Wp + l.rank),
                     (int32_t*)(Wp + l.sorted), (int32_t*)(Wp + l.loc), (int32_t*)(Wp + l.n_emit), d_status);
  SPX_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(kColThreads), 0, s, (const int32_t*)(Wp + l.n_emit), (int)n,
                     (int32_t*)(Wp + l.base), n_rows, faked);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_roiaware_sparse_pool(const float* part, const float* rpn, int32_t b, int64_t n_per, int64_t np,
                                        int64_t pf, int32_t c, int32_t ox, int32_t oy, int32_t oz, int64_t rows,
                                        const int64_t* n_rows, const int32_t* faked, int32_t* row_of_cell,
                                        int32_t* coords, float* out_part, float* out_rpn, int32_t* arg, int32_t* cnt,
                                        int32_t* d_status, const void* ws, size_t ws_bytes, spx_stream_t stream) {
  if (b < 0 || n_per < 0 || np < 0 || pf < 0 || c < 0 || rows < 0 || !pool_dims_ok(ox, oy, oz)) return SPX_ERR_INVALID_ARG;
  const int64_t n = (int64_t)b * n_per, V = (int64_t)ox * oy * oz;
  if (n == 0) return SPX_OK;
  if (!n_rows || !faked || !row_of_cell || (np > 0 && (!part || (c > 0 && !rpn))) ||
      (rows > 0 && (!coords || !out_part || !cnt || (c > 0 && (!out_rpn || !arg)))))
    return SPX_ERR_INVALID_ARG;
  const int lim = sparse_limits(b, n_per, np, pf, V);
  if (lim != SPX_OK) return lim;
  if (rows >= INT32_MAX / 4 || rows * (c > 0 ? c : 1) >= INT32_MAX || (int64_t)np * (c > 0 ? c : 1) >= INT32_MAX)
    return SPX_ERR_TOO_LARGE;
  const SparseWs l = sparse_ws_layout(n, pf, V);
  if (!ws || ws_bytes < l.total) return SPX_ERR_WORKSPACE;
  const char* Wp = (const char*)ws;
  const int64_t fill64 = (rows * (c + 4) + kEmitThreads - 1) / kEmitThreads;
  const unsigned nfill = (unsigned)(fill64 < 1024 ? fill64 : 1024);
  hipLaunchKernelGGL(k_sp_emit, dim3((unsigned)n + nfill), dim3(kEmitThreads), 0, spx_s(stream), part, rpn,
                     (const int32_t*)(Wp + l.vox_cnt), (const int32_t*)(Wp + l.off), (const int32_t*)(Wp + l.sorted),
                     (const int32_t*)(Wp + l.loc), (const int32_t*)(Wp + l.base), n_rows, faked, (int)n, (int)pf, ox, oy,
                     oz, c, rows, row_of_cell, coords, out_part, out_rpn, arg, cnt, d_status);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_roiaware_sparse_bwd(const float* grad, const int32_t* arg, const int32_t* cnt,
                                       const int32_t* row_of_cell, const int32_t* frame_cnt, int32_t b, int64_t n_per,
                                       int64_t np, int64_t pf, int32_t c, int32_t ox, int32_t oy, int32_t oz, int64_t rows,
                                       int32_t mode, float* grad_in, const void* ws, size_t ws_bytes,
                                       spx_stream_t stream) {
  if (b < 0 || n_per < 0 || np < 0 || pf < 0 || c < 0 || rows < 0 || !pool_dims_ok(ox, oy, oz) || (mode != 0 && mode != 1))
    return SPX_ERR_INVALID_ARG;
  if (np == 0 || c == 0) return SPX_OK;
  if (!grad_in) return SPX_ERR_INVALID_ARG;
  const int64_t n = (int64_t)b * n_per, V = (int64_t)ox * oy * oz;
  if ((int64_t)np * c >= INT32_MAX || rows * c >= INT32_MAX) return SPX_ERR_TOO_LARGE;
  hipStream_t s = spx_s(stream);
  if (n == 0 || rows == 0) {
    spx_fill_async(grad_in, 0, (size_t)np * c * 4, s);
    SPX_CHECK_LAUNCH();
    return SPX_OK;
  }
  if (!grad || !row_of_cell || !frame_cnt || (mode == 0 ? !arg : !cnt)) return SPX_ERR_INVALID_ARG;
  const int lim = sparse_limits(b, n_per, np, pf, V);
  if (lim != SPX_OK) return lim;
  const SparseWs l = sparse_ws_layout(n, pf, V);
  if (!ws || ws_bytes < l.total) return SPX_ERR_WORKSPACE;
  const int32_t* pt_cell = (const int32_t*)((const char*)ws + l.pt_cell);
  const unsigned nblk = (unsigned)(((int64_t)np * c + 255) / 256);
  if (mode == 0)
    hipLaunchKernelGGL(k_sp_bwd<true>, dim3(nblk), dim3(256), 0, s, grad, arg, cnt, row_of_cell, pt_cell, frame_cnt,
                       (int)b, (int)n_per, (int)np, (int)pf, (int)V, c, rows, grad_in);
  else
    hipLaunchKernelGGL(k_sp_bwd<false>, dim3(nblk), dim3(256), 0, s, grad, arg, cnt, row_of_cell, pt_cell, frame_cnt,
                       (int)b, (int)n_per, (int)np, (int)pf, (int)V, c, rows, grad_in);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
