// roiaware_pool3d.hip — points in boxes and RoI-aware pooling (include/spx.h §12).  Replaces the roiaware_pool3d
// extension, reference pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu (python side roiaware_pool3d_utils.py).
//
// Pinned semantics (tests/roiaware_ref.py restates all of it in float32 numpy):
//   - inside test: `fabsf(z - cz) > dz / 2.0` (double) rejects, so a point on a z face is inside; the xy test is
//     `fabsf(local) < (double)d / 2.0 + (double)1e-5f`, in double.  The per-box limits are precomputed in double.
//   - local_x = shift_x*cosa + shift_y*(-sina), local_y = shift_x*sina + shift_y*cosa in float, FMA contraction OFF for
//     this whole file (device code contracts by default).  cosa / sina are cos(-rz) / sin(-rz) evaluated in double and
//     rounded to float once per box: a correctly rounded cosf, which is what the reference's CPU op gets from glibc.  The
//     reference's CUDA cosf may differ from it by an ulp, and whether its nvcc build contracted the local-coordinate
//     lines cannot be checked without a CUDA device: both are unpinned against the CUDA build.
//   - cell index: x_res = dx / ox, int((local_x + dx / 2) / x_res) in float, the conversion saturating (NaN -> 0), then
//     stored unsigned and clamped with an unsigned min(u, ox - 1): a negative index lands in the LAST cell.
//   - collection: each voxel keeps the first max_pts - 1 in-box points in ascending point index (the reference's serial
//     per-RoI scan), rebuilt here in parallel: per RoI one workgroup compacts each chunk of points in index order
//     (ballot + prefix), one wave ranks the compacted chunk per cell (its lanes in order, one counter add per cell), and
//     a counting sort by cell lays the kept points out cell-major.
//   - max pool: start at -inf (the reference's -1e50 in float), strict `>` in list order; no winner -> argmax -1, value 0.
//     avg pool: sum in list order from 0, then sum / count.
//   - backward: grad_in[p, c] = sum over RoIs r = 0, 1, 2, ... in ascending order, starting from 0.0f, of that RoI's
//     contribution (max: grad_out where argmax == p; avg: grad_out * (1 / fmaxf(count, 1))).  A point lies in at most one
//     voxel per RoI, so the backward is a gather: no sort, no atomics, deterministic.
#include "spx_common.h"

#pragma clang fp contract(off)

#include "box_inside.h"   // BoxC, box_consts, in_box, cell_axis: after the pragma, which covers them

namespace {

constexpr int kPibThreads = 256;     // points_in_boxes: points per workgroup = boxes staged per LDS chunk
constexpr int kColThreads = 1024;    // collection: one workgroup per RoI
constexpr int kColWaves = kColThreads / SPX_WAVE;
constexpr int kLdsCells = 8192;      // voxel counters live in LDS up to this many cells per RoI, else in vox_cnt

// ------------------------------------------------------------------------------------------- points in boxes
// grid (ceil(m / 256), b); each workgroup stages the frame's boxes 256 at a time with their constants and every thread
// scans them in ascending k, stopping at its first hit.  The workgroup leaves the chunk loop once all its points have hit.
__global__ __launch_bounds__(kPibThreads) void k_points_in_boxes(const float* __restrict__ pts,
                                                                 const float* __restrict__ boxes, int m, int t,
                                                                 int32_t* __restrict__ box_idx) {
  __shared__ BoxC s_box[kPibThreads];
  const int b = blockIdx.y, i = blockIdx.x * kPibThreads + threadIdx.x;
  const bool live = i < m;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    const float* p = pts + ((size_t)b * m + i) * 3;
    x = p[0];
    y = p[1];
    z = p[2];
  }
  const float* B = boxes + (size_t)b * t * 7;
  int hit = -1;
  for (int base = 0; base < t; base += kPibThreads) {
    if (!__syncthreads_or(live && hit < 0)) break;   // also orders the previous chunk's reads before the refill
    const int len = min(kPibThreads, t - base);
    if ((int)threadIdx.x < len) s_box[threadIdx.x] = box_consts(B + (size_t)(base + threadIdx.x) * 7);
    __syncthreads();
    if (live && hit < 0) {
      for (int k = 0; k < len; ++k) {
        float lx, ly;
        if (in_box(s_box[k], x, y, z, lx, ly)) {
          hit = base + k;
          break;
        }
      }
    }
  }
  if (live) box_idx[(size_t)b * m + i] = hit;
}

// ------------------------------------------------------------------------------------------- collection
// One workgroup per RoI r.  Writes pt_cell[r, :] (cell of each kept point, else -1), vox_cnt[r, :] (kept per cell),
// off[r, :] (exclusive scan of vox_cnt) and sorted[r, off[v] .. off[v] + vox_cnt[v]) = the kept points of cell v in
// ascending index.  rank[r, p] is scratch.  Counters: LDS when V <= kLdsCells, else vox_cnt itself (flat pointer).
__global__ __launch_bounds__(kColThreads) void k_collect(const float* __restrict__ rois, const float* __restrict__ pts,
                                                         int np, int ox, int oy, int oz, int cap,
                                                         int32_t* __restrict__ pt_cell, int32_t* __restrict__ vox_cnt,
                                                         int32_t* __restrict__ off, int32_t* __restrict__ rank,
                                                         int32_t* __restrict__ sorted) {
  extern __shared__ int32_t s_dyn[];
  __shared__ int32_t s_code[kColThreads], s_pt[kColThreads], s_w[kColWaves];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (SPX_WAVE - 1), w = tid / SPX_WAVE;
  const int V = ox * oy * oz;
  const size_t rp = (size_t)r * np, rv = (size_t)r * V;
  int32_t* cnt = V <= kLdsCells ? s_dyn : vox_cnt + rv;
  for (int v = tid; v < V; v += kColThreads) cnt[v] = 0;

  const float* R = rois + (size_t)r * 7;
  const BoxC bc = box_consts(R);
  const float dx = R[3], dy = R[4], dz = R[5];

  for (int base = 0; base < np; base += kColThreads) {
    __syncthreads();   // counters zeroed / previous chunk's walk done
    const int p = base + tid;
    int code = -1;
    if (p < np) {
      const float* q = pts + (size_t)p * 3;
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
        const int len = min(SPX_WAVE, total - j0);
        const bool v = lane < len;
        const int c = v ? s_code[j0 + lane] : -1, q = v ? s_pt[j0 + lane] : 0;
        int below = 0, last = lane;
        for (int j = 0; j < len; ++j) {
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
    int inc = x;
#pragma unroll
    for (int d = 1; d < SPX_WAVE; d <<= 1) {
      const int y = __shfl_up(inc, d);
      if (lane >= d) inc += y;
    }
    __syncthreads();
    if (lane == SPX_WAVE - 1) s_w[w] = inc;
    __syncthreads();
    int wpre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kColWaves; ++i) {
      const int c = s_w[i];
      wpre += i < w ? c : 0;
      tot += c;
    }
    if (v < V) off[rv + v] = carry + wpre + inc - x;
    carry += tot;
  }
  __syncthreads();
  for (int p = tid; p < np; p += kColThreads) {
    const int c = pt_cell[rp + p];
    if (c >= 0) sorted[rp + off[rv + c] + rank[rp + p]] = p;
  }
}

// ------------------------------------------------------------------------------------------- pooling
// one thread per (r, cell, channel); every element of pooled (and argmax for max) is written
template <bool MAX>
__global__ __launch_bounds__(256) void k_pool(const float* __restrict__ feats, const int32_t* __restrict__ vox_cnt,
                                              const int32_t* __restrict__ off, const int32_t* __restrict__ sorted,
                                              int64_t total, int V, int c, int np, float* __restrict__ pooled,
                                              int32_t* __restrict__ argmax) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int64_t rv = e / c;
    const int ch = (int)(e - rv * c);
    const int r = (int)(rv / V);
    const int n = vox_cnt[rv];
    const int32_t* L = sorted + (size_t)r * np + off[rv];
    if (MAX) {
      float best = -INFINITY;
      int am = -1;
      for (int k = 0; k < n; ++k) {
        const int p = L[k];
        const float f = feats[(size_t)p * c + ch];
        if (f > best) {
          best = f;
          am = p;
        }
      }
      pooled[e] = am != -1 ? best : 0.f;
      argmax[e] = am;
    } else {
      float s = 0.f;
      for (int k = 0; k < n; ++k) s += feats[(size_t)L[k] * c + ch];
      pooled[e] = n > 0 ? s / (float)n : 0.f;
    }
  }
}

// one thread per (point, channel): the RoIs in ascending order, from 0.0f
template <bool MAX>
__global__ __launch_bounds__(256) void k_pool_bwd(const float* __restrict__ grad_out, const int32_t* __restrict__ argmax,
                                                  const int32_t* __restrict__ pt_cell,
                                                  const int32_t* __restrict__ vox_cnt, int n, int np, int V, int c,
                                                  float* __restrict__ grad_in) {
  constexpr int U = 8;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)np * c) return;
  const int p = (int)(e / c), ch = (int)(e - (int64_t)p * c);
  float acc = 0.f;
  for (int r0 = 0; r0 < n; r0 += U) {
    int cell[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cell[u] = r0 + u < n ? pt_cell[(size_t)(r0 + u) * np + p] : -1;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (cell[u] < 0) continue;
      const size_t rv = (size_t)(r0 + u) * V + cell[u];
      const size_t o = rv * c + ch;
      if (MAX) {
        if (argmax[o] == p) acc += grad_out[o];
      } else {
        acc += grad_out[o] * (1.f / fmaxf((float)vox_cnt[rv], 1.f));
      }
    }
  }
  grad_in[e] = acc;
}

struct PoolWs {
  size_t off, rank, sorted, total;
};

PoolWs pool_ws_layout(int64_t n, int64_t np, int64_t V) {
  PoolWs l;
  l.off = 0;
  l.rank = spx_align((size_t)n * V * 4);
  l.sorted = l.rank + spx_align((size_t)n * np * 4);
  l.total = l.sorted + spx_align((size_t)n * np * 4);
  return l;
}

bool pool_dims_ok(int32_t ox, int32_t oy, int32_t oz) {
  return ox >= 1 && oy >= 1 && oz >= 1 && ox < 256 && oy < 256 && oz < 256;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int spx_points_in_boxes(const float* pts, const float* boxes, int32_t b, int64_t m, int64_t t,
                                   int32_t* box_idx, spx_stream_t stream) {
  if (b < 0 || m < 0 || t < 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || m == 0) return SPX_OK;
  if (!pts || !box_idx || (t > 0 && !boxes)) return SPX_ERR_INVALID_ARG;
  if (m >= INT32_MAX / 3 || t >= INT32_MAX / 7 || b > 65535 || (int64_t)b * m * 3 >= ((int64_t)1 << 40))
    return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_points_in_boxes, dim3((unsigned)((m + kPibThreads - 1) / kPibThreads), (unsigned)b),
                     dim3(kPibThreads), 0, spx_s(stream), pts, boxes, (int)m, (int)t, box_idx);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_roiaware_pool3d_ws_bytes(int64_t n, int64_t np, int32_t ox, int32_t oy, int32_t oz) {
  if (n <= 0 || np < 0 || !pool_dims_ok(ox, oy, oz)) return 0;
  return pool_ws_layout(n, np, (int64_t)ox * oy * oz).total;
}

extern "C" int spx_roiaware_pool3d_fwd(const float* rois, const float* pts, const float* feats, int64_t n, int64_t np,
                                       int32_t c, int32_t ox, int32_t oy, int32_t oz, int32_t max_pts, int32_t mode,
                                       float* pooled, int32_t* argmax, int32_t* pt_cell, int32_t* vox_cnt, void* ws,
                                       size_t ws_bytes, spx_stream_t stream) {
  if (n < 0 || np < 0 || c < 0 || !pool_dims_ok(ox, oy, oz) || max_pts < 1 || (mode != 0 && mode != 1))
    return SPX_ERR_INVALID_ARG;
  if (n == 0) return SPX_OK;
  const int64_t V = (int64_t)ox * oy * oz;
  if (!rois || !vox_cnt || (np > 0 && (!pts || !pt_cell)) || (c > 0 && (!pooled || (mode == 0 && !argmax))) ||
      (c > 0 && np > 0 && !feats))
    return SPX_ERR_INVALID_ARG;
  if (n >= INT32_MAX || np >= INT32_MAX / 3 || n * np >= INT32_MAX || n * V >= INT32_MAX ||
      (int64_t)np * c >= INT32_MAX || n * V * c >= ((int64_t)1 << 40))
    return SPX_ERR_TOO_LARGE;
  const PoolWs l = pool_ws_layout(n, np, V);
  if (!ws || ws_bytes < l.total) return SPX_ERR_WORKSPACE;
  char* W = (char*)ws;
  int32_t* off = (int32_t*)(W + l.off);
  int32_t* rank = (int32_t*)(W + l.rank);
  int32_t* sorted = (int32_t*)(W + l.sorted);
  hipStream_t s = spx_s(stream);
  const size_t lds = V <= kLdsCells ? (size_t)V * 4 : 0;
  hipLaunchKernelGGL(k_collect, dim3((unsigned)n), dim3(kColThreads), lds, s, rois, pts, (int)np, ox, oy, oz,
                     max_pts - 1, pt_cell, vox_cnt, off, rank, sorted);
  SPX_CHECK_LAUNCH();
  const int64_t total = n * V * c;
  if (total == 0) return SPX_OK;
  const int64_t nb64 = (total + 255) / 256;
  const unsigned nb = (unsigned)(nb64 < 65536 ? nb64 : 65536);
  if (mode == 0)
    hipLaunchKernelGGL(k_pool<true>, dim3(nb), dim3(256), 0, s, feats, vox_cnt, off, sorted, total, (int)V, c, (int)np,
                       pooled, argmax);
  else
    hipLaunchKernelGGL(k_pool<false>, dim3(nb), dim3(256), 0, s, feats, vox_cnt, off, sorted, total, (int)V, c, (int)np,
                       pooled, nullptr);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_roiaware_pool3d_bwd(const float* grad_out, const int32_t* argmax, const int32_t* pt_cell,
                                       const int32_t* vox_cnt, int64_t n, int64_t np, int32_t c, int32_t ox, int32_t oy,
                                       int32_t oz, int32_t mode, float* grad_in, spx_stream_t stream) {
  if (n < 0 || np < 0 || c < 0 || !pool_dims_ok(ox, oy, oz) || (mode != 0 && mode != 1)) return SPX_ERR_INVALID_ARG;
  if (np == 0 || c == 0) return SPX_OK;
  if (!grad_in || (n > 0 && (!grad_out || !pt_cell || (mode == 0 ? !argmax : !vox_cnt)))) return SPX_ERR_INVALID_ARG;
  const int64_t V = (int64_t)ox * oy * oz;
  if (n >= INT32_MAX || np >= INT32_MAX || n * np >= INT32_MAX || (int64_t)np * c >= INT32_MAX ||
      n * V * c >= ((int64_t)1 << 40))
    return SPX_ERR_TOO_LARGE;
  const unsigned nb = (unsigned)(((int64_t)np * c + 255) / 256);
  if (mode == 0)
    hipLaunchKernelGGL(k_pool_bwd<true>, dim3(nb), dim3(256), 0, spx_s(stream), grad_out, argmax, pt_cell, vox_cnt,
                       (int)n, (int)np, (int)V, c, grad_in);
  else
    hipLaunchKernelGGL(k_pool_bwd<false>, dim3(nb), dim3(256), 0, spx_s(stream), grad_out, argmax, pt_cell, vox_cnt,
                       (int)n, (int)np, (int)V, c, grad_in);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
