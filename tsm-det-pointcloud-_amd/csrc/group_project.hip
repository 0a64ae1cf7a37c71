// group_project.hip — the first 1x1 conv of a PointNet++ set-abstraction grouper, fused with the grouping that feeds it
// (include/spx.h §13).  The reference (pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py, the voxel-point SA
// modules) materialises the grouped tensor (B, 3 + C, npoint, nsample) — gather, subtract the centre, cat xyz and
// features, zero empty balls, permute — and only then runs Conv2d(k=1).  Here the feature half of that conv is a GEMM
// over the SOURCE rows, P = F · Wf^T (the caller's, 8x fewer rows than gathered columns), and this file does the rest:
//
//   Y[b, o, p, s] = empty[m] ? 0 : P[r, o] + sum_j Wx[o, j] * (xyz[r, j] - ctr[m, j]),   m = b * npoint + p,
//                                                                                          r = idx[m, s]
//
// The xyz term stays relative: folding Wx·xyz into P would subtract two ~70 m products to get a ~1 m one.
// Backward, deterministic (no float atomics):
//   dP^T[o, r] = sum of dY[m, s, o] over the live (m, s) with idx = r: sorted runs by r (sorted_runs.h), then every
//                (o, r) adds its run in ascending entry order;
//   dWx[o, j]  = sum over live columns of dY * rel: each block sums a fixed chunk of columns (wave shuffles, then the
//                four waves in order), one block per output then adds the per-block partials in a fixed order.
// dWx is a K = 3 GEMM over ~2 M columns: memory bound on reading dY, and a 16x16x4 f32 MFMA would use 3 of its 16 N
// columns, so it stays on the VALU.
#include "block_ops.h"
#include "sorted_runs.h"

namespace {

constexpr int kThreads = 256;
constexpr int kColsPerThread = 8;                        // dWx: columns per thread per block
constexpr int kColsPerBlock = kThreads * kColsPerThread;
constexpr int kOTile = 128;                              // dWx: outputs reduced per LDS round

struct Geom {
  int64_t total;      // b * npoint * nsample columns
  int64_t per_frame;  // npoint * nsample
  int nsample;
  int c_out;
  int64_t n_src;
};

// column -> offset of Y[b, 0, p, s]; add o * per_frame for channel o
__device__ __forceinline__ size_t y_base(const Geom& g, int64_t col) {
  const int64_t b = col / g.per_frame;
  return (size_t)b * g.c_out * g.per_frame + (size_t)(col - b * g.per_frame);
}

// source row of a column, or -1 if the column is empty (empty ball or row outside [0, n_src))
__device__ __forceinline__ int64_t live_row(const Geom& g, const int32_t* __restrict__ idx,
                                            const uint8_t* __restrict__ empty, int64_t col) {
  const int64_t m = col / g.nsample;
  const int32_t r = idx[col];
  if ((empty && empty[m]) || r < 0 || (int64_t)r >= g.n_src) return -1;
  return r;
}

template <bool HP, bool HX, bool V4>
__global__ __launch_bounds__(kThreads) void k_group_project(const float* __restrict__ p, const float* __restrict__ wx,
                                                            const float* __restrict__ xyz, const float* __restrict__ ctr,
                                                            const int32_t* __restrict__ idx,
                                                            const uint8_t* __restrict__ empty, Geom g,
                                                            float* __restrict__ y) {
  const int64_t col = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (col >= g.total) return;
  const int64_t r = live_row(g, idx, empty, col);
  float* yc = y + y_base(g, col);
  const size_t pf = (size_t)g.per_frame;
  if (r < 0) {
    for (int o = 0; o < g.c_out; ++o) yc[o * pf] = 0.f;
    return;
  }
  float rx = 0.f, ry = 0.f, rz = 0.f;
  if (HX) {
    const int64_t m = col / g.nsample;
    rx = xyz[r * 3 + 0] - ctr[m * 3 + 0];
    ry = xyz[r * 3 + 1] - ctr[m * 3 + 1];
    rz = xyz[r * 3 + 2] - ctr[m * 3 + 2];
  }
  const float* pr = HP ? p + (size_t)r * g.c_out : nullptr;
  auto one = [&](int o, float pv) {
    float v = pv;
    if (HX) v += wx[o * 3 + 0] * rx + wx[o * 3 + 1] * ry + wx[o * 3 + 2] * rz;
    yc[o * pf] = v;
  };
  if (V4) {
    for (int o = 0; o < g.c_out; o += 4) {
      float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (HP) pv = *reinterpret_cast<const float4*>(pr + o);
      one(o, pv.x);
      one(o + 1, pv.y);
      one(o + 2, pv.z);
      one(o + 3, pv.w);
    }
  } else {
    for (int o = 0; o < g.c_out; ++o) one(o, HP ? pr[o] : 0.f);
  }
}

// ---------------------------------------------------------------------------------------------- dP^T
__global__ __launch_bounds__(kThreads) void k_gp_keys(const int32_t* __restrict__ idx, const uint8_t* __restrict__ empty,
                                                      Geom g, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t col = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (col >= g.total) return;
  const int64_t r = live_row(g, idx, empty, col);
  keys[col] = r < 0 ? (uint32_t)g.n_src : (uint32_t)r;
  vals[col] = (uint32_t)col;
}

// dpt[o][r] = sum over r's sorted run of dY at (o, column), in ascending column order
__global__ __launch_bounds__(kThreads) void k_gp_dp(const float* __restrict__ dy, const uint32_t* __restrict__ vals,
                                                    const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                                                    Geom g, float* __restrict__ dpt) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int o = blockIdx.y;
  if (r >= g.n_src) return;
  const int32_t s = start[r], e = end[r];
  const size_t off = (size_t)o * g.per_frame;
  float acc = 0.f;
  for (int32_t q = s; q < e; ++q) acc += dy[y_base(g, vals[q]) + off];
  dpt[(size_t)o * g.n_src + r] = acc;
}

// ---------------------------------------------------------------------------------------------- dWx
// part[blk][o][j] = sum over the block's columns of dY[o, col] * rel[col, j]
__global__ __launch_bounds__(kThreads) void k_gp_dwx_part(const float* __restrict__ dy, const float* __restrict__ xyz,
                                                          const float* __restrict__ ctr, const int32_t* __restrict__ idx,
                                                          const uint8_t* __restrict__ empty, Geom g,
                                                          float* __restrict__ part) {
  __shared__ float s_w[kThreads / SPX_WAVE][kOTile * 3];
  const int tid = threadIdx.x, wave = tid / SPX_WAVE, lane = tid % SPX_WAVE;
  const int64_t base = (int64_t)blockIdx.x * kColsPerBlock;
  size_t yb[kColsPerThread];
  float rel[kColsPerThread][3];
#pragma unroll
  for (int i = 0; i < kColsPerThread; ++i) {
    const int64_t col = base + (int64_t)i * kThreads + tid;
    yb[i] = 0;
    rel[i][0] = rel[i][1] = rel[i][2] = 0.f;
    if (col < g.total) {
      const int64_t r = live_row(g, idx, empty, col);
      yb[i] = y_base(g, col);
      if (r >= 0) {
        const int64_t m = col / g.nsample;
        rel[i][0] = xyz[r * 3 + 0] - ctr[m * 3 + 0];
        rel[i][1] = xyz[r * 3 + 1] - ctr[m * 3 + 1];
        rel[i][2] = xyz[r * 3 + 2] - ctr[m * 3 + 2];
      }
    }
  }
  const size_t pf = (size_t)g.per_frame;
  float* out = part + (size_t)blockIdx.x * g.c_out * 3;
  for (int o0 = 0; o0 < g.c_out; o0 += kOTile) {
    const int nt = min(kOTile, g.c_out - o0);
    for (int t = 0; t < nt; ++t) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int i = 0; i < kColsPerThread; ++i) {
        const int64_t col = base + (int64_t)i * kThreads + tid;
        const float d = col < g.total ? dy[yb[i] + (size_t)(o0 + t) * pf] : 0.f;
        a0 += d * rel[i][0];
        a1 += d * rel[i][1];
        a2 += d * rel[i][2];
      }
      a0 = spx_wave_sum(a0);
      a1 = spx_wave_sum(a1);
      a2 = spx_wave_sum(a2);
      if (lane == 0) {
        s_w[wave][t * 3 + 0] = a0;
        s_w[wave][t * 3 + 1] = a1;
        s_w[wave][t * 3 + 2] = a2;
      }
    }
    __syncthreads();
    for (int q = tid; q < nt * 3; q += kThreads) {
      float v = s_w[0][q];
#pragma unroll
      for (int w = 1; w < kThreads / SPX_WAVE; ++w) v += s_w[w][q];
      out[(size_t)o0 * 3 + q] = v;
    }
    __syncthreads();
  }
}

struct BwdWs : SortedRunsWs {
  float* part;   // dWx: [dwx_blocks][c_out][3]
};

int64_t dwx_blocks(int64_t total) { return (total + kColsPerBlock - 1) / kColsPerBlock; }

// the sorted-runs block, then part
size_t bwd_ws_layout(int64_t total, int64_t n_src, int c_out, char* base, BwdWs* ws) {
  const size_t sr = spx_sorted_runs_layout(total, n_src, base, ws);
  if (ws) ws->part = (float*)(base + sr);
  return sr + spx_align((size_t)dwx_blocks(total) * c_out * 3 * 4);
}

int check_geom(int32_t c_out, int64_t n_src, int32_t b, int64_t npoint, int32_t nsample, Geom* g) {
  if (c_out <= 0 || n_src < 0 || b < 0 || npoint < 0 || nsample <= 0) return SPX_ERR_INVALID_ARG;
  const int64_t pf = npoint * nsample, total = pf * b;
  if (c_out > 65535 || n_src >= (int64_t)UINT32_MAX || total >= (int64_t)INT32_MAX) return SPX_ERR_TOO_LARGE;
  g->total = total;
  g->per_frame = pf;
  g->nsample = nsample;
  g->c_out = c_out;
  g->n_src = n_src;
  return SPX_OK;
}

template <bool HP, bool HX>
void launch_fwd(const float* p, const float* wx, const float* xyz, const float* ctr, const int32_t* idx,
                const uint8_t* empty, const Geom& g, float* y, hipStream_t s) {
  const dim3 grid((unsigned)((g.total + kThreads - 1) / kThreads));
  const bool v4 = HP && (g.c_out % 4) == 0 && ((uintptr_t)p % 16) == 0;
  if (v4)
    hipLaunchKernelGGL((k_group_project<HP, HX, true>), grid, dim3(kThreads), 0, s, p, wx, xyz, ctr, idx, empty, g, y);
  else
    hipLaunchKernelGGL((k_group_project<HP, HX, false>), grid, dim3(kThreads), 0, s, p, wx, xyz, ctr, idx, empty, g, y);
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int spx_group_project(const float* p, const float* wx, const float* xyz, const float* ctr, const int32_t* idx,
                                 const uint8_t* empty, int32_t c_out, int64_t n_src, int32_t b, int64_t npoint,
                                 int32_t nsample, float* y, spx_stream_t stream) {
  Geom g;
  const int rc = check_geom(c_out, n_src, b, npoint, nsample, &g);
  if (rc != SPX_OK) return rc;
  if (!p && !wx) return SPX_ERR_INVALID_ARG;
  if (g.total == 0) return SPX_OK;
  if (!idx || !y || (wx && (!xyz || !ctr))) return SPX_ERR_INVALID_ARG;
  hipStream_t s = spx_s(stream);
  if (p && wx) launch_fwd<true, true>(p, wx, xyz, ctr, idx, empty, g, y, s);
  else if (p) launch_fwd<true, false>(p, wx, xyz, ctr, idx, empty, g, y, s);
  else launch_fwd<false, true>(p, wx, xyz, ctr, idx, empty, g, y, s);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_group_project_bwd_ws_bytes(int32_t c_out, int64_t n_src, int32_t b, int64_t npoint,
                                                 int32_t nsample) {
  Geom g;
  if (check_geom(c_out, n_src, b, npoint, nsample, &g) != SPX_OK) return 0;
  return bwd_ws_layout(g.total, n_src, c_out, nullptr, nullptr);
}

extern "C" int spx_group_project_bwd(const float* dy, const float* xyz, const float* ctr, const int32_t* idx,
                                     const uint8_t* empty, int32_t c_out, int64_t n_src, int32_t b, int64_t npoint,
                                     int32_t nsample, float* dpt, float* dwx, void* ws, size_t ws_bytes,
                                     spx_stream_t stream) {
  Geom g;
  const int rc = check_geom(c_out, n_src, b, npoint, nsample, &g);
  if (rc != SPX_OK) return rc;
  if (!dpt && !dwx) return SPX_ERR_INVALID_ARG;
  if (g.total > 0 && (!dy || !idx)) return SPX_ERR_INVALID_ARG;
  if (dwx && g.total > 0 && (!xyz || !ctr)) return SPX_ERR_INVALID_ARG;
  if (!ws || ws_bytes < bwd_ws_layout(g.total, n_src, c_out, nullptr, nullptr)) return SPX_ERR_WORKSPACE;
  BwdWs L;
  bwd_ws_layout(g.total, n_src, c_out, (char*)ws, &L);
  hipStream_t s = spx_s(stream);
  if (dpt && n_src > 0) {
    if (g.total > 0)
      hipLaunchKernelGGL(k_gp_keys, dim3((unsigned)((g.total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, idx,
                         empty, g, L.keys_in, L.vals_in);
    if (const int e = spx_sorted_runs(L, g.total, n_src, s); e != SPX_OK) return e;
    hipLaunchKernelGGL(k_gp_dp, dim3((unsigned)((n_src + kThreads - 1) / kThreads), (unsigned)c_out), dim3(kThreads), 0,
                       s, dy, L.vals_out, L.start, L.end, g, dpt);
  }
  if (dwx) {
    const int64_t nblk = dwx_blocks(g.total);
    if (nblk > 0)
      hipLaunchKernelGGL(k_gp_dwx_part, dim3((unsigned)nblk), dim3(kThreads), 0, s, dy, xyz, ctr, idx, empty, g, L.part);
    hipLaunchKernelGGL(spx_k_column_sum<float>, dim3((unsigned)(c_out * 3)), dim3(256), 0, s, L.part, nblk, c_out * 3, dwx);
  }
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
