// voxel_pool.hip — the pooling tail of NeighborVoxelSAModuleMSG at RoI-grid size, fused (include/spx.h §27).  The torch
// composition gathers (M, C, nsample) features, masks empty balls, runs the position Conv2d + BatchNorm2d on the
// (M, 3, nsample) offsets, adds, applies ReLU and takes the max over the slots: half a dozen (M, C, nsample) tensors
// forward and again backward.  With BatchNorm folded by the caller into an affine map (A, b) of the offset, the whole
// tail is
//
//   out[m, c] = max(0, max_s f[r, c] + A[c] . (xyz[r] - new_xyz[m]) + b[c]),   r = idx[m, s]
//
// one gather of C-float rows and three multiply-adds per slot; only (M, C) outputs reach memory.  The statistics that
// BatchNorm2d needs in training are the first and second moments of the offsets (nine numbers), summed here in double.
// Backward, deterministic (no float atomics):
//   df[r, c]  = sum of dout[m, c] over the (m, c) whose winning slot points at r: sorted runs of the (m, s) entries by
//               r (sorted_runs.h), then every (r, c) walks its run in ascending m;
//   dA, db    = each block sums a fixed chunk of queries (one wave per query, strided, then the four waves in order),
//               one block per output then adds the per-block partials in a fixed order.
#include "block_ops.h"
#include "sorted_runs.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SPX_WAVE;
constexpr int kMomColsPerThread = 8;                       // moments: columns per thread per block
constexpr int kMomCols = kThreads * kMomColsPerThread;
constexpr int kQChunk = 128;                               // dA / db: queries per block

struct Geom {
  int64_t m;       // queries
  int64_t total;   // m * nsample columns
  int64_t n_src;
  int nsample;
  int c;
};

// source row of slot (m, s), or -1 when it is outside [0, n_src); the caller has checked empty[m]
__device__ __forceinline__ int64_t slot_row(const Geom& g, const int32_t* __restrict__ idx, int64_t m, int s) {
  const int32_t r = idx[m * g.nsample + s];
  return (r < 0 || (int64_t)r >= g.n_src) ? -1 : (int64_t)r;
}

// ---------------------------------------------------------------------------------------------- forward
// One thread owns V consecutive channels of one query and walks the slots in ascending order.
template <int V>
__global__ __launch_bounds__(kThreads) void k_vp_fwd(const float* __restrict__ f, const float* __restrict__ xyz,
                                                     const float* __restrict__ new_xyz,
                                                     const int32_t* __restrict__ idx,
                                                     const uint8_t* __restrict__ empty, const float* __restrict__ a,
                                                     const float* __restrict__ b, Geom g, float* __restrict__ out,
                                                     int32_t* __restrict__ arg) {
  const int cg = g.c / V;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= g.m * cg) return;
  const int64_t m = t / cg;
  const int c0 = (int)(t - m * cg) * V;
  float a0[V], a1[V], a2[V], bb[V], best[V];
  int32_t win[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    a0[j] = a[(c0 + j) * 3 + 0];
    a1[j] = a[(c0 + j) * 3 + 1];
    a2[j] = a[(c0 + j) * 3 + 2];
    bb[j] = b[c0 + j];
    best[j] = -INFINITY;
    win[j] = -1;
  }
  bool any = false;
  if (!(empty && empty[m])) {
    const float cx = new_xyz[m * 3 + 0], cy = new_xyz[m * 3 + 1], cz = new_xyz[m * 3 + 2];
    for (int s = 0; s < g.nsample; ++s) {
      const int64_t r = slot_row(g, idx, m, s);
      if (r < 0) continue;
      any = true;
      const float dx = xyz[r * 3 + 0] - cx, dy = xyz[r * 3 + 1] - cy, dz = xyz[r * 3 + 2] - cz;
      float fv[V];
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(f + (size_t)r * g.c + c0);
        fv[0] = q.x;
        fv[1] = q.y;
        fv[2] = q.z;
        fv[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) fv[j] = f[(size_t)r * g.c + c0 + j];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float v = fv[j] + (((a0[j] * dx + a1[j] * dy) + a2[j] * dz) + bb[j]);
        if (v > best[j]) {
          best[j] = v;
          win[j] = s;
        }
      }
    }
  }
  if (!any) {  // empty: every slot holds 0 + (A . 0 + b), the lowest slot attains it
#pragma unroll
    for (int j = 0; j < V; ++j) {
      best[j] = bb[j];
      win[j] = 0;
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const bool pos = best[j] > 0.f;
    best[j] = pos ? best[j] : 0.f;
    win[j] = pos ? win[j] : -1;
  }
  const size_t o = (size_t)m * g.c + c0;
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(out + o) = make_float4(best[0], best[1], best[2], best[3]);
    *reinterpret_cast<int4*>(arg + o) = make_int4(win[0], win[1], win[2], win[3]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      out[o + j] = best[j];
      arg[o + j] = win[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------- moments
// part[blk][9] = (sum d, upper triangle of sum d d^T) over the block's kMomCols columns
__global__ __launch_bounds__(kThreads) void k_vp_mom_part(const float* __restrict__ xyz,
                                                          const float* __restrict__ new_xyz,
                                                          const int32_t* __restrict__ idx,
                                                          const uint8_t* __restrict__ empty, Geom g,
                                                          double* __restrict__ part) {
  __shared__ double s_w[kWaves][9];
  const int tid = threadIdx.x, wave = tid / SPX_WAVE, lane = tid % SPX_WAVE;
  const int64_t base = (int64_t)blockIdx.x * kMomCols;
  double acc[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) acc[q] = 0.0;
#pragma unroll
  for (int i = 0; i < kMomColsPerThread; ++i) {
    const int64_t col = base + (int64_t)i * kThreads + tid;
    if (col >= g.total) continue;
    const int64_t m = col / g.nsample;
    if (empty && empty[m]) continue;
    const int64_t r = slot_row(g, idx, m, (int)(col - m * g.nsample));
    if (r < 0) continue;
    const double x = (double)(xyz[r * 3 + 0] - new_xyz[m * 3 + 0]);
    const double y = (double)(xyz[r * 3 + 1] - new_xyz[m * 3 + 1]);
    const double z = (double)(xyz[r * 3 + 2] - new_xyz[m * 3 + 2]);
    acc[0] += x;
    acc[1] += y;
    acc[2] += z;
    acc[3] += x * x;
    acc[4] += x * y;
    acc[5] += x * z;
    acc[6] += y * y;
    acc[7] += y * z;
    acc[8] += z * z;
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const double v = spx_wave_sum(acc[q]);
    if (lane == 0) s_w[wave][q] = v;
  }
  __syncthreads();
  if (tid < 9) {
    double v = s_w[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += s_w[w][tid];
    part[(size_t)blockIdx.x * 9 + tid] = v;
  }
}

// ---------------------------------------------------------------------------------------------- df
__global__ __launch_bounds__(kThreads) void k_vp_keys(const int32_t* __restrict__ idx, const uint8_t* __restrict__ empty,
                                                      Geom g, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t col = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (col >= g.total) return;
  const int64_t m = col / g.nsample;
  int64_t r = -1;
  if (!(empty && empty[m])) r = slot_row(g, idx, m, (int)(col - m * g.nsample));
  keys[col] = r < 0 ? (uint32_t)g.n_src : (uint32_t)r;
  vals[col] = (uint32_t)col;
}

// df[r, c] = sum over r's sorted run of dout[m, c] where the winning slot of (m, c) is the entry's, in ascending m
__global__ __launch_bounds__(kThreads) void k_vp_df(const float* __restrict__ dout, const int32_t* __restrict__ arg,
                                                    const uint32_t* __restrict__ vals,
                                                    const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                                                    Geom g, float* __restrict__ df) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= g.n_src * g.c) return;
  const int64_t r = t / g.c;
  const int c = (int)(t - r * g.c);
  const int32_t lo = start[r], hi = end[r];
  float acc = 0.f;
  for (int32_t q = lo; q < hi; ++q) {
    const uint32_t col = vals[q];
    const uint32_t m = col / (uint32_t)g.nsample;
    const int32_t s = (int32_t)(col - m * (uint32_t)g.nsample);
    const size_t o = (size_t)m * g.c + c;
    if (arg[o] == s) acc += dout[o];
  }
  df[t] = acc;
}

// ---------------------------------------------------------------------------------------------- dA, db
// part[chunk][c][4] = sum over the chunk's queries of g * (dx, dy, dz, 1); lane = channel, one wave per query
__global__ __launch_bounds__(kThreads) void k_vp_dab_part(const float* __restrict__ dout,
                                                          const int32_t* __restrict__ arg,
                                                          const int32_t* __restrict__ idx,
                                                          const uint8_t* __restrict__ empty,
                                                          const float* __restrict__ xyz,
                                                          const float* __restrict__ new_xyz, Geom g,
                                                          float* __restrict__ part) {
  __shared__ float s_w[kWaves][SPX_WAVE][4];
  const int tid = threadIdx.x, wave = tid / SPX_WAVE, lane = tid % SPX_WAVE;
  const int c = blockIdx.y * SPX_WAVE + lane;
  const int64_t m0 = (int64_t)blockIdx.x * kQChunk;
  float ax = 0.f, ay = 0.f, az = 0.f, ab = 0.f;
  if (c < g.c) {
    for (int i = wave; i < kQChunk; i += kWaves) {
      const int64_t m = m0 + i;
      if (m >= g.m) break;
      const size_t o = (size_t)m * g.c + c;
      const int32_t s = arg[o];
      if (s < 0 || s >= g.nsample) continue;
      const float gv = dout[o];
      ab += gv;
      if (empty && empty[m]) continue;
      const int64_t r = slot_row(g, idx, m, s);
      if (r < 0) continue;
      ax += gv * (xyz[r * 3 + 0] - new_xyz[m * 3 + 0]);
      ay += gv * (xyz[r * 3 + 1] - new_xyz[m * 3 + 1]);
      az += gv * (xyz[r * 3 + 2] - new_xyz[m * 3 + 2]);
    }
  }
  s_w[wave][lane][0] = ax;
  s_w[wave][lane][1] = ay;
  s_w[wave][lane][2] = az;
  s_w[wave][lane][3] = ab;
  __syncthreads();
  const int l = tid / 4, j = tid % 4, cc = blockIdx.y * SPX_WAVE + l;   // kThreads == SPX_WAVE * 4
  if (cc < g.c) {
    float v = s_w[0][l][j];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += s_w[w][l][j];
    part[((size_t)blockIdx.x * g.c + cc) * 4 + j] = v;
  }
}

// dab4 [c][4] -> da [c][3], db [c]
__global__ __launch_bounds__(kThreads) void k_vp_dab_split(const float* __restrict__ dab4, int c, float* __restrict__ da,
                                                           float* __restrict__ db) {
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= c * 4) return;
  const int cc = q / 4, j = q % 4;
  if (j < 3) {
    if (da) da[cc * 3 + j] = dab4[q];
  } else if (db) {
    db[cc] = dab4[q];
  }
}

int check_geom(int32_t c, int64_t n_src, int64_t m, int32_t nsample, Geom* g) {
  if (c <= 0 || n_src < 0 || m < 0 || nsample <= 0) return SPX_ERR_INVALID_ARG;
  if (c > 65535 || n_src >= (int64_t)UINT32_MAX || m >= (int64_t)INT32_MAX) return SPX_ERR_TOO_LARGE;
  if (m * nsample >= (int64_t)INT32_MAX || m * c >= (int64_t)INT32_MAX) return SPX_ERR_TOO_LARGE;
  if (n_src * c / kThreads >= (int64_t)INT32_MAX) return SPX_ERR_TOO_LARGE;
  g->m = m;
  g->total = m * nsample;
  g->n_src = n_src;
  g->nsample = nsample;
  g->c = c;
  return SPX_OK;
}

int64_t mom_blocks(int64_t total) { return (total + kMomCols - 1) / kMomCols; }
int64_t dab_chunks(int64_t m) { return (m + kQChunk - 1) / kQChunk; }

struct BwdWs : SortedRunsWs {
  float *part, *dab4;   // dA / db: [dab_chunks][c][4] partials, [c][4] sums
};

// the sorted-runs block, then part | dab4
size_t bwd_ws_layout(const Geom& g, char* base, BwdWs* ws) {
  const size_t sr = spx_sorted_runs_layout(g.total, g.n_src, base, ws);
  const size_t pb = spx_align((size_t)dab_chunks(g.m) * g.c * 4 * 4), fb = spx_align((size_t)g.c * 4 * 4);
  if (ws) {
    ws->part = (float*)(base + sr);
    ws->dab4 = (float*)(base + sr + pb);
  }
  return sr + pb + fb;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" size_t spx_voxel_pool_moments_ws_bytes(int64_t m, int32_t nsample) {
  Geom g;
  if (check_geom(1, 0, m, nsample, &g) != SPX_OK) return 0;
  return spx_align((size_t)mom_blocks(g.total) * 9 * sizeof(double));
}

extern "C" int spx_voxel_pool_moments(const float* xyz, const float* new_xyz, const int32_t* idx, const uint8_t* empty,
                                      int64_t n_src, int64_t m, int32_t nsample, double* moments, void* ws,
                                      size_t ws_bytes, spx_stream_t stream) {
  Geom g;
  const int rc = check_geom(1, n_src, m, nsample, &g);
  if (rc != SPX_OK) return rc;
  if (!moments) return SPX_ERR_INVALID_ARG;
  if (g.total > 0 && (!new_xyz || !idx || (n_src > 0 && !xyz))) return SPX_ERR_INVALID_ARG;
  const int64_t nblk = mom_blocks(g.total);
  if (nblk > 0 && (!ws || ws_bytes < spx_align((size_t)nblk * 9 * sizeof(double)))) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  double* part = (double*)ws;
  if (nblk > 0)
    hipLaunchKernelGGL(k_vp_mom_part, dim3((unsigned)nblk), dim3(kThreads), 0, s, xyz, new_xyz, idx, empty, g, part);
  hipLaunchKernelGGL(spx_k_column_sum<double>, dim3(9), dim3(256), 0, s, part, nblk, 9, moments);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_voxel_pool_max_fwd(const float* f, const float* xyz, const float* new_xyz, const int32_t* idx,
                                      const uint8_t* empty, const float* a, const float* b, int32_t c, int64_t n_src,
                                      int64_t m, int32_t nsample, float* out, int32_t* arg, spx_stream_t stream) {
  Geom g;
  const int rc = check_geom(c, n_src, m, nsample, &g);
  if (rc != SPX_OK) return rc;
  if (g.m == 0) return SPX_OK;
  if (!new_xyz || !idx || !a || !b || !out || !arg || (n_src > 0 && (!f || !xyz))) return SPX_ERR_INVALID_ARG;
  hipStream_t s = spx_s(stream);
  const bool v4 = (c % 4) == 0 && (((uintptr_t)f | (uintptr_t)out | (uintptr_t)arg) % 16) == 0;
  if (v4) {
    const int64_t nt = g.m * (c / 4);
    hipLaunchKernelGGL((k_vp_fwd<4>), dim3((unsigned)((nt + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, f, xyz,
                       new_xyz, idx, empty, a, b, g, out, arg);
  } else {
    const int64_t nt = g.m * c;
    hipLaunchKernelGGL((k_vp_fwd<1>), dim3((unsigned)((nt + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, f, xyz,
                       new_xyz, idx, empty, a, b, g, out, arg);
  }
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_voxel_pool_max_bwd_ws_bytes(int32_t c, int64_t n_src, int64_t m, int32_t nsample) {
  Geom g;
  if (check_geom(c, n_src, m, nsample, &g) != SPX_OK) return 0;
  return bwd_ws_layout(g, nullptr, nullptr);
}

extern "C" int spx_voxel_pool_max_bwd(const float* dout, const int32_t* arg, const int32_t* idx, const uint8_t* empty,
                                      const float* xyz, const float* new_xyz, int32_t c, int64_t n_src, int64_t m,
                                      int32_t nsample, float* df, float* da, float* db, void* ws, size_t ws_bytes,
                                      spx_stream_t stream) {
  Geom g;
  const int rc = check_geom(c, n_src, m, nsample, &g);
  if (rc != SPX_OK) return rc;
  if (!df && !da && !db) return SPX_ERR_INVALID_ARG;
  if (g.m > 0 && (!dout || !arg || !idx)) return SPX_ERR_INVALID_ARG;
  if ((da || db) && g.m > 0 && (!new_xyz || (n_src > 0 && !xyz))) return SPX_ERR_INVALID_ARG;
  if (!ws || ws_bytes < bwd_ws_layout(g, nullptr, nullptr)) return SPX_ERR_WORKSPACE;
  BwdWs L;
  bwd_ws_layout(g, (char*)ws, &L);
  hipStream_t s = spx_s(stream);
  if (df && n_src > 0) {
    if (g.total > 0)
      hipLaunchKernelGGL(k_vp_keys, dim3((unsigned)((g.total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, idx,
                         empty, g, L.keys_in, L.vals_in);
    if (const int e = spx_sorted_runs(L, g.total, n_src, s); e != SPX_OK) return e;
    const int64_t nt = n_src * c;
    hipLaunchKernelGGL(k_vp_df, dim3((unsigned)((nt + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, dout, arg,
                       L.vals_out, L.start, L.end, g, df);
  }
  if (da || db) {
    const int64_t nchunk = dab_chunks(g.m);
    if (nchunk > 0)
      hipLaunchKernelGGL(k_vp_dab_part, dim3((unsigned)nchunk, (unsigned)((c + SPX_WAVE - 1) / SPX_WAVE)), dim3(kThreads),
                         0, s, dout, arg, idx, empty, xyz, new_xyz, g, L.part);
    hipLaunchKernelGGL(spx_k_column_sum<float>, dim3((unsigned)(c * 4)), dim3(256), 0, s, L.part, nchunk, c * 4, L.dab4);
    hipLaunchKernelGGL(k_vp_dab_split, dim3((unsigned)((c * 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, L.dab4,
                       c, da, db);
  }
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
