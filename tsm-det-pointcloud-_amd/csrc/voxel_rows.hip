// voxel_rows.hip — the two index steps that keep the voxel-point SA modules on static row capacities (include/spx.h §19).
//
//  * spx_voxel_table_build: the dense cell -> row table of a sparse tensor whose live row count is on the device
//    (generate_voxel2pinds, reference pcdet/utils/common_utils.py:257-265, which scatters every row it is given).
//  * spx_voxel_rows_mean: per-cell mean of a layer's new point features written to the rows of an existing sparse tensor
//    (the chain get_voxel_indices -> get_centroid_per_voxel -> get_nonempty_voxel_feature_indices -> masked assignment
//    of _VoxelPointnetSAModuleFSDistillationBase._unet_update, reference pointnet2_modules.py; about ten launches and
//    two host reads there).
//
// Both are integer work on a few thousand rows: what matters is the launch count and that no dead row is ever read, not
// bandwidth.  Nothing here uses atomics on data (the status word aside), so the results are bitwise reproducible.
#include "spx_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxPoints = 4096;   // points per frame: their cell keys sit in LDS (16 KiB)

__global__ void k_table_scatter(const int32_t* __restrict__ idx, int64_t cap, const int64_t* d_n, int batch, Int3 shape,
                                int32_t* __restrict__ table, int32_t* status) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= spx_live_n(d_n, cap)) return;          // dead rows are never read
  const int4 c = reinterpret_cast<const int4*>(idx)[r];
  if ((unsigned)c.x >= (unsigned)batch || (unsigned)c.y >= (unsigned)shape.v[0] ||
      (unsigned)c.z >= (unsigned)shape.v[1] || (unsigned)c.w >= (unsigned)shape.v[2]) {
    if (status) atomicMin(status, (int32_t)SPX_ERR_OUT_OF_GRID);
    return;
  }
  table[spx_lin_key(c.x, c.y, c.z, c.w, shape)] = (int32_t)r;
}

struct RowsGeom {
  float lo[3], vs[3];   // x, y, z
  Int3 shape;           // Z, Y, X
};

struct RowsWs {
  int32_t *row, *next, *count;   // [batch * m] each
  size_t total;
};

static inline RowsWs rows_layout(void* ws, int64_t batch, int64_t m) {
  RowsWs w;
  char* p = reinterpret_cast<char*>(ws);
  const size_t one = spx_align((size_t)(batch * m) * 4);
  w.row = reinterpret_cast<int32_t*>(p);
  w.next = reinterpret_cast<int32_t*>(p + one);
  w.count = reinterpret_cast<int32_t*>(p + 2 * one);
  w.total = 3 * one;
  return w;
}

// trunc((p - lo) / vs) per axis in fp32 with a correctly rounded division (what get_voxel_indices computes with
// torch's sub, div and .long()); -1 for a point outside the grid
__device__ __forceinline__ int32_t point_key(const float* __restrict__ p, const RowsGeom& g) {
  int c[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float f = __fdiv_rn(__fsub_rn(p[j], g.lo[j]), g.vs[j]);
    const int dim = g.shape.v[2 - j];
    if (!(f > -1.0f) || !(f < (float)dim)) return -1;   // NaN too; (-1, 0) truncates to cell 0 like .long()
    c[j] = (int)f;
  }
  return (c[2] * g.shape.v[1] + c[1]) * g.shape.v[2] + c[0];
}

// grid (ceil(m / 256), batch).  Every workgroup recomputes the m cell keys of its frame into LDS, then each thread links
// its own point: the FIRST point of a cell owns the cell; `next` chains a cell's points in ascending point order.  The
// owner's table row (or -1: cell not active, point outside, or not the owner) goes to ws.row.  The workgroups together
// also zero the live rows of `out`, so that the mean kernel only has to write the rows that are hit.
__global__ __launch_bounds__(kBlock) void k_rows_link(const float* __restrict__ new_xyz, int m, RowsGeom g,
                                                      const int32_t* __restrict__ table, RowsWs w,
                                                      float* __restrict__ out, int64_t cap, const int64_t* d_n, int C) {
  __shared__ int32_t key_s[kMaxPoints];
  const int b = blockIdx.y;
  const float* xyz = new_xyz + (int64_t)b * m * 3;
  for (int j = threadIdx.x; j < m; j += kBlock) key_s[j] = point_key(xyz + (int64_t)j * 3, g);
  __syncthreads();

  const int64_t nblk = (int64_t)gridDim.x * gridDim.y;
  const int64_t live = spx_live_n(d_n, cap) * C;
  for (int64_t t = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x; t < live; t += nblk * kBlock)
    out[t] = 0.f;

  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const int32_t key = key_s[i];
  int first = i, nxt = -1, cnt = 0;
  if (key >= 0) {
    for (int j = 0; j < m; ++j) {                    // uniform loop, broadcast LDS reads
      const bool same = key_s[j] == key;
      cnt += same ? 1 : 0;
      if (same && j < first) first = j;
      if (same && j > i && nxt < 0) nxt = j;
    }
  }
  const int64_t o = (int64_t)b * m + i;
  int32_t row = -1;
  if (key >= 0 && first == i) row = table[(int64_t)b * g.shape.v[0] * g.shape.v[1] * g.shape.v[2] + key];
  if (row >= spx_live_n(d_n, cap)) row = -1;         // a table that was not built from these rows: never write a dead row
  w.row[o] = row;
  w.next[o] = nxt;
  w.count[o] = cnt;
}

// grid (ceil(m / 256), C, batch): thread (point i, column c).  Owners walk their cell's chain: the sum starts at 0 and
// adds the points in ascending order, then multiplies by 1 / count — the sequence of rounded operations of k_dyn_mean
// (csrc/rulebook.hip), so the rows equal spx_dynamic_voxelize's bit for bit.
__global__ __launch_bounds__(kBlock) void k_rows_mean(const float* __restrict__ feats, int m, int C, RowsWs w,
                                                      float* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= m) return;
  const int c = blockIdx.y, b = blockIdx.z;
  const int64_t base = (int64_t)b * m;
  const int32_t row = w.row[base + i];
  if (row < 0) return;
  const float* f = feats + ((int64_t)b * C + c) * m;
  const float inv_m = 1.0f / (float)w.count[base + i];
  float s = 0.f;
  for (int j = i; j >= 0; j = w.next[base + j]) s += f[j];
  out[(int64_t)row * C + c] = s * inv_m;
}

static inline bool bad_shape(const int32_t* shape3) { return shape3[0] <= 0 || shape3[1] <= 0 || shape3[2] <= 0; }

}  // namespace

extern "C" int spx_voxel_table_build(const int32_t* indices, int64_t cap, const int64_t* d_n, int32_t batch,
                                     const int32_t* shape3, int32_t* table, int32_t* d_status, spx_stream_t stream) {
  if (!indices || !shape3 || !table || cap <= 0 || batch <= 0 || bad_shape(shape3)) return SPX_ERR_INVALID_ARG;
  const int64_t cells = (int64_t)batch * shape3[0] * shape3[1] * shape3[2];
  if (cap >= (int64_t(1) << 31) || cells >= (int64_t(1) << 40)) return SPX_ERR_TOO_LARGE;
  hipStream_t s = spx_s(stream);
  spx_fill_async(table, 0xFF, (size_t)cells * 4, s);   // -1 everywhere
  hipLaunchKernelGGL(k_table_scatter, dim3((unsigned)((cap + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, indices, cap, d_n,
                     batch, spx_i3(shape3), table, d_status);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_voxel_rows_mean_ws_bytes(int32_t batch, int64_t m) {
  if (batch <= 0 || m <= 0) return 0;
  return rows_layout(nullptr, batch, m).total;
}

extern "C" int spx_voxel_rows_mean(const float* new_xyz, const float* feats, int32_t batch, int32_t c, int64_t m,
                                   const int32_t* table, const int32_t* shape3, const float* range_lo3,
                                   const float* voxel_size3, const int64_t* d_n_rows, int64_t cap, float* out, void* ws,
                                   size_t ws_bytes, spx_stream_t stream) {
  if (!new_xyz || !feats || !table || !shape3 || !range_lo3 || !voxel_size3 || !out || batch <= 0 || c <= 0 || m <= 0 ||
      cap <= 0 || bad_shape(shape3))
    return SPX_ERR_INVALID_ARG;
  for (int j = 0; j < 3; ++j)
    if (!(voxel_size3[j] > 0.f)) return SPX_ERR_INVALID_ARG;
  if (m > kMaxPoints || batch > 65535 || c > 65535 || cap >= (int64_t(1) << 31) ||
      (int64_t)shape3[0] * shape3[1] * shape3[2] >= (int64_t(1) << 31))
    return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < spx_voxel_rows_mean_ws_bytes(batch, m)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  RowsWs w = rows_layout(ws, batch, m);
  RowsGeom g;
  for (int j = 0; j < 3; ++j) {
    g.lo[j] = range_lo3[j];
    g.vs[j] = voxel_size3[j];
  }
  g.shape = spx_i3(shape3);
  const unsigned nb = (unsigned)((m + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_rows_link, dim3(nb, (unsigned)batch), dim3(kBlock), 0, s, new_xyz, (int)m, g, table, w, out, cap,
                     d_n_rows, (int)c);
  hipLaunchKernelGGL(k_rows_mean, dim3(nb, (unsigned)c, (unsigned)batch), dim3(kBlock), 0, s, feats, (int)m, (int)c, w, out);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
