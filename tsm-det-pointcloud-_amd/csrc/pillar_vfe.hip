// pillar_vfe.hip — PointPillars' PillarVFE with one last-layer PFNLayer, forward and parameter gradients (include/spx.h §23).
//
// Restates PillarVFE.forward + PFNLayer.forward (reference pcdet/models/backbones_3d/vfe/pillar_vfe.py:29-123) for
// NUM_FILTERS of length 1 with USE_NORM: the per-point features [raw | xyz - pillar mean | xyz - pillar centre | norm],
// Linear(C_in, 64, bias=False), BatchNorm1d over all M * T rows (padding rows are all-zero feature rows and COUNT), ReLU
// and the max over the T rows of a pillar.  The composition writes an [M, T, 64] tensor five times; here it never exists.
//
// The PFN core — the 13 fixed feature slots and their slot -> weight-column table, the S1 / G statistics, the BatchNorm
// fold and the closed-form weight gradient — is pfn_layer.h, shared with dyn_pillar_vfe.hip; the derivations are there.
// One builder (build_tile) puts the features of 8 pillars x 32 point slots into LDS as doubles; every kernel goes through
// it, so the statistics, the forward and the backward see identical features.
//
// Training forward, three launches:
//   1. k_stats: S1 = sum f and G = sum f f^T over the real points (13 + 169 doubles), one partial per block;
//   2. k_stats_final: fixed-order sum of the partials, N = live rows * T (padding rows are all-zero feature rows and
//      count), then pfn_layer.h's per-channel statistics, running update (whenever N > 0) and counter;
//   3. k_fwd: one thread per (pillar, channel): x = w.f in double over the real points, z = x * scale + shift, the ReLU,
//      the max and its index; a pillar with fewer than T points also offers relu(shift), the value of its padding rows.
// Eval forward: launch 3 alone, scale / shift folded from the running statistics.
//
// Backward, two launches: k_bwd_gather takes A, d_beta, d_gamma of pfn_layer.h's dW formula (one partial per block; a
// selected padding row has f = 0 and xhat = -mean invstd), pfn_k_bwd_final adds them in a fixed order and applies it.
//
// No float atomics, no host read, every sum in double in a fixed order: outputs and gradients are bitwise reproducible,
// and every launch shape depends on host values only (the live row count d_n is read on the device).
#include "pfn_layer.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileP = 8;         // pillars per tile
constexpr int kMaxT = 32;         // point slots per pillar
constexpr int kMaxPart = 256;     // partial-writing blocks of k_stats and k_bwd_gather

struct Geo {
  float vx, vy, vz, ox, oy, oz;
  int c, t;
  int col[kSlots];                // slot -> weight column, -1 absent
  int c_in;
};

struct In {
  const float* voxels;            // [m, t, c]
  const int32_t* num;             // [m]
  const int32_t* coords;          // [m, 4] (b, z, y, x)
  const int64_t* d_n;
  int64_t m;
};

// Features of pillars [p0, p0 + 8) into fs[(p * 32 + t) * 13 + slot] for t < s_num[p]; s_num[p] = the row's point
// count clamped to [0, T], 0 for a row at or beyond n_live (never dereferenced).  Thread = (p = tid >> 5, t = tid & 31).
__device__ __forceinline__ void build_tile(const In& in, const Geo& g, int64_t p0, int64_t n_live, double* fs, int* s_num) {
  const int p = threadIdx.x >> 5, t = threadIdx.x & 31;
  const int64_t row = p0 + p;
  int num = 0;
  if (row < n_live) {
    num = in.num[row];
    num = num < 0 ? 0 : (num > g.t ? g.t : num);
  }
  const bool real = t < num;
  float x = 0.f, y = 0.f, z = 0.f, e[3] = {0.f, 0.f, 0.f};
  if (real) {
    const float* __restrict__ pt = in.voxels + (row * g.t + t) * g.c;
    x = pt[0];
    y = pt[1];
    z = pt[2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (3 + j < g.c) e[j] = pt[3 + j];
  }
  // the pillar's sum over its real points: an xor butterfly inside the 32-lane group, the same bits in every lane
  double sx = x, sy = y, sz = z;
#pragma unroll
  for (int d = 16; d > 0; d >>= 1) {
    sx += __shfl_xor(sx, d, 32);
    sy += __shfl_xor(sy, d, 32);
    sz += __shfl_xor(sz, d, 32);
  }
  if (t == 0) s_num[p] = num;
  if (!real) return;
  const double inv = 1.0 / (double)num;
  const int32_t* __restrict__ cd = in.coords + row * 4;
  const float cx = centre32(cd[3], g.vx, g.ox);
  const float cy = centre32(cd[2], g.vy, g.oy);
  const float cz = centre32(cd[1], g.vz, g.oz);
  double* __restrict__ f = fs + (p * kMaxT + t) * kSlots;
  const double dx = x, dy = y, dz = z;
  f[0] = dx;
  f[1] = dy;
  f[2] = dz;
  f[3] = dx - sx * inv;
  f[4] = dy - sy * inv;
  f[5] = dz - sz * inv;
  f[6] = dx - (double)cx;
  f[7] = dy - (double)cy;
  f[8] = dz - (double)cz;
  f[9] = sqrt(dx * dx + dy * dy + dz * dz);
  f[10] = e[0];
  f[11] = e[1];
  f[12] = e[2];
}

// ---------------------------------------------------------------------------------------------------- statistics
__global__ __launch_bounds__(kBlock) void k_stats(In in, Geo g, double* __restrict__ part) {
  __shared__ double fs[kTileP * kMaxT * kSlots];
  __shared__ int s_num[kTileP];
  const int64_t n_live = spx_live_n(in.d_n, in.m);
  const int e = threadIdx.x;
  const bool gram = e < kG;
  const int i = gram ? e / kSlots : 0, j = gram ? e % kSlots : (e < kStat ? e - kG : 0);
  double acc = 0.0;
  for (int64_t tile = blockIdx.x; tile * kTileP < n_live; tile += gridDim.x) {
    build_tile(in, g, tile * kTileP, n_live, fs, s_num);
    __syncthreads();
    if (e < kStat) {
      for (int p = 0; p < kTileP; ++p) {
        const int num = s_num[p];
        const double* __restrict__ f = fs + p * kMaxT * kSlots;
        for (int t = 0; t < num; ++t, f += kSlots) acc = gram ? fma(f[i], f[j], acc) : acc + f[j];
      }
    }
    __syncthreads();
  }
  if (e < kStat) part[(int64_t)blockIdx.x * kStat + e] = acc;
}

__global__ __launch_bounds__(kBlock) void k_stats_final(In in, Geo g, BN bn, const double* __restrict__ part, int n_part,
                                                        double* __restrict__ stats, double* __restrict__ ss,
                                                        float* __restrict__ save_mean, float* __restrict__ save_invstd) {
  __shared__ double s[kStat];
  const int e = threadIdx.x;
  const int64_t n_live = spx_live_n(in.d_n, in.m);
  if (e < kStat) {
    double a = 0.0;
    for (int b = 0; b < n_part; ++b) a += part[(int64_t)b * kStat + e];
    s[e] = a;
    stats[e] = a;
  }
  __syncthreads();
  const double n = (double)n_live * (double)g.t;
  if (e == 0) {
    stats[kOffN] = n;
    stats[kOffN + 1] = 0.0;
    if (n > 0.0 && bn.nbt) bn.nbt[0] += 1;
  }
  if (e >= kCout) return;
  stats_channel(bn, g, s, n, n > 0.0, e, stats, ss, save_mean, save_invstd);
}

// ------------------------------------------------------------------------------------------------------- forward
// ss: the folded scale / shift of k_stats_final, or nullptr: fold the running statistics here (eval, one pass)
__global__ __launch_bounds__(kBlock) void k_fwd(In in, Geo g, BN bn, const double* __restrict__ ss, float* __restrict__ out,
                                                uint8_t* __restrict__ arg) {
  __shared__ double fs[kTileP * kMaxT * kSlots];
  __shared__ int s_num[kTileP];
  const int64_t n_live = spx_live_n(in.d_n, in.m);
  const int64_t p0 = (int64_t)blockIdx.x * kTileP;
  const int q = threadIdx.x >> 6, ch = threadIdx.x & 63;
  if (p0 >= n_live) {             // a tile of dead rows: exact zeros, nothing read
    for (int h = 0; h < 2; ++h) {
      const int64_t row = p0 + q + 4 * h;
      if (row < in.m) {
        out[row * kCout + ch] = 0.f;
        arg[row * kCout + ch] = 0;
      }
    }
    return;
  }
  build_tile(in, g, p0, n_live, fs, s_num);
  double w[kSlots];
  load_w(bn.weight, g, ch, w);
  double scale, shift;
  fold_scale_shift(bn, ss, ch, scale, shift);
  const double pad = shift > 0.0 ? shift : 0.0;
  __syncthreads();
  for (int h = 0; h < 2; ++h) {
    const int p = q + 4 * h;
    const int64_t row = p0 + p;
    if (row >= in.m) continue;
    float o = 0.f;
    int a = 0;
    if (row < n_live) {
      const int num = s_num[p];
      const double* __restrict__ f = fs + p * kMaxT * kSlots;
      double best = -1.0;
      for (int t = 0; t < num; ++t, f += kSlots) {
        const double z = fma(dot13(w, f), scale, shift);
        const double r = z > 0.0 ? z : 0.0;
        if (r > best) {           // strict: ties keep the lowest index
          best = r;
          a = t;
        }
      }
      if (num < g.t && pad > best) {
        best = pad;
        a = g.t;
      }
      o = (float)best;
    }
    out[row * kCout + ch] = o;
    arg[row * kCout + ch] = (uint8_t)a;
  }
}

// ------------------------------------------------------------------------------------------------------ backward
__global__ __launch_bounds__(kBlock) void k_bwd_gather(In in, Geo g, BN bn, Bwd<uint8_t> b, double* __restrict__ part) {
  __shared__ double fs[kTileP * kMaxT * kSlots];
  __shared__ int s_num[kTileP];
  const int64_t n_live = spx_live_n(in.d_n, in.m);
  const int q = threadIdx.x >> 6, ch = threadIdx.x & 63;
  double w[kSlots];
  load_w(bn.weight, g, ch, w);
  double mean, invstd;
  mean_invstd(bn, b, ch, mean, invstd);
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  for (int64_t tile = blockIdx.x; tile * kTileP < n_live; tile += gridDim.x) {
    build_tile(in, g, tile * kTileP, n_live, fs, s_num);
    __syncthreads();
    for (int h = 0; h < 2; ++h) {
      const int p = q + 4 * h;
      const int64_t row = tile * kTileP + p;
      if (row >= n_live) continue;
      if (!(b.out[row * kCout + ch] > 0.f)) continue;
      const double gr = (double)b.d_out[row * kCout + ch];
      const int a = b.arg[row * kCout + ch];
      double xhat = -mean * invstd;           // a padding row: x = 0, f = 0
      if (a < s_num[p]) {
        const double* __restrict__ f = fs + (p * kMaxT + a) * kSlots;
        xhat = (dot13(w, f) - mean) * invstd;
#pragma unroll
        for (int k = 0; k < kSlots; ++k) acc[2 + k] = fma(gr, f[k], acc[2 + k]);
      }
      acc[0] += gr;
      acc[1] = fma(gr, xhat, acc[1]);
    }
    __syncthreads();
  }
  // the four pillar lanes of a channel, added in the order q = 0, 1, 2, 3 (fs is free after the loop's last barrier)
  double* red = fs;
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

// The partial-writing grids do not depend on m: tile i always goes to block i % kMaxPart, so a call at static capacity
// with d_n live rows adds the same numbers in the same order as the exact-size call on those rows.
inline int n_part_of(int64_t) { return kMaxPart; }

// Shared argument checks; fills the geometry and (make_cols) the slot -> column table.
inline int make_geo(int64_t m, int32_t t, int32_t c, int32_t c_in, int32_t c_out, const float* geom6, int use_absolute_xyz,
                    int with_distance, Geo* g) {
  if (m < 0 || !geom6 || t < 1 || t > kMaxT || c < 3 || c > 6) return SPX_ERR_INVALID_ARG;
  const int rc = make_cols(c, c_in, c_out, use_absolute_xyz, with_distance, g->col);
  if (rc != SPX_OK) return rc;
  if (m * (int64_t)t * c >= (1ll << 40)) return SPX_ERR_TOO_LARGE;
  g->vx = geom6[0];
  g->vy = geom6[1];
  g->vz = geom6[2];
  g->ox = geom6[3];
  g->oy = geom6[4];
  g->oz = geom6[5];
  g->c = c;
  g->c_in = c_in;
  g->t = t;
  return SPX_OK;
}

}  // namespace

extern "C" size_t spx_pillar_vfe_stats_len(void) { return kStatsLen; }

extern "C" size_t spx_pillar_vfe_ws_bytes(int64_t m) {
  const size_t np = (size_t)n_part_of(m < 0 ? 0 : m);
  const size_t fwd = spx_align(np * kStat * 8) + spx_align(2 * kCout * 8);
  const size_t bwd = spx_align(np * kAcc * kCout * 8);
  return fwd > bwd ? fwd : bwd;
}

extern "C" int spx_pillar_vfe_fwd(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t m,
                                  const int64_t* d_n, int32_t t, int32_t c, const float* weight, int32_t c_in,
                                  int32_t c_out, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                                  const float* geom6, int use_absolute_xyz, int with_distance, int training, float* out,
                                  uint8_t* arg, float* save_mean, float* save_invstd, double* stats, void* ws,
                                  size_t ws_bytes, spx_stream_t stream) {
  Geo g;
  const int rc = make_geo(m, t, c, c_in, c_out, geom6, use_absolute_xyz, with_distance, &g);
  if (rc != SPX_OK) return rc;
  if (!weight || !gamma || !beta) return SPX_ERR_INVALID_ARG;
  if (training && (!save_mean || !save_invstd || !stats)) return SPX_ERR_INVALID_ARG;
  if (!training && (!running_mean || !running_var)) return SPX_ERR_INVALID_ARG;
  if ((running_mean == nullptr) != (running_var == nullptr)) return SPX_ERR_INVALID_ARG;
  if (m > 0 && (!voxels || !num_points || !coords || !out || !arg)) return SPX_ERR_INVALID_ARG;
  if (m == 0) return SPX_OK;
  if (training && (!ws || ws_bytes < spx_pillar_vfe_ws_bytes(m))) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  In in{voxels, num_points, coords, d_n, m};
  BN bn{weight, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps};
  const double* ss = nullptr;
  if (training) {
    const int np = n_part_of(m);
    double* part = reinterpret_cast<double*>(ws);
    double* ssw = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + spx_align((size_t)np * kStat * 8));
    hipLaunchKernelGGL(k_stats, dim3((unsigned)np), dim3(kBlock), 0, s, in, g, part);
    hipLaunchKernelGGL(k_stats_final, dim3(1), dim3(kBlock), 0, s, in, g, bn, part, np, stats, ssw, save_mean, save_invstd);
    ss = ssw;
  }
  const int64_t tiles = (m + kTileP - 1) / kTileP;
  if (tiles >= (1ll << 31)) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_fwd, dim3((unsigned)tiles), dim3(kBlock), 0, s, in, g, bn, ss, out, arg);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_pillar_vfe_bwd(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t m,
                                  const int64_t* d_n, int32_t t, int32_t c, const float* weight, int32_t c_in,
                                  int32_t c_out, const float* gamma, const float* running_mean, const float* running_var,
                                  float eps, const float* geom6, int use_absolute_xyz, int with_distance, int training,
                                  const float* out, const uint8_t* arg, const float* d_out, const double* stats,
                                  float* d_weight, float* d_gamma, float* d_beta, void* ws, size_t ws_bytes,
                                  spx_stream_t stream) {
  Geo g;
  const int rc = make_geo(m, t, c, c_in, c_out, geom6, use_absolute_xyz, with_distance, &g);
  if (rc != SPX_OK) return rc;
  if (!weight || !gamma || !d_weight || !d_gamma || !d_beta) return SPX_ERR_INVALID_ARG;
  if (training ? !stats : (!running_mean || !running_var)) return SPX_ERR_INVALID_ARG;
  if (m > 0 && (!voxels || !num_points || !coords || !out || !arg || !d_out)) return SPX_ERR_INVALID_ARG;
  if (!ws || ws_bytes < spx_pillar_vfe_ws_bytes(m)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  In in{voxels, num_points, coords, d_n, m};
  BN bn{weight, gamma, nullptr, const_cast<float*>(running_mean), const_cast<float*>(running_var), nullptr, 0.f, eps};
  Bwd<uint8_t> b{out, d_out, arg, stats, training};
  double* part = reinterpret_cast<double*>(ws);
  int np = 0;                     // m == 0: the gradients are zeros, from pfn_k_bwd_final alone
  if (m > 0) {
    np = n_part_of(m);
    hipLaunchKernelGGL(k_bwd_gather, dim3((unsigned)np), dim3(kBlock), 0, s, in, g, bn, b, part);
  }
  hipLaunchKernelGGL((pfn_k_bwd_final<Geo, uint8_t>), dim3(1), dim3(kBlock), 0, s, g, bn, b, part, np, d_weight, d_gamma,
                     d_beta);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
