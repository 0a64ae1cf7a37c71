// pointnet2.hip — the point-sampling op family of the fork's 3DSSD-style model (include/spx.h §11): furthest point
// sampling, ball query, grouping / gather, three-NN and three-point interpolation.  Replaces the pointnet2_batch
// extension, reference pcdet/ops/pointnet2/pointnet2_batch/src/{sampling,ball_query,group_points,interpolate}_gpu.cu
// (python side pointnet2_utils.py).
//
// Pinned semantics (tests/pointnet2_ref.py restates all of it in float32 numpy):
//   - every distance is ((dx*dx) + (dy*dy)) + (dz*dz) with dx = a.x - b.x, rounded after each operation: FMA
//     contraction is OFF for this whole file (device code contracts by default).  Whether the reference's nvcc build
//     contracted those lines cannot be checked without a CUDA device; the uncontracted source order is what is pinned.
//     (The __f*_rn intrinsics are plain operators in HIP's headers, compiled outside this pragma, so they are not used.)
//   - the weighted FPS ranks (float)((double)temp * max((double)w, 1e-12)): the reference writes max(weights[k], 1e-12)
//     with a double literal, which CUDA's mixed max(float, double) overload evaluates in double.
//   - FPS ties: the reference scans point k in thread k mod bs (bs = min(2^floor(log2 N), 1024)), each thread keeping
//     its first maximum, then merges the threads in a left-preferring LDS tree.  Among equal maxima the winner is the
//     k with the smallest (bitrev_log2(bs)(k mod bs), k div bs).  That priority is the low half of a 64-bit key whose
//     high half is the value as an order-preserving uint, so any reduction order gives the reference's pick.  A thread
//     whose values are all <= -1 reports nothing (the reference's `best = -1` start); no candidate at all picks 0.
#include "sorted_runs.h"

#pragma clang fp contract(off)

#include "point_dist.h"   // sq_dist, ord_f32: after the pragma, which covers them

namespace {

constexpr int kFpsMaxThreads = 1024;
constexpr int kFpsRegPoints = 16;   // register-resident FPS: up to 16 points per thread, N <= 16384

int fps_log2_bs(int64_t n) {   // the reference's opt_n_threads, as log2
  int l = 0;
  while (l < 10 && (int64_t(2) << l) <= n) ++l;
  return l;
}

// MODE bit 0: weights; bit 1: distance matrix (else xyz).  PPT > 0: points and temp in registers (xyz only);
// PPT == 0: temp in the workspace, points streamed every round.  One workgroup of bs = 2^L threads per frame; thread t
// owns k = t + j*bs, the reference's own layout, so a strict `>` keeps each thread's best-priority maximum.
template <int MODE, int PPT>
__global__ __launch_bounds__(kFpsMaxThreads) void k_fps(const float* __restrict__ data, const float* __restrict__ weights,
                                                        float* __restrict__ temp_ws, int N, int npoint, int L,
                                                        int32_t* __restrict__ idx) {
  constexpr bool WEI = (MODE & 1) != 0, MAT = (MODE & 2) != 0;
  constexpr int R = PPT > 0 ? PPT : 1;
  __shared__ uint64_t s_key[2][kFpsMaxThreads / SPX_WAVE];
  __shared__ float4 s_pt[2][kFpsMaxThreads / SPX_WAVE];   // winner of each wave: x, y, z, k

  const int b = blockIdx.x, t = threadIdx.x, bs = 1 << L;
  const float* P = data + (size_t)b * N * (MAT ? (size_t)N : 3);
  const float* W = WEI ? weights + (size_t)b * N : nullptr;
  float* T = temp_ws ? temp_ws + (size_t)b * N : nullptr;
  int32_t* out = idx + (size_t)b * npoint;
  const uint32_t hi = L ? (__brev((uint32_t)t) >> (32 - L)) << 22 : 0u;
  const int lane = t & (SPX_WAVE - 1), wv = t / SPX_WAVE, nw = (bs + SPX_WAVE - 1) / SPX_WAVE;
  const int wred = bs < SPX_WAVE ? bs : SPX_WAVE;

  float px[R], py[R], pz[R], pt[R];
  float pw[R];
  if (PPT > 0) {   // slots past N get temp = -inf: they never win and need no branch in the round loop
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int k = t + j * bs, kk = k < N ? k : 0;
      pt[j] = k < N ? 1e10f : -INFINITY;
      px[j] = P[3 * kk];
      py[j] = P[3 * kk + 1];
      pz[j] = P[3 * kk + 2];
      pw[j] = WEI ? W[kk] : 0.f;
    }
  } else {
    for (int k = t; k < N; k += bs) T[k] = 1e10f;
  }

  int old = 0;
  float ox = 0.f, oy = 0.f, oz = 0.f;
  if (!MAT) {
    ox = P[0];
    oy = P[1];
    oz = P[2];
  }
  const float x0 = ox, y0 = oy, z0 = oz;
  int r0 = 0;
  if (!WEI) {
    if (t == 0) out[0] = 0;
    r0 = 1;
  }
  for (int r = r0; r < npoint; ++r) {
    float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    int bj = 0;
    const float* row = MAT ? P + (size_t)old * N : nullptr;
    if (WEI && r == 0) {                       // weighted forms: round 0 is the arg-max of the raw weights
      for (int j = 0, k = t; k < N; ++j, k += bs) {
        const float v = W[k];
        if (v > best) {
          best = v;
          bj = j;
          if (!MAT) {
            bx = P[3 * k];
            by = P[3 * k + 1];
            bz = P[3 * k + 2];
          }
        }
      }
    } else if (PPT > 0) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float d = fminf(sq_dist(px[j], py[j], pz[j], ox, oy, oz), pt[j]);
        pt[j] = d;
        const float v = WEI ? (float)((double)d * fmax((double)pw[j], 1e-12)) : d;
        if (v > best) {
          best = v;
          bj = j;
          bx = px[j];
          by = py[j];
          bz = pz[j];
        }
      }
    } else {
      for (int j = 0, k = t; k < N; ++j, k += bs) {
        float x = 0.f, y = 0.f, z = 0.f, d;
        if (MAT) {
          d = row[k];
        } else {
          x = P[3 * k];
          y = P[3 * k + 1];
          z = P[3 * k + 2];
          d = sq_dist(x, y, z, ox, oy, oz);
        }
        d = fminf(d, T[k]);
        T[k] = d;
        const float v = WEI ? (float)((double)d * fmax((double)W[k], 1e-12)) : d;
        if (v > best) {
          best = v;
          bj = j;
          bx = x;
          by = y;
          bz = z;
        }
      }
    }
    const uint64_t mine = best > -1.f ? ((uint64_t)ord_f32(best) << 32) | (uint32_t)~(hi | (uint32_t)bj) : 0ull;
    uint64_t wk = mine;
    for (int off = 1; off < wred; off <<= 1) {
      const uint64_t o = __shfl_xor(wk, off);
      wk = o > wk ? o : wk;
    }
    const int buf = r & 1;
    if (mine == wk && (wk != 0ull || lane == 0)) {
      s_key[buf][wv] = wk;
      s_pt[buf][wv] = make_float4(bx, by, bz, __int_as_float(t + bj * bs));
    }
    __syncthreads();   // double-buffered slots: the next round writes the other half, so one barrier per round
    uint64_t gk = 0ull;
    int gw = 0;
    for (int i = 0; i < nw; ++i) {
      const uint64_t kk = s_key[buf][i];
      if (kk > gk) {
        gk = kk;
        gw = i;
      }
    }
    if (gk == 0ull) {
      old = 0;
      ox = x0;
      oy = y0;
      oz = z0;
    } else {
      const float4 w = s_pt[buf][gw];
      old = __float_as_int(w.w);
      ox = w.x;
      oy = w.y;
      oz = w.z;
    }
    if (t == 0) out[r] = old;
  }
}

template <int MODE, int PPT>
void launch_fps_t(const float* data, const float* w, float* temp, int b, int n, int npoint, int L, int32_t* idx,
                  hipStream_t s) {
  hipLaunchKernelGGL((k_fps<MODE, PPT>), dim3(b), dim3(1 << L), 0, s, data, w, temp, n, npoint, L, idx);
}

template <int MODE>
void launch_fps_reg(const float* data, const float* w, int b, int n, int npoint, int L, int32_t* idx, hipStream_t s) {
  const int per = (int)((n + (1 << L) - 1) >> L);
  if (per <= 1) launch_fps_t<MODE, 1>(data, w, nullptr, b, n, npoint, L, idx, s);
  else if (per <= 2) launch_fps_t<MODE, 2>(data, w, nullptr, b, n, npoint, L, idx, s);
  else if (per <= 4) launch_fps_t<MODE, 4>(data, w, nullptr, b, n, npoint, L, idx, s);
  else if (per <= 8) launch_fps_t<MODE, 8>(data, w, nullptr, b, n, npoint, L, idx, s);
  else launch_fps_t<MODE, 16>(data, w, nullptr, b, n, npoint, L, idx, s);
}

bool fps_in_registers(int64_t n) { return n <= (int64_t)kFpsMaxThreads * kFpsRegPoints; }

// ---------------------------------------------------------------------------------------------- ball query
constexpr int kBqThreads = 256;
constexpr int kBqChunk = 512;

// One thread per query, a workgroup's 256 queries (one frame) share chunks of the frame's points staged in LDS; the
// scan stops once every query of the workgroup holds nsample hits.
__global__ __launch_bounds__(kBqThreads) void k_ball_query(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                           int N, int M, int nsample, float r_in2, float r_out2,
                                                           int32_t* __restrict__ idx_cnt, int32_t* __restrict__ idx) {
  __shared__ float s_p[kBqChunk * 3];
  const int b = blockIdx.y, q = blockIdx.x * kBqThreads + threadIdx.x;
  const bool live = q < M;
  const float* X = xyz + (size_t)b * N * 3;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  int32_t* o = idx + ((size_t)b * M + (live ? q : 0)) * nsample;
  if (live) {
    const float* c = new_xyz + ((size_t)b * M + q) * 3;
    qx = c[0];
    qy = c[1];
    qz = c[2];
  }
  int cnt = 0;
  for (int base = 0; base < N; base += kBqChunk) {
    if (__syncthreads_count(live && cnt < nsample) == 0) break;
    const int len = min(kBqChunk, N - base);
    for (int i = threadIdx.x; i < len * 3; i += kBqThreads) s_p[i] = X[(size_t)base * 3 + i];
    __syncthreads();
    if (live) {
      for (int i = 0; i < len && cnt < nsample; ++i) {
        const float d2 = sq_dist(qx, qy, qz, s_p[3 * i], s_p[3 * i + 1], s_p[3 * i + 2]);
        if (d2 >= r_in2 && d2 < r_out2) o[cnt++] = base + i;
      }
    }
  }
  if (!live) return;
  idx_cnt[(size_t)b * M + q] = cnt;
  if (cnt == 0) {
    for (int l = 0; l < nsample; ++l) o[l] = 0;
  } else {
    for (int l = 0; cnt < nsample; ++l, ++cnt) o[cnt] = o[l];
  }
}

// ---------------------------------------------------------------------------------------------- group / gather
// out[b][c][e] = f[b][c][idx[b][e]], e over the M*S entries of a frame; an index outside [0, N) reads as 0.
__global__ __launch_bounds__(256) void k_group(const float* __restrict__ f, const int32_t* __restrict__ idx, int C, int N,
                                               int64_t E, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, b = blockIdx.z;
  if (e >= E) return;
  const int32_t k = idx[(size_t)b * E + e];
  out[((size_t)b * C + c) * E + e] = (k >= 0 && k < N) ? f[((size_t)b * C + c) * N + k] : 0.f;
}

// Deterministic scatter-add backward on sorted runs (sorted_runs.h): the key of an entry is its target b*N + k, then one
// thread per (b, c, k) sums its run in ascending entry order — no float atomics.
__global__ __launch_bounds__(256) void k_scatter_keys(const int32_t* __restrict__ idx, int64_t total, int64_t per_frame,
                                                      int N, uint32_t sentinel, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ vals) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int32_t k = idx[e];
  keys[e] = (k >= 0 && k < N) ? (uint32_t)((e / per_frame) * N + k) : sentinel;
  vals[e] = (uint32_t)e;
}

// grad_f[b][c][k] = sum over the sorted run of target b*N + k of g[b][c][e / G] * (w ? w[e] : 1), e the entry
// (G = 1 for grouping: e indexes the (M, S) grid; G = 3 for interpolation: e = point*3 + neighbour).
__global__ __launch_bounds__(256) void k_scatter_sum(const float* __restrict__ g, const float* __restrict__ w,
                                                     const uint32_t* __restrict__ vals, const int32_t* __restrict__ start,
                                                     const int32_t* __restrict__ end, int C, int N, int64_t per_frame,
                                                     int G, float* __restrict__ grad) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, b = blockIdx.z;
  if (k >= N) return;
  const size_t key = (size_t)b * N + k;
  const int32_t s = start[key], e = end[key];
  const int64_t cols = per_frame / G;
  const float* gb = g + ((size_t)b * C + c) * cols;
  float acc = 0.f;
  for (int32_t p = s; p < e; ++p) {
    const int64_t ent = vals[p], local = ent - (int64_t)b * per_frame;
    const float gv = gb[local / G];
    acc += w ? gv * w[ent] : gv;
  }
  grad[((size_t)b * C + c) * N + k] = acc;
}

// idx [B, per_frame] int32 (targets in [0, N)), g [B, C, per_frame / G], w [B, per_frame] or NULL -> grad [B, C, N]
int scatter_bwd(const float* g, const int32_t* idx, const float* w, int b, int c, int n, int64_t per_frame, int G,
                float* grad, void* ws, size_t ws_bytes, hipStream_t s) {
  const int64_t total = (int64_t)b * per_frame, targets = (int64_t)b * n;
  if (total >= (int64_t)INT32_MAX || targets >= (int64_t)UINT32_MAX) return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < spx_sorted_runs_layout(total, targets, nullptr, nullptr)) return SPX_ERR_WORKSPACE;
  SortedRunsWs L;
  spx_sorted_runs_layout(total, targets, (char*)ws, &L);
  if (total > 0)
    hipLaunchKernelGGL(k_scatter_keys, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, idx, total, per_frame, n,
                       (uint32_t)targets, L.keys_in, L.vals_in);
  if (const int e = spx_sorted_runs(L, total, targets, s); e != SPX_OK) return e;
  hipLaunchKernelGGL(k_scatter_sum, dim3((unsigned)((n + 255) / 256), (unsigned)c, (unsigned)b), dim3(256), 0, s, g, w,
                     L.vals_out, L.start, L.end, c, n, per_frame, G, grad);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

// ---------------------------------------------------------------------------------------------- three-NN / interpolate
constexpr int kNnThreads = 256;
constexpr int kNnChunk = 512;

__global__ __launch_bounds__(kNnThreads) void k_three_nn(const float* __restrict__ unknown, const float* __restrict__ known,
                                                         int n, int m, float* __restrict__ dist2,
                                                         int32_t* __restrict__ idx) {
  __shared__ float s_p[kNnChunk * 3];
  const int b = blockIdx.y, q = blockIdx.x * kNnThreads + threadIdx.x;
  const bool live = q < n;
  const float* K = known + (size_t)b * m * 3;
  float ux = 0.f, uy = 0.f, uz = 0.f;
  if (live) {
    const float* u = unknown + ((size_t)b * n + q) * 3;
    ux = u[0];
    uy = u[1];
    uz = u[2];
  }
  float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;   // the reference starts at 1e40 in double: same order, inf out
  int i1 = 0, i2 = 0, i3 = 0;
  for (int base = 0; base < m; base += kNnChunk) {
    const int len = min(kNnChunk, m - base);
    __syncthreads();
    for (int i = threadIdx.x; i < len * 3; i += kNnThreads) s_p[i] = K[(size_t)base * 3 + i];
    __syncthreads();
    if (!live) continue;
    for (int i = 0; i < len; ++i) {
      const float d = sq_dist(ux, uy, uz, s_p[3 * i], s_p[3 * i + 1], s_p[3 * i + 2]);
      if (d < b1) {
        b3 = b2; i3 = i2;
        b2 = b1; i2 = i1;
        b1 = d; i1 = base + i;
      } else if (d < b2) {
        b3 = b2; i3 = i2;
        b2 = d; i2 = base + i;
      } else if (d < b3) {
        b3 = d; i3 = base + i;
      }
    }
  }
  if (!live) return;
  const size_t o = ((size_t)b * n + q) * 3;
  dist2[o] = b1;
  dist2[o + 1] = b2;
  dist2[o + 2] = b3;
  idx[o] = i1;
  idx[o + 1] = i2;
  idx[o + 2] = i3;
}

__global__ __launch_bounds__(256) void k_three_interp(const float* __restrict__ f, const int32_t* __restrict__ idx,
                                                      const float* __restrict__ w, int C, int m, int n,
                                                      float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (j >= n) return;
  const float* fr = f + ((size_t)b * C + c) * m;
  const size_t e = ((size_t)b * n + j) * 3;
  float acc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int32_t k = idx[e + i];
    acc[i] = w[e + i] * ((k >= 0 && k < m) ? fr[k] : 0.f);
  }
  out[((size_t)b * C + c) * n + j] = (acc[0] + acc[1]) + acc[2];
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" size_t spx_furthest_point_sample_ws_bytes(int32_t b, int64_t n) {
  return (b <= 0 || n <= 0 || fps_in_registers(n)) ? 0 : spx_align((size_t)b * (size_t)n * 4);
}

extern "C" int spx_furthest_point_sample(const float* xyz, const float* weights, int32_t b, int64_t n, int32_t npoint,
                                         int32_t* idx, void* ws, size_t ws_bytes, spx_stream_t stream) {
  if (b < 0 || n <= 0 || npoint < 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || npoint == 0) return SPX_OK;
  if (!xyz || !idx) return SPX_ERR_INVALID_ARG;
  if (n >= INT32_MAX / 3 || (int64_t)b * n >= INT32_MAX) return SPX_ERR_TOO_LARGE;
  const int L = fps_log2_bs(n);
  hipStream_t s = spx_s(stream);
  if (fps_in_registers(n)) {
    if (weights) launch_fps_reg<1>(xyz, weights, b, (int)n, npoint, L, idx, s);
    else launch_fps_reg<0>(xyz, weights, b, (int)n, npoint, L, idx, s);
  } else {
    if (!ws || ws_bytes < spx_furthest_point_sample_ws_bytes(b, n)) return SPX_ERR_WORKSPACE;
    if (weights) launch_fps_t<1, 0>(xyz, weights, (float*)ws, b, (int)n, npoint, L, idx, s);
    else launch_fps_t<0, 0>(xyz, weights, (float*)ws, b, (int)n, npoint, L, idx, s);
  }
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_furthest_point_sample_matrix_ws_bytes(int32_t b, int64_t n) {
  return (b <= 0 || n <= 0) ? 0 : spx_align((size_t)b * (size_t)n * 4);
}

extern "C" int spx_furthest_point_sample_matrix(const float* matrix, const float* weights, int32_t b, int64_t n,
                                                int32_t npoint, int32_t* idx, void* ws, size_t ws_bytes,
                                                spx_stream_t stream) {
  if (b < 0 || n <= 0 || npoint < 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || npoint == 0) return SPX_OK;
  if (!matrix || !idx) return SPX_ERR_INVALID_ARG;
  if (n >= INT32_MAX || (int64_t)b * n >= INT32_MAX) return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < spx_furthest_point_sample_matrix_ws_bytes(b, n)) return SPX_ERR_WORKSPACE;
  const int L = fps_log2_bs(n);
  hipStream_t s = spx_s(stream);
  if (weights) launch_fps_t<3, 0>(matrix, weights, (float*)ws, b, (int)n, npoint, L, idx, s);
  else launch_fps_t<2, 0>(matrix, weights, (float*)ws, b, (int)n, npoint, L, idx, s);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_ball_query(const float* xyz, const float* new_xyz, int32_t b, int64_t n, int64_t m, float r_in,
                              float r_out, int32_t nsample, int32_t* idx_cnt, int32_t* idx, spx_stream_t stream) {
  if (b < 0 || n < 0 || m < 0 || nsample <= 0 || !(r_in >= 0.f) || !(r_out >= 0.f)) return SPX_ERR_INVALID_ARG;
  if (b == 0 || m == 0) return SPX_OK;
  if (!new_xyz || !idx_cnt || !idx || (n > 0 && !xyz)) return SPX_ERR_INVALID_ARG;
  if (n >= INT32_MAX / 3 || m >= INT32_MAX || b > 65535 || m * (int64_t)nsample * b >= ((int64_t)1 << 40))
    return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_ball_query, dim3((unsigned)((m + kBqThreads - 1) / kBqThreads), (unsigned)b), dim3(kBqThreads), 0,
                     spx_s(stream), xyz, new_xyz, (int)n, (int)m, nsample, r_in * r_in, r_out * r_out,
                     idx_cnt, idx);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_group_points(const float* features, const int32_t* idx, int32_t b, int32_t c, int64_t n, int64_t m,
                                int32_t nsample, float* out, spx_stream_t stream) {
  if (b < 0 || c < 0 || n <= 0 || m < 0 || nsample <= 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || c == 0 || m == 0) return SPX_OK;
  if (!features || !idx || !out) return SPX_ERR_INVALID_ARG;
  const int64_t e = m * nsample;
  if (n >= INT32_MAX || e >= INT32_MAX || b > 65535 || c > 65535) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_group, dim3((unsigned)((e + 255) / 256), (unsigned)c, (unsigned)b), dim3(256), 0, spx_s(stream),
                     features, idx, c, (int)n, e, out);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_group_points_bwd_ws_bytes(int32_t b, int64_t n, int64_t m, int32_t nsample) {
  if (b <= 0 || n <= 0 || m < 0 || nsample <= 0) return 0;
  return spx_sorted_runs_layout((int64_t)b * m * nsample, (int64_t)b * n, nullptr, nullptr);
}

extern "C" int spx_group_points_bwd(const float* grad_out, const int32_t* idx, int32_t b, int32_t c, int64_t n, int64_t m,
                                    int32_t nsample, float* grad_features, void* ws, size_t ws_bytes,
                                    spx_stream_t stream) {
  if (b < 0 || c < 0 || n <= 0 || m < 0 || nsample <= 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || c == 0) return SPX_OK;
  if (!grad_features || (m > 0 && (!grad_out || !idx))) return SPX_ERR_INVALID_ARG;
  if (n >= INT32_MAX || b > 65535 || c > 65535) return SPX_ERR_TOO_LARGE;
  return scatter_bwd(grad_out, idx, nullptr, b, c, (int)n, m * nsample, 1, grad_features, ws, ws_bytes, spx_s(stream));
}

extern "C" int spx_three_nn(const float* unknown, const float* known, int32_t b, int64_t n, int64_t m, float* dist2,
                            int32_t* idx, spx_stream_t stream) {
  if (b < 0 || n < 0 || m < 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || n == 0) return SPX_OK;
  if (!unknown || !dist2 || !idx || (m > 0 && !known)) return SPX_ERR_INVALID_ARG;
  if (n >= INT32_MAX / 3 || m >= INT32_MAX / 3 || b > 65535) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_three_nn, dim3((unsigned)((n + kNnThreads - 1) / kNnThreads), (unsigned)b), dim3(kNnThreads), 0,
                     spx_s(stream), unknown, known, (int)n, (int)m, dist2, idx);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_three_interpolate(const float* features, const int32_t* idx, const float* weight, int32_t b, int32_t c,
                                     int64_t m, int64_t n, float* out, spx_stream_t stream) {
  if (b < 0 || c < 0 || m <= 0 || n < 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || c == 0 || n == 0) return SPX_OK;
  if (!features || !idx || !weight || !out) return SPX_ERR_INVALID_ARG;
  if (m >= INT32_MAX || n >= INT32_MAX / 3 || b > 65535 || c > 65535) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_three_interp, dim3((unsigned)((n + 255) / 256), (unsigned)c, (unsigned)b), dim3(256), 0,
                     spx_s(stream), features, idx, weight, c, (int)m, (int)n, out);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_three_interpolate_bwd_ws_bytes(int32_t b, int64_t m, int64_t n) {
  if (b <= 0 || m <= 0 || n < 0) return 0;
  return spx_sorted_runs_layout((int64_t)b * n * 3, (int64_t)b * m, nullptr, nullptr);
}

extern "C" int spx_three_interpolate_bwd(const float* grad_out, const int32_t* idx, const float* weight, int32_t b,
                                         int32_t c, int64_t m, int64_t n, float* grad_features, void* ws, size_t ws_bytes,
                                         spx_stream_t stream) {
  if (b < 0 || c < 0 || m <= 0 || n < 0) return SPX_ERR_INVALID_ARG;
  if (b == 0 || c == 0) return SPX_OK;
  if (!grad_features || (n > 0 && (!grad_out || !idx || !weight))) return SPX_ERR_INVALID_ARG;
  if (m >= INT32_MAX || b > 65535 || c > 65535) return SPX_ERR_TOO_LARGE;
  return scatter_bwd(grad_out, idx, weight, b, c, (int)m, n * 3, 3, grad_features, ws, ws_bytes, spx_s(stream));
}
