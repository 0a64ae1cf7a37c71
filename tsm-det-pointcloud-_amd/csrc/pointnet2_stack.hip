// pointnet2_stack.hip — the stacked (ragged-batch) point ops (include/spx.h §18): ball query, grouping, furthest point
// sampling, three-NN and three-point interpolation over (N1 + N2 + ..., C) tensors with per-frame counts.  Replaces the
// rest of the pointnet2_stack extension, reference pcdet/ops/pointnet2/pointnet2_stack/src/{ball_query,group_points,
// sampling,interpolate}_gpu.cu (python side pointnet2_utils.py); the voxel-query kernels of that extension are
// csrc/voxel_query.hip.
//
// Pinned semantics (tests/pointnet2_stack_ref.py restates all of it in float32 numpy):
//   - every distance is ((dx*dx) + (dy*dy)) + (dz*dz) with dx = a.x - b.x, rounded after each operation: FMA contraction
//     is OFF for this whole file, as in pointnet2.hip and for the same reason (whether the reference's nvcc build
//     contracted those lines cannot be checked without a CUDA device; the uncontracted source order is what is pinned).
//   - the counts live on the device and are never read by the host.  Every kernel turns them into frame starts itself
//     (an exclusive prefix sum in LDS, b <= 256, clamped to the tensor's row count so that no count, however wrong, makes
//     a kernel leave its tensors).  Rows past the sum of the counts are DEAD (static-capacity mode): dead query rows get
//     a fixed fill, dead source rows are never read and get a zero gradient.
//   - a kernel whose workgroup shares LDS-staged source points (ball query, three-NN) needs all its queries in ONE
//     frame: workgroup w is mapped on the device to a (frame, tile of 256 queries) pair by walking the frames' tile
//     counts; the grid is sized to the host-known bound ceil(m_rows / 256) + b and surplus workgroups skip the scan.
//   - stack FPS ties: the reference always launches 1024 threads, whatever the frame's size, so the winner among equal
//     maxima is the k with the smallest (bitrev10(k mod 1024), k div 1024): the 64-bit key of pointnet2.hip with L = 10.
#include "sorted_runs.h"

#pragma clang fp contract(off)

#include "point_dist.h"   // sq_dist, ord_f32: after the pragma, which covers them

namespace {

constexpr int kMaxFrames = 256;
constexpr int kTile = 256;     // queries per workgroup
constexpr int kChunk = 512;    // source points staged in LDS at a time
constexpr int kRunChunk = 128; // sorted entries per partial sum of the backward

// s[0 .. b] = exclusive prefix sums of max(cnt, 0), each clamped to `rows`: s[f] is the first row of frame f and s[b]
// the number of live rows.  Called by every thread of the workgroup; ends with a barrier.
__device__ void frame_starts(const int32_t* __restrict__ cnt, int b, int64_t rows, int32_t* s) {
  for (int i = threadIdx.x; i < b; i += blockDim.x) s[i + 1] = cnt[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t acc = 0;
    s[0] = 0;
    for (int i = 1; i <= b; ++i) {
      const int32_t c = s[i];
      if (c > 0) acc += c;
      s[i] = (int32_t)(acc < rows ? acc : rows);
    }
  }
  __syncthreads();
}

// the frame f with s[f] <= row < s[f + 1]; row must be below s[b]
__device__ __forceinline__ int frame_of(int32_t row, const int32_t* s, int b) {
  int lo = 0, hi = b;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Workgroup w -> (frame, tile) over frames cut into tiles of kTile rows; ft[0] = -1 for a surplus workgroup.
__device__ void tile_of(const int32_t* s, int b, int w, int32_t* ft) {
  if (threadIdx.x == 0) {
    int acc = 0, f = -1, t = 0;
    for (int i = 0; i < b; ++i) {
      const int nt = (s[i + 1] - s[i] + kTile - 1) / kTile;
      if (w < acc + nt) {
        f = i;
        t = w - acc;
        break;
      }
      acc += nt;
    }
    ft[0] = f;
    ft[1] = t;
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------- ball query
// One thread per query; the queries of a workgroup lie in one frame and share chunks of that frame's points staged in
// LDS; the scan stops once every live query of the workgroup holds nsample hits.
__global__ __launch_bounds__(kTile) void k_stack_ball_query(const float* __restrict__ xyz, const int32_t* __restrict__ xyz_cnt,
                                                            const float* __restrict__ new_xyz,
                                                            const int32_t* __restrict__ new_cnt, int b, int n_rows,
                                                            int m_rows, int nsample, float r2, int32_t* __restrict__ idx,
                                                            uint8_t* __restrict__ empty) {
  __shared__ int32_t s_n[kMaxFrames + 1], s_m[kMaxFrames + 1], s_ft[2];
  __shared__ float s_p[kChunk * 3];
  frame_starts(xyz_cnt, b, n_rows, s_n);
  frame_starts(new_cnt, b, m_rows, s_m);
  tile_of(s_m, b, blockIdx.x, s_ft);
  const int f = s_ft[0];
  if (f >= 0) {
    const int local = s_ft[1] * kTile + threadIdx.x;
    const bool live = local < s_m[f + 1] - s_m[f];
    const int q = s_m[f] + (live ? local : 0);
    const int N = s_n[f + 1] - s_n[f];
    const float* X = xyz + (size_t)s_n[f] * 3;
    int32_t* o = idx + (size_t)q * nsample;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
      qx = new_xyz[(size_t)q * 3];
      qy = new_xyz[(size_t)q * 3 + 1];
      qz = new_xyz[(size_t)q * 3 + 2];
    }
    int cnt = 0, first = 0;
    for (int base = 0; base < N; base += kChunk) {
      if (__syncthreads_count(live && cnt < nsample) == 0) break;
      const int len = min(kChunk, N - base);
      for (int i = threadIdx.x; i < len * 3; i += kTile) s_p[i] = X[(size_t)base * 3 + i];
      __syncthreads();
      if (live) {
        for (int i = 0; i < len && cnt < nsample; ++i) {
          const float d2 = sq_dist(qx, qy, qz, s_p[3 * i], s_p[3 * i + 1], s_p[3 * i + 2]);
          if (d2 < r2) {
            if (cnt == 0) first = base + i;
            o[cnt++] = base + i;
          }
        }
      }
    }
    if (live) {
      empty[q] = cnt == 0;
      for (; cnt < nsample; ++cnt) o[cnt] = first;   // unfilled slots: the first hit; an empty ball: zeros
    }
  }
  // dead rows, shared among all workgroups
  for (int64_t r = (int64_t)s_m[b] + (int64_t)blockIdx.x * kTile + threadIdx.x; r < m_rows; r += (int64_t)gridDim.x * kTile) {
    for (int l = 0; l < nsample; ++l) idx[(size_t)r * nsample + l] = 0;
    empty[r] = 1;
  }
}

// ---------------------------------------------------------------------------------------------- three-NN
__global__ __launch_bounds__(kTile) void k_stack_three_nn(const float* __restrict__ unknown,
                                                          const int32_t* __restrict__ unknown_cnt,
                                                          const float* __restrict__ known,
                                                          const int32_t* __restrict__ known_cnt, int b, int n_rows,
                                                          int m_rows, float* __restrict__ dist2, int32_t* __restrict__ idx) {
  __shared__ int32_t s_n[kMaxFrames + 1], s_m[kMaxFrames + 1], s_ft[2];
  __shared__ float s_p[kChunk * 3];
  frame_starts(unknown_cnt, b, n_rows, s_n);
  frame_starts(known_cnt, b, m_rows, s_m);
  tile_of(s_n, b, blockIdx.x, s_ft);
  const int f = s_ft[0];
  if (f >= 0) {
    const int local = s_ft[1] * kTile + threadIdx.x;
    const bool live = local < s_n[f + 1] - s_n[f];
    const int q = s_n[f] + (live ? local : 0);
    const int start = s_m[f], M = s_m[f + 1] - start;
    const float* K = known + (size_t)start * 3;
    float ux = 0.f, uy = 0.f, uz = 0.f;
    if (live) {
      ux = unknown[(size_t)q * 3];
      uy = unknown[(size_t)q * 3 + 1];
      uz = unknown[(size_t)q * 3 + 2];
    }
    float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;   // the reference starts at 1e40 in double: same order, inf out
    int i1 = 0, i2 = 0, i3 = 0;
    for (int base = 0; base < M; base += kChunk) {
      const int len = min(kChunk, M - base);
      __syncthreads();
      for (int i = threadIdx.x; i < len * 3; i += kTile) s_p[i] = K[(size_t)base * 3 + i];
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
    if (live) {
      const size_t o = (size_t)q * 3;
      dist2[o] = b1;
      dist2[o + 1] = b2;
      dist2[o + 2] = b3;
      idx[o] = start + i1;
      idx[o + 1] = start + i2;
      idx[o + 2] = start + i3;
    }
  }
  for (int64_t r = (int64_t)s_n[b] + (int64_t)blockIdx.x * kTile + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * kTile) {
    for (int l = 0; l < 3; ++l) {
      dist2[(size_t)r * 3 + l] = INFINITY;
      idx[(size_t)r * 3 + l] = 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------- grouping / interpolation
// out[m][c][s] = features[start(frame of m) + idx[m][s]][c]; an index outside the frame reads as 0, a dead row is 0.
__global__ __launch_bounds__(256) void k_stack_group(const float* __restrict__ feat, const int32_t* __restrict__ feat_cnt,
                                                     const int32_t* __restrict__ idx, const int32_t* __restrict__ idx_cnt,
                                                     int b, int n_rows, int m_rows, int C, int nsample,
                                                     float* __restrict__ out) {
  __shared__ int32_t s_n[kMaxFrames + 1], s_m[kMaxFrames + 1];
  frame_starts(feat_cnt, b, n_rows, s_n);
  frame_starts(idx_cnt, b, m_rows, s_m);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_row = (int64_t)C * nsample;
  if (e >= (int64_t)m_rows * per_row) return;
  const int m = (int)(e / per_row), c = (int)((e % per_row) / nsample), s = (int)(e % nsample);
  float v = 0.f;
  if (m < s_m[b]) {
    const int f = frame_of(m, s_m, b);
    const int32_t k = idx[(size_t)m * nsample + s];
    if (k >= 0 && k < s_n[f + 1] - s_n[f]) v = feat[((size_t)s_n[f] + k) * C + c];
  }
  out[e] = v;
}

// out[n][c] = ((w0*f0) + (w1*f1)) + (w2*f2), f_i = features[idx[n][i]][c] (global rows; outside [0, m_rows) reads as 0);
// with cnt given, the rows past the sum of the counts are dead: 0.
__global__ __launch_bounds__(256) void k_stack_interp(const float* __restrict__ feat, const int32_t* __restrict__ idx,
                                                      const float* __restrict__ w, const int32_t* __restrict__ cnt, int b,
                                                      int m_rows, int n_rows, int C, float* __restrict__ out) {
  __shared__ int32_t s_n[kMaxFrames + 1];
  int live = n_rows;
  if (cnt) {
    frame_starts(cnt, b, n_rows, s_n);
    live = s_n[b];
  }
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_rows * C) return;
  const int n = (int)(e / C), c = (int)(e % C);
  float r = 0.f;
  if (n < live) {
    float acc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int32_t k = idx[(size_t)n * 3 + i];
      acc[i] = w[(size_t)n * 3 + i] * ((k >= 0 && k < m_rows) ? feat[(size_t)k * C + c] : 0.f);
    }
    r = (acc[0] + acc[1]) + acc[2];
  }
  out[e] = r;
}

// ---------------------------------------------------------------------------------------------- deterministic backward
// Sorted runs (sorted_runs.h) with key = global target row.  The sorted array is cut into chunks of kRunChunk
// positions; one thread per (chunk, channel) adds each run's piece inside its chunk in order.  A run that lies
// inside one chunk is finished there.  A run that crosses chunk borders leaves one partial per chunk (at most one run
// enters a chunk from the left and one leaves it to the right), and a second pass adds a target's partials in chunk
// order: a heavy target costs ceil(len / kRunChunk) additions there instead of len, and the order stays fixed.
__global__ __launch_bounds__(256) void k_group_keys(const int32_t* __restrict__ idx, const int32_t* __restrict__ feat_cnt,
                                                    const int32_t* __restrict__ idx_cnt, int b, int n_rows, int m_rows,
                                                    int nsample, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ int32_t s_n[kMaxFrames + 1], s_m[kMaxFrames + 1];
  frame_starts(feat_cnt, b, n_rows, s_n);
  frame_starts(idx_cnt, b, m_rows, s_m);
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)m_rows * nsample) return;
  const int m = (int)(e / nsample);
  uint32_t key = (uint32_t)n_rows;
  if (m < s_m[b]) {
    const int f = frame_of(m, s_m, b);
    const int32_t k = idx[e];
    if (k >= 0 && k < s_n[f + 1] - s_n[f]) key = (uint32_t)(s_n[f] + k);
  }
  keys[e] = key;
  vals[e] = (uint32_t)e;
}

__global__ __launch_bounds__(256) void k_interp_keys(const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int b,
                                                     int m_rows, int n_rows, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ vals) {
  __shared__ int32_t s_n[kMaxFrames + 1];
  int live = n_rows;
  if (cnt) {
    frame_starts(cnt, b, n_rows, s_n);
    live = s_n[b];
  }
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n_rows * 3) return;
  const int32_t k = idx[e];
  keys[e] = (e / 3 < live && k >= 0 && k < m_rows) ? (uint32_t)k : (uint32_t)m_rows;
  vals[e] = (uint32_t)e;
}

// WEIGHTED: entry = row * 3 + neighbour, contribution g[row][c] * w[entry]; else entry = row * nsample + slot,
// contribution g[row][c][slot].
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void k_chunk_sums(const float* __restrict__ g, const float* __restrict__ w,
                                                    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    int64_t total, uint32_t sentinel, int C, int nsample,
                                                    float* __restrict__ part_l, float* __restrict__ part_r,
                                                    float* __restrict__ grad) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t j = t / C, p0 = j * kRunChunk;
  const int c = (int)(t % C);
  if (p0 >= total) return;
  const int64_t p1 = min(p0 + (int64_t)kRunChunk, total);
  uint32_t cur = keys[p0];
  bool left = p0 > 0 && keys[p0 - 1] == cur;
  int64_t p = p0;
  while (cur != sentinel) {
    float acc = 0.f;
    while (p < p1 && keys[p] == cur) {
      const uint32_t ent = vals[p];
      if (WEIGHTED) acc += g[(size_t)(ent / 3) * C + c] * w[ent];
      else acc += g[((size_t)(ent / nsample) * C + c) * nsample + ent % nsample];
      ++p;
    }
    const bool right = p == p1 && p1 < total && keys[p1] == cur;
    if (left) part_l[(size_t)j * C + c] = acc;
    else if (right) part_r[(size_t)j * C + c] = acc;
    else grad[(size_t)cur * C + c] = acc;
    if (p >= p1) break;
    cur = keys[p];
    left = false;
  }
}

__global__ __launch_bounds__(256) void k_run_finish(const int32_t* __restrict__ start, const int32_t* __restrict__ end,
                                                    const float* __restrict__ part_l, const float* __restrict__ part_r,
                                                    int64_t targets, int C, float* __restrict__ grad) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= targets * C) return;
  const int64_t k = t / C;
  const int c = (int)(t % C);
  const int32_t s = start[k], e = end[k];
  if (s == e) {
    grad[t] = 0.f;
    return;
  }
  const int j0 = s / kRunChunk, j1 = (e - 1) / kRunChunk;
  if (j0 == j1) return;   // finished by k_chunk_sums
  float acc = part_r[(size_t)j0 * C + c];
  for (int j = j0 + 1; j <= j1; ++j) acc += part_l[(size_t)j * C + c];
  grad[t] = acc;
}

struct ScatterWs : SortedRunsWs {
  float *part_l, *part_r;   // one partial per (chunk, channel) for the run that enters / leaves the chunk
};

int64_t run_chunks(int64_t total) { return (total + kRunChunk - 1) / kRunChunk; }

// the sorted-runs block (no sort temp when total == 0), then part_l | part_r
size_t scatter_ws_layout(int64_t total, int64_t targets, int c, char* base, ScatterWs* ws) {
  const size_t sr = spx_sorted_runs_layout(total, targets, base, ws, false);
  const size_t pp = spx_align((size_t)run_chunks(total) * (size_t)c * 4);
  if (ws) {
    ws->part_l = (float*)(base + sr);
    ws->part_r = (float*)(base + sr + pp);
  }
  return sr + 2 * pp;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// keys_in / vals_in are filled by the caller's key kernel; grad [targets, c] is written in full.
int scatter_sorted(const float* g, const float* w, const ScatterWs& L, int64_t total, int64_t targets, int c, int nsample,
                   float* grad, hipStream_t s) {
  const uint32_t sentinel = (uint32_t)targets;
  if (const int e = spx_sorted_runs(L, total, targets, s); e != SPX_OK) return e;
  if (total > 0) {
    const int64_t threads = run_chunks(total) * c;
    if (w)
      hipLaunchKernelGGL((k_chunk_sums<true>), dim3(blocks_of(threads)), dim3(256), 0, s, g, w, L.keys_out, L.vals_out, total,
                         sentinel, c, nsample, L.part_l, L.part_r, grad);
    else
      hipLaunchKernelGGL((k_chunk_sums<false>), dim3(blocks_of(threads)), dim3(256), 0, s, g, w, L.keys_out, L.vals_out,
                         total, sentinel, c, nsample, L.part_l, L.part_r, grad);
  }
  hipLaunchKernelGGL(k_run_finish, dim3(blocks_of(targets * c)), dim3(256), 0, s, L.start, L.end, L.part_l, L.part_r, targets,
                     c, grad);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

// ---------------------------------------------------------------------------------------------- stack FPS
constexpr int kFpsThreads = 1024;
constexpr int kFpsRegPoints = 16;   // register-resident: up to 16 points per thread, frames of up to 16384 points

// One workgroup of 1024 threads per frame; thread t owns k = t + j * 1024, the reference's own layout, so a strict `>`
// keeps each thread's best-priority maximum.  A frame of up to 1024 * PPT points keeps points and temp in registers; a
// larger one (only possible when n_rows is larger, and then temp_ws is given) keeps temp in the workspace.
// The rounds of one frame.  PPT > 0: points and temp in registers; PPT == 0: temp in T, points streamed every round.
template <int PPT>
__device__ __forceinline__ void fps_rounds(const float* __restrict__ P, float* __restrict__ T, int N, int M, int start,
                                           int32_t* __restrict__ out, uint64_t (*s_key)[kFpsThreads / SPX_WAVE],
                                           float4 (*s_pt)[kFpsThreads / SPX_WAVE]) {
  constexpr int R = PPT > 0 ? PPT : 1;
  constexpr int bs = kFpsThreads, nw = kFpsThreads / SPX_WAVE;
  const int t = threadIdx.x;
  const uint32_t hi = (__brev((uint32_t)t) >> 22) << 22;
  const int lane = t & (SPX_WAVE - 1), wv = t / SPX_WAVE;

  float px[R], py[R], pz[R], pt[R];
  if (PPT > 0) {   // slots past N get temp = -inf: they never win and need no branch in the round loop
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int k = t + j * bs;
      const bool in = k < N;
      pt[j] = in ? 1e10f : -INFINITY;
      px[j] = in ? P[3 * k] : 0.f;
      py[j] = in ? P[3 * k + 1] : 0.f;
      pz[j] = in ? P[3 * k + 2] : 0.f;
    }
  } else {
    for (int k = t; k < N; k += bs) T[k] = 1e10f;
  }

  int old = 0;
  float ox = 0.f, oy = 0.f, oz = 0.f;
  if (N > 0) {
    ox = P[0];
    oy = P[1];
    oz = P[2];
  }
  const float x0 = ox, y0 = oy, z0 = oz;
  if (t == 0) out[0] = start;
  for (int r = 1; r < M; ++r) {
    float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    int bj = 0;
    if (PPT > 0) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float d = fminf(sq_dist(px[j], py[j], pz[j], ox, oy, oz), pt[j]);
        pt[j] = d;
        if (d > best) {
          best = d;
          bj = j;
          bx = px[j];
          by = py[j];
          bz = pz[j];
        }
      }
    } else {
      for (int j = 0, k = t; k < N; ++j, k += bs) {
        const float x = P[3 * k], y = P[3 * k + 1], z = P[3 * k + 2];
        const float d = fminf(sq_dist(x, y, z, ox, oy, oz), T[k]);
        T[k] = d;
        if (d > best) {
          best = d;
          bj = j;
          bx = x;
          by = y;
          bz = z;
        }
      }
    }
    const uint64_t mine = best > -1.f ? ((uint64_t)ord_f32(best) << 32) | (uint32_t)~(hi | (uint32_t)bj) : 0ull;
    uint64_t wk = mine;
    for (int off = 1; off < SPX_WAVE; off <<= 1) {
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
#pragma unroll 1
    for (int i = 0; i < nw; ++i) {
      const uint64_t kk = s_key[buf][i];
      if (kk > gk) {
        gk = kk;
        gw = i;
      }
    }
    if (gk == 0ull) {   // no candidate (an empty frame): the reference's besti = 0
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
    if (t == 0) out[r] = start + old;
  }
}

template <int PPT>
__global__ __launch_bounds__(kFpsThreads) void k_stack_fps(const float* __restrict__ xyz, const int32_t* __restrict__ cnt,
                                                           const int32_t* __restrict__ npoint, int b, int n_rows,
                                                           int out_rows, float* __restrict__ temp_ws,
                                                           int32_t* __restrict__ idx) {
  __shared__ int32_t s_n[kMaxFrames + 1], s_o[kMaxFrames + 1];
  __shared__ uint64_t s_key[2][kFpsThreads / SPX_WAVE];
  __shared__ float4 s_pt[2][kFpsThreads / SPX_WAVE];   // winner of each wave: x, y, z, k
  frame_starts(cnt, b, n_rows, s_n);
  frame_starts(npoint, b, out_rows, s_o);
  const int f = blockIdx.x;
  const int start = s_n[f], N = s_n[f + 1] - start, M = s_o[f + 1] - s_o[f];
  if (M <= 0) return;
  const float* P = xyz + (size_t)start * 3;
  int32_t* out = idx + s_o[f];
  if (N <= kFpsThreads * PPT) fps_rounds<PPT>(P, nullptr, N, M, start, out, s_key, s_pt);   // uniform over the workgroup
  else fps_rounds<0>(P, temp_ws + start, N, M, start, out, s_key, s_pt);
}

template <int PPT>
void launch_stack_fps(const float* xyz, const int32_t* cnt, const int32_t* npoint, int b, int n_rows, int out_rows,
                      float* temp, int32_t* idx, hipStream_t s) {
  hipLaunchKernelGGL((k_stack_fps<PPT>), dim3(b), dim3(kFpsThreads), 0, s, xyz, cnt, npoint, b, n_rows, out_rows, temp, idx);
}

bool fps_in_registers(int64_t n) { return n <= (int64_t)kFpsThreads * kFpsRegPoints; }

bool rows_ok(int64_t r) { return r < (int64_t)INT32_MAX / 4; }

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int spx_stack_ball_query(const float* xyz, const int32_t* xyz_batch_cnt, const float* new_xyz,
                                    const int32_t* new_xyz_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows,
                                    float radius, int32_t nsample, int32_t* idx, uint8_t* empty, spx_stream_t stream) {
  if (b <= 0 || n_rows < 0 || m_rows < 0 || nsample <= 0 || !(radius >= 0.f)) return SPX_ERR_INVALID_ARG;
  if (b > kMaxFrames) return SPX_ERR_UNSUPPORTED;
  if (!xyz_batch_cnt || !new_xyz_batch_cnt || !new_xyz || !idx || !empty || (n_rows > 0 && !xyz)) return SPX_ERR_INVALID_ARG;
  if (m_rows == 0) return SPX_OK;
  if (!rows_ok(n_rows) || !rows_ok(m_rows) || m_rows * (int64_t)nsample >= ((int64_t)1 << 40)) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_stack_ball_query, dim3((unsigned)((m_rows + kTile - 1) / kTile + b)), dim3(kTile), 0, spx_s(stream),
                     xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, b, (int)n_rows, (int)m_rows, nsample, radius * radius,
                     idx, empty);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_stack_group_points(const float* features, const int32_t* features_batch_cnt, const int32_t* idx,
                                      const int32_t* idx_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows, int32_t c,
                                      int32_t nsample, float* out, spx_stream_t stream) {
  if (b <= 0 || n_rows < 0 || m_rows < 0 || c < 0 || nsample <= 0) return SPX_ERR_INVALID_ARG;
  if (b > kMaxFrames) return SPX_ERR_UNSUPPORTED;
  if ((n_rows > 0 && !features) || !features_batch_cnt || !idx || !idx_batch_cnt || !out) return SPX_ERR_INVALID_ARG;
  if (m_rows == 0 || c == 0) return SPX_OK;
  const int64_t total = m_rows * c * (int64_t)nsample;
  if (!rows_ok(n_rows) || !rows_ok(m_rows) || total >= ((int64_t)1 << 39)) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_stack_group, dim3(blocks_of(total)), dim3(256), 0, spx_s(stream), features, features_batch_cnt, idx,
                     idx_batch_cnt, b, (int)n_rows, (int)m_rows, c, nsample, out);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_stack_group_points_bwd_ws_bytes(int64_t n_rows, int64_t m_rows, int32_t c, int32_t nsample) {
  if (n_rows <= 0 || m_rows < 0 || c <= 0 || nsample <= 0 || m_rows * (int64_t)nsample >= (int64_t)INT32_MAX) return 0;
  return scatter_ws_layout(m_rows * nsample, n_rows, c, nullptr, nullptr);
}

extern "C" int spx_stack_group_points_bwd(const float* grad_out, const int32_t* features_batch_cnt, const int32_t* idx,
                                          const int32_t* idx_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows,
                                          int32_t c, int32_t nsample, float* grad_features, void* ws, size_t ws_bytes,
                                          spx_stream_t stream) {
  if (b <= 0 || n_rows < 0 || m_rows < 0 || c < 0 || nsample <= 0) return SPX_ERR_INVALID_ARG;
  if (b > kMaxFrames) return SPX_ERR_UNSUPPORTED;
  if ((m_rows > 0 && (!grad_out || !idx)) || !features_batch_cnt || !idx_batch_cnt || !grad_features) return SPX_ERR_INVALID_ARG;
  if (n_rows == 0 || c == 0) return SPX_OK;
  const int64_t total = m_rows * nsample;
  if (!rows_ok(n_rows) || !rows_ok(m_rows) || total >= (int64_t)INT32_MAX || n_rows * c >= ((int64_t)1 << 39))
    return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < scatter_ws_layout(total, n_rows, c, nullptr, nullptr)) return SPX_ERR_WORKSPACE;
  ScatterWs L;
  scatter_ws_layout(total, n_rows, c, (char*)ws, &L);
  hipStream_t s = spx_s(stream);
  if (total > 0)
    hipLaunchKernelGGL(k_group_keys, dim3(blocks_of(total)), dim3(256), 0, s, idx, features_batch_cnt, idx_batch_cnt, b,
                       (int)n_rows, (int)m_rows, nsample, L.keys_in, L.vals_in);
  return scatter_sorted(grad_out, nullptr, L, total, n_rows, c, nsample, grad_features, s);
}

extern "C" int spx_stack_three_nn(const float* unknown, const int32_t* unknown_batch_cnt, const float* known,
                                  const int32_t* known_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows, float* dist2,
                                  int32_t* idx, spx_stream_t stream) {
  if (b <= 0 || n_rows < 0 || m_rows < 0) return SPX_ERR_INVALID_ARG;
  if (b > kMaxFrames) return SPX_ERR_UNSUPPORTED;
  if (!unknown || !unknown_batch_cnt || (m_rows > 0 && !known) || !known_batch_cnt || !dist2 || !idx) return SPX_ERR_INVALID_ARG;
  if (n_rows == 0) return SPX_OK;
  if (!rows_ok(n_rows) || !rows_ok(m_rows)) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_stack_three_nn, dim3((unsigned)((n_rows + kTile - 1) / kTile + b)), dim3(kTile), 0, spx_s(stream),
                     unknown, unknown_batch_cnt, known, known_batch_cnt, b, (int)n_rows, (int)m_rows, dist2, idx);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_stack_three_interpolate(const float* features, const int32_t* idx, const float* weight,
                                           const int32_t* batch_cnt, int32_t b, int64_t m_rows, int64_t n_rows, int32_t c,
                                           float* out, spx_stream_t stream) {
  if (b < 0 || m_rows < 0 || n_rows < 0 || c < 0 || (batch_cnt && b == 0)) return SPX_ERR_INVALID_ARG;
  if (b > kMaxFrames) return SPX_ERR_UNSUPPORTED;
  if ((m_rows > 0 && !features) || !idx || !weight || !out) return SPX_ERR_INVALID_ARG;
  if (n_rows == 0 || c == 0) return SPX_OK;
  if (!rows_ok(n_rows) || !rows_ok(m_rows) || n_rows * c >= ((int64_t)1 << 39)) return SPX_ERR_TOO_LARGE;
  hipLaunchKernelGGL(k_stack_interp, dim3(blocks_of(n_rows * c)), dim3(256), 0, spx_s(stream), features, idx, weight,
                     batch_cnt, b, (int)m_rows, (int)n_rows, c, out);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_stack_three_interpolate_bwd_ws_bytes(int64_t m_rows, int64_t n_rows, int32_t c) {
  if (m_rows <= 0 || n_rows < 0 || c <= 0 || n_rows * 3 >= (int64_t)INT32_MAX) return 0;
  return scatter_ws_layout(n_rows * 3, m_rows, c, nullptr, nullptr);
}

extern "C" int spx_stack_three_interpolate_bwd(const float* grad_out, const int32_t* idx, const float* weight,
                                               const int32_t* batch_cnt, int32_t b, int64_t m_rows, int64_t n_rows,
                                               int32_t c, float* grad_features, void* ws, size_t ws_bytes,
                                               spx_stream_t stream) {
  if (b < 0 || m_rows < 0 || n_rows < 0 || c < 0 || (batch_cnt && b == 0)) return SPX_ERR_INVALID_ARG;
  if (b > kMaxFrames) return SPX_ERR_UNSUPPORTED;
  if ((n_rows > 0 && (!grad_out || !idx || !weight)) || !grad_features) return SPX_ERR_INVALID_ARG;
  if (m_rows == 0 || c == 0) return SPX_OK;
  const int64_t total = n_rows * 3;
  if (!rows_ok(n_rows) || !rows_ok(m_rows) || m_rows * c >= ((int64_t)1 << 39)) return SPX_ERR_TOO_LARGE;
  if (!ws || ws_bytes < scatter_ws_layout(total, m_rows, c, nullptr, nullptr)) return SPX_ERR_WORKSPACE;
  ScatterWs L;
  scatter_ws_layout(total, m_rows, c, (char*)ws, &L);
  hipStream_t s = spx_s(stream);
  if (total > 0)
    hipLaunchKernelGGL(k_interp_keys, dim3(blocks_of(total)), dim3(256), 0, s, idx, batch_cnt, b, (int)m_rows, (int)n_rows,
                       L.keys_in, L.vals_in);
  return scatter_sorted(grad_out, weight, L, total, m_rows, c, 3, grad_features, s);
}

extern "C" size_t spx_stack_furthest_point_sample_ws_bytes(int64_t n_rows) {
  return (n_rows <= 0 || fps_in_registers(n_rows)) ? 0 : spx_align((size_t)n_rows * 4);   // a frame may exceed 16384
}

extern "C" int spx_stack_furthest_point_sample(const float* xyz, const int32_t* xyz_batch_cnt, const int32_t* npoint,
                                               int32_t b, int64_t n_rows, int64_t out_rows, int32_t* idx, void* ws,
                                               size_t ws_bytes, spx_stream_t stream) {
  if (b <= 0 || n_rows < 0 || out_rows < 0) return SPX_ERR_INVALID_ARG;
  if (b > kMaxFrames) return SPX_ERR_UNSUPPORTED;
  if ((n_rows > 0 && !xyz) || !xyz_batch_cnt || !npoint || !idx) return SPX_ERR_INVALID_ARG;
  if (out_rows == 0) return SPX_OK;
  if (!rows_ok(n_rows) || !rows_ok(out_rows)) return SPX_ERR_TOO_LARGE;
  hipStream_t s = spx_s(stream);
  const int nr = (int)n_rows, orows = (int)out_rows;
  float* temp = nullptr;
  if (!fps_in_registers(n_rows)) {
    if (!ws || ws_bytes < spx_stack_furthest_point_sample_ws_bytes(n_rows)) return SPX_ERR_WORKSPACE;
    temp = (float*)ws;
  }
  const int per = (int)((std::min<int64_t>(n_rows, (int64_t)kFpsThreads * kFpsRegPoints) + kFpsThreads - 1) / kFpsThreads);
  if (per <= 1) launch_stack_fps<1>(xyz, xyz_batch_cnt, npoint, b, nr, orows, temp, idx, s);
  else if (per <= 2) launch_stack_fps<2>(xyz, xyz_batch_cnt, npoint, b, nr, orows, temp, idx, s);
  else if (per <= 4) launch_stack_fps<4>(xyz, xyz_batch_cnt, npoint, b, nr, orows, temp, idx, s);
  else if (per <= 8) launch_stack_fps<8>(xyz, xyz_batch_cnt, npoint, b, nr, orows, temp, idx, s);
  else launch_stack_fps<16>(xyz, xyz_batch_cnt, npoint, b, nr, orows, temp, idx, s);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
