// sa_mlp.hip — the eval-mode tail of a two-layer stacked set-abstraction pointnet, fused (include/spx.h §28).  The torch
// composition groups (M, 3 + C, S) columns, runs Conv2d + BatchNorm2d + ReLU twice over (1, C, M, S) tensors and takes
// the max over the S slots.  With the first conv split into the caller's GEMM over the source rows (P = features Wf^T,
// as spx_group_project takes it) plus its three xyz columns, and both BatchNorms folded into affine maps, the tail is
//
//   h[m, s, c] = relu(a1[c] * (P[r, c] + Wx[c] . (xyz[r] - new_xyz[m])) + b1[c]),   r = idx[m, s]
//   out[m, o]  = max_s relu(a2[o] * (sum_c W2[o, c] * h[m, s, c]) + b2[o])
//
// The xyz term stays relative (group_project.hip says why: absolute coordinates times Wx cancel catastrophically).
//
// Schedule.  One wave owns one query at a time and walks the queries with a grid stride.  A tile of 16 slots is one
// row block of the exact-fp32 v_mfma_f32_16x16x4_f32: D[s, o] += A[s, k] * B[k, o] with A[l & 15][l >> 4],
// B[l >> 4][l & 15], D[4 * (l >> 4) + reg][l & 15].  Lane l gathers the quarter [g * C1 / 4, (g + 1) * C1 / 4),
// g = l >> 4, of the P row of slot l & 15 as float4 loads, applies layer 1 in registers and feeds channel g * C1 / 4 + j
// as the k = g element of MFMA step j (any fixed bijection of channels onto (step, k) is a valid K order as long as A
// and B agree).  W2 sits in registers for the whole kernel, laid out as those B operands: C2 / 16 * C1 / 4 floats per
// lane.  The layer-1 constants sit in LDS; the four lane groups of a wave read four addresses, a broadcast each.  The
// max over the 16 rows of D is taken where the accumulator leaves them: over the 4 registers, then across the four
// 16-lane groups.  S = 32 is two tiles combined by max.  No atomics, no workspace, fixed order: bitwise reproducible.
#include "spx_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SPX_WAVE;
constexpr int kMaxBlocks = 2048;   // 8 blocks of 4 waves per CU; a wave then walks M / 8192 queries on one load of W2

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int C1, int C2>
__global__ __launch_bounds__(kThreads) void k_sa_mlp2_max(
    const float* __restrict__ p, const float* __restrict__ xyz, const float* __restrict__ new_xyz,
    const int32_t* __restrict__ idx, const uint8_t* __restrict__ empty, const float* __restrict__ wx,
    const float* __restrict__ a1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ a2, const float* __restrict__ b2, int64_t n_src, int64_t m_total, int tiles,
    float* __restrict__ out) {
  constexpr int KQ = C1 / 4;    // channels per lane group = MFMA steps per tile
  constexpr int NB = C2 / 16;   // 16-column blocks of the output
  __shared__ float4 s_wa[C1];   // (Wx[c, 0..2], a1[c])
  __shared__ float s_b1[C1];
  const int tid = threadIdx.x;
  if (tid < C1) {
    s_wa[tid] = make_float4(wx[tid * 3 + 0], wx[tid * 3 + 1], wx[tid * 3 + 2], a1[tid]);
    s_b1[tid] = b1[tid];
  }
  __syncthreads();
  const int lane = tid % SPX_WAVE, g = lane >> 4, col = lane & 15;
  const int c0 = g * KQ;
  float bw[NB][KQ], a2v[NB], b2v[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int o = nb * 16 + col;
    a2v[nb] = a2[o];
    b2v[nb] = b2[o];
#pragma unroll
    for (int j = 0; j < KQ; ++j) bw[nb][j] = w2[o * C1 + c0 + j];
  }
  const int s_total = tiles * 16;
  const int64_t wave0 = (int64_t)blockIdx.x * kWaves + tid / SPX_WAVE, nwave = (int64_t)gridDim.x * kWaves;
  for (int64_t m = wave0; m < m_total; m += nwave) {   // wave-uniform: every MFMA runs with all 64 lanes
    const bool e = empty != nullptr && empty[m] != 0;
    const float cx = new_xyz[m * 3 + 0], cy = new_xyz[m * 3 + 1], cz = new_xyz[m * 3 + 2];
    float best[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) best[nb] = -INFINITY;
    for (int t = 0; t < tiles; ++t) {
      int64_t r = -1;
      if (!e) {
        const int32_t ri = idx[m * s_total + t * 16 + col];
        if (ri >= 0 && (int64_t)ri < n_src) r = ri;
      }
      // an empty ball, a dead query and a row outside [0, n_src) are zero columns of the grouped tensor: h = relu(b1)
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (r >= 0) {
        dx = xyz[r * 3 + 0] - cx;
        dy = xyz[r * 3 + 1] - cy;
        dz = xyz[r * 3 + 2] - cz;
      }
      f32x4 acc[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j4 = 0; j4 < KQ / 4; ++j4) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r >= 0 && p != nullptr) q = *reinterpret_cast<const float4*>(p + (size_t)r * C1 + c0 + j4 * 4);
        const float pv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int j = j4 * 4 + jj;
          const float4 wa = s_wa[c0 + j];
          const float pre = pv[jj] + ((wa.x * dx + wa.y * dy) + wa.z * dz);
          const float h = fmaxf(wa.w * pre + s_b1[c0 + j], 0.f);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(h, bw[nb][j], acc[nb], 0, 0, 0);
        }
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) best[nb] = fmaxf(best[nb], fmaxf(a2v[nb] * acc[nb][q] + b2v[nb], 0.f));
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      float v = best[nb];
      v = fmaxf(v, __shfl_xor(v, 16, SPX_WAVE));
      v = fmaxf(v, __shfl_xor(v, 32, SPX_WAVE));
      if (g == 0) out[(size_t)m * C2 + nb * 16 + col] = v;
    }
  }
}

bool chan_ok(int32_t c) { return c == 16 || c == 32 || c == 64; }

template <int C1>
void launch_c1(int32_t c2, dim3 grid, hipStream_t s, const float* p, const float* xyz, const float* new_xyz,
               const int32_t* idx, const uint8_t* empty, const float* wx, const float* a1, const float* b1,
               const float* w2, const float* a2, const float* b2, int64_t n_src, int64_t m, int tiles, float* out) {
  if (c2 == 16)
    hipLaunchKernelGGL((k_sa_mlp2_max<C1, 16>), grid, dim3(kThreads), 0, s, p, xyz, new_xyz, idx, empty, wx, a1, b1, w2, a2,
                       b2, n_src, m, tiles, out);
  else if (c2 == 32)
    hipLaunchKernelGGL((k_sa_mlp2_max<C1, 32>), grid, dim3(kThreads), 0, s, p, xyz, new_xyz, idx, empty, wx, a1, b1, w2, a2,
                       b2, n_src, m, tiles, out);
  else
    hipLaunchKernelGGL((k_sa_mlp2_max<C1, 64>), grid, dim3(kThreads), 0, s, p, xyz, new_xyz, idx, empty, wx, a1, b1, w2, a2,
                       b2, n_src, m, tiles, out);
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int spx_sa_mlp2_max(const float* p, const float* xyz, const float* new_xyz, const int32_t* idx,
                               const uint8_t* empty, const float* wx, const float* a1, const float* b1, const float* w2,
                               const float* a2, const float* b2, int32_t c1, int32_t c2, int64_t n_src, int64_t m,
                               int32_t nsample, float* out, spx_stream_t stream) {
  if (c1 <= 0 || c2 <= 0 || nsample <= 0 || n_src < 0 || m < 0) return SPX_ERR_INVALID_ARG;
  if (!chan_ok(c1) || !chan_ok(c2) || (nsample != 16 && nsample != 32)) return SPX_ERR_UNSUPPORTED;
  if (n_src >= (int64_t)INT32_MAX || m * nsample >= (int64_t)INT32_MAX || m * c2 >= (int64_t)INT32_MAX)
    return SPX_ERR_TOO_LARGE;
  if (m == 0) return SPX_OK;
  if (!new_xyz || !idx || !wx || !a1 || !b1 || !w2 || !a2 || !b2 || !out || (n_src > 0 && !xyz))
    return SPX_ERR_INVALID_ARG;
  if (((uintptr_t)p % 16) != 0) return SPX_ERR_INVALID_ARG;   // rows of P are read as float4
  int64_t nblk = (m + kWaves - 1) / kWaves;
  if (nblk > kMaxBlocks) nblk = kMaxBlocks;
  const dim3 grid((unsigned)nblk);
  hipStream_t s = spx_s(stream);
  const int tiles = nsample / 16;
  if (c1 == 16)
    launch_c1<16>(c2, grid, s, p, xyz, new_xyz, idx, empty, wx, a1, b1, w2, a2, b2, n_src, m, tiles, out);
  else if (c1 == 32)
    launch_c1<32>(c2, grid, s, p, xyz, new_xyz, idx, empty, wx, a1, b1, w2, a2, b2, n_src, m, tiles, out);
  else
    launch_c1<64>(c2, grid, s, p, xyz, new_xyz, idx, empty, wx, a1, b1, w2, a2, b2, n_src, m, tiles, out);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
