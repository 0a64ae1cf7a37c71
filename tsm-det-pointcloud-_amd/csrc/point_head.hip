// point_head.hip — the eval tail of the fork's fast_cpc point head (include/spx.h §14).  The reference
// (pcdet/models/dense_heads/point_head_vote_sasa_statistic_distillation.py, student branch) runs, per frame batch:
//
//   vote:     offset = Conv1d(128->128) -> BN -> ReLU -> Conv1d(128->3) over the candidate columns [lo, hi),
//             vote = cand + min(max(offset, -range), range);
//   predict:  for each class k: logit_k = Conv1d(64->1)(ReLU(BN(Conv1d(256->64)(x * stat_k)))),
//             reg = Conv1d(128->30)(ReLU(BN(Conv1d(256->128)(x)))), box = decode(reg, vote) (PointBinResidualCoder,
//             use_mean_size False);
//
// as ~48 small launches plus permutes.  Here each is one launch.  A workgroup owns a tile of kTile points: the input
// tile [c][kTile] and the hidden activations [h][kTile] stay in LDS, so both layers (and the decode) run without a
// round trip through memory.  The GEMMs are on the VALU: per point the whole tail is ~82 K MACs, the problem is a few
// thousand points, and the weights (≤ 128 KB per MLP) come from L2 in 16-channel chunks staged through LDS.
//   hidden layer: wave w owns points [8w, 8w + 8) of the tile, lane j owns hidden units j and j + 64; the point values
//                 are LDS broadcasts, the weights a conflict-free LDS row.  BatchNorm is applied as its eval affine
//                 (x - mean) / sqrt(var + eps) * gamma + beta from the module's own tensors.
//   out layer:    one thread per (output, point); the weight row is a uniform (cached) load.
// The per-class statistic multiplies the staged weight chunk (W[j, c] * stat[c]) rather than the input tile.
// Parameters arrive as a struct of device pointers passed by value: nothing is folded or cached on the host, so the
// kernels always read the module's current tensors (load_state_dict needs no invalidation) and both ops capture.
#include "spx_common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                       // points per workgroup
constexpr int kWaves = kThreads / SPX_WAVE;     // 4
constexpr int kPPW = kTile / kWaves;            // points per wave: 8
constexpr int kMaxC = 256;                      // input channels
constexpr int kMaxH = 128;                      // hidden units (two per lane)
constexpr int kMaxClass = 8;
constexpr int kMaxBins = 32;
constexpr int kMaxOut = 6 + 2 * kMaxBins;       // 70
constexpr int kKc = 16;                         // weight chunk (input channels) staged per round
constexpr int kPitch = kMaxH + 1;               // padded LDS row of the staged chunk
constexpr int kScratch = (kKc * kPitch > kMaxOut * kTile) ? kKc * kPitch : kMaxOut * kTile;

static_assert(kTile % kWaves == 0 && kPPW == 8, "the hidden layer holds 8 points per lane");
static_assert(kMaxH == 2 * SPX_WAVE, "two hidden units per lane");

struct Tile {
  float xs[kMaxC * kTile];        // input tile [c][p]
  float hs[kMaxH * kTile];        // hidden activations [j][p]
  float scr[kScratch];            // staged weight chunk [kk][j], then the out layer's [o][p]
  float cls[kMaxClass * kTile];   // class logits [k][p]
};

struct VoteArgs {
  spx_point_mlp mlp;
  const float* feat;   // [b, c, n]
  const float* xyz;    // [b, n, 3]
  float* vote;         // [b, nv, 3]
  int64_t n, lo, nv, total;
  int c, h;
  float range[3];
};

struct PredictArgs {
  spx_point_mlp cls[kMaxClass];
  spx_point_mlp reg;
  const float* feat;   // [b, c, n]
  const float* stat;   // [num_class, c]
  const float* vxyz;   // [b * n, 3]
  float* cls_out;      // [b * n, num_class]
  float* reg_out;      // [b * n, 6 + 2 * bins]
  float* box_out;      // [b * n, 7]
  int64_t n, total;
  int c, nc, hc, hr, bins;
  float angle_step;    // (float)(2 pi / bins)
};

// hs[j][p] = ReLU(BN(sum_c W1[j, c] * (stat ? stat[c] : 1) * xs[c][p])), j < h.  Ends with a barrier.
__device__ __forceinline__ void hidden_layer(const float* __restrict__ xs, int c, const spx_point_mlp& m, int h,
                                             const float* __restrict__ stat, float* __restrict__ ws,
                                             float* __restrict__ hs) {
  const int lane = threadIdx.x & (SPX_WAVE - 1);
  const int wave = threadIdx.x / SPX_WAVE;
  const bool two = h > SPX_WAVE;
  float a0[kPPW], a1[kPPW];
#pragma unroll
  for (int p = 0; p < kPPW; ++p) a0[p] = a1[p] = 0.f;
  for (int kc = 0; kc < c; kc += kKc) {
    __syncthreads();  // the previous chunk (or out layer) is done with ws
    for (int q = threadIdx.x; q < h * kKc; q += kThreads) {
      const int j = q / kKc, kk = q - j * kKc, ch = kc + kk;
      float w = 0.f;
      if (ch < c) {
        w = m.w1[(size_t)j * c + ch];
        if (stat) w *= stat[ch];
      }
      ws[kk * kPitch + j] = w;
    }
    __syncthreads();
    const int kn = min(kKc, c - kc);
    for (int kk = 0; kk < kn; ++kk) {
      const float4* xr = reinterpret_cast<const float4*>(xs + (kc + kk) * kTile + wave * kPPW);
      const float4 xa = xr[0], xb = xr[1];
      const float x[kPPW] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
      const float w0 = ws[kk * kPitch + lane];
#pragma unroll
      for (int p = 0; p < kPPW; ++p) a0[p] = fmaf(w0, x[p], a0[p]);
      if (two) {
        const float w1 = ws[kk * kPitch + lane + SPX_WAVE];
#pragma unroll
        for (int p = 0; p < kPPW; ++p) a1[p] = fmaf(w1, x[p], a1[p]);
      }
    }
  }
  for (int half = 0; half < 2; ++half) {
    const int j = lane + half * SPX_WAVE;
    if (j >= h) break;
    const float inv = 1.0f / sqrtf(m.bn_var[j] + m.bn_eps);
    const float mu = m.bn_mean[j], g = m.bn_weight[j], be = m.bn_bias[j];
#pragma unroll
    for (int p = 0; p < kPPW; ++p) {
      const float v = ((half ? a1[p] : a0[p]) - mu) * inv * g + be;
      hs[j * kTile + wave * kPPW + p] = v > 0.f ? v : 0.f;
    }
  }
  __syncthreads();
}

// out[o][p] = sum_j W2[o, j] * hs[j][p] + b2[o], o < n_out.  Ends with a barrier.
__device__ __forceinline__ void out_layer(const float* __restrict__ hs, int h, const spx_point_mlp& m, int n_out,
                                          float* __restrict__ out) {
  for (int q = threadIdx.x; q < n_out * kTile; q += kThreads) {
    const int o = q / kTile, p = q - o * kTile;
    const float* w = m.w2 + (size_t)o * h;
    float s = 0.f;
    for (int j = 0; j < h; ++j) s = fmaf(w[j], hs[j * kTile + p], s);
    out[o * kTile + p] = s + m.b2[o];
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_point_vote(VoteArgs a) {
  __shared__ __attribute__((aligned(16))) Tile t;
  const int64_t m0 = (int64_t)blockIdx.x * kTile;
  for (int q = threadIdx.x; q < a.c * kTile; q += kThreads) {
    const int ch = q / kTile, p = q - ch * kTile;
    const int64_t m = m0 + p;
    float v = 0.f;
    if (m < a.total) {
      const int64_t bi = m / a.nv, i = a.lo + (m - bi * a.nv);
      v = a.feat[((size_t)bi * a.c + ch) * a.n + i];
    }
    t.xs[q] = v;
  }
  __syncthreads();
  hidden_layer(t.xs, a.c, a.mlp, a.h, nullptr, t.scr, t.hs);
  out_layer(t.hs, a.h, a.mlp, 3, t.scr);
  for (int q = threadIdx.x; q < 3 * kTile; q += kThreads) {
    const int p = q / 3, o = q - p * 3;
    const int64_t m = m0 + p;
    if (m >= a.total) continue;
    const int64_t bi = m / a.nv, i = a.lo + (m - bi * a.nv);
    const float r = a.range[o];
    float off = t.scr[o * kTile + p];
    if (!isnan(off)) off = fminf(fmaxf(off, -r), r);  // torch.max / torch.min propagate NaN
    a.vote[m * 3 + o] = a.xyz[((size_t)bi * a.n + i) * 3 + o] + off;
  }
}

__global__ __launch_bounds__(kThreads) void k_point_head_predict(PredictArgs a) {
  __shared__ __attribute__((aligned(16))) Tile t;
  const int64_t m0 = (int64_t)blockIdx.x * kTile;
  for (int q = threadIdx.x; q < a.c * kTile; q += kThreads) {
    const int ch = q / kTile, p = q - ch * kTile;
    const int64_t m = m0 + p;
    float v = 0.f;
    if (m < a.total) {
      const int64_t bi = m / a.n, i = m - bi * a.n;
      v = a.feat[((size_t)bi * a.c + ch) * a.n + i];
    }
    t.xs[q] = v;
  }
  __syncthreads();
  for (int k = 0; k < a.nc; ++k) {
    hidden_layer(t.xs, a.c, a.cls[k], a.hc, a.stat + (size_t)k * a.c, t.scr, t.hs);
    out_layer(t.hs, a.hc, a.cls[k], 1, t.cls + k * kTile);
  }
  const int r_out = 6 + 2 * a.bins;
  hidden_layer(t.xs, a.c, a.reg, a.hr, nullptr, t.scr, t.hs);
  out_layer(t.hs, a.hr, a.reg, r_out, t.scr);
  for (int q = threadIdx.x; q < a.nc * kTile; q += kThreads) {
    const int p = q / a.nc, k = q - p * a.nc;
    const int64_t m = m0 + p;
    if (m < a.total) a.cls_out[m * a.nc + k] = t.cls[k * kTile + p];
  }
  for (int q = threadIdx.x; q < r_out * kTile; q += kThreads) {
    const int p = q / r_out, o = q - p * r_out;
    const int64_t m = m0 + p;
    if (m < a.total) a.reg_out[m * r_out + o] = t.scr[o * kTile + p];
  }
  if (threadIdx.x < kTile) {
    const int p = threadIdx.x;
    const int64_t m = m0 + p;
    if (m < a.total) {
      const float* r = t.scr + p;  // r[o * kTile] = reg[o]
      float* box = a.box_out + m * 7;
      box[0] = r[0 * kTile] + a.vxyz[m * 3 + 0];
      box[1] = r[1 * kTile] + a.vxyz[m * 3 + 1];
      box[2] = r[2 * kTile] + a.vxyz[m * 3 + 2];
      box[3] = expf(r[3 * kTile]);
      box[4] = expf(r[4 * kTile]);
      box[5] = expf(r[5 * kTile]);
      // first maximum, NaN above everything (torch.argmax)
      int bin = 0;
      float best = r[6 * kTile];
      for (int j = 1; j < a.bins; ++j) {
        const float v = r[(6 + j) * kTile];
        if (!isnan(best) && (v > best || isnan(v))) {
          best = v;
          bin = j;
        }
      }
      box[6] = ((float)bin + r[(6 + a.bins + bin) * kTile]) * a.angle_step;
    }
  }
}

bool mlp_ok(const spx_point_mlp& m) {
  return m.w1 && m.bn_mean && m.bn_var && m.bn_weight && m.bn_bias && m.w2 && m.b2;
}

int64_t n_tiles(int64_t total) { return (total + kTile - 1) / kTile; }

}  // namespace

extern "C" int spx_point_vote(const float* feat, const float* xyz, int32_t b, int32_t c_in, int64_t n, int64_t lo,
                              int64_t hi, const spx_point_mlp* mlp, int32_t hidden, const float* range, float* vote,
                              spx_stream_t stream) {
  if (b < 0 || n < 0 || lo < 0 || hi < lo || hi > n || !mlp || !range) return SPX_ERR_INVALID_ARG;
  if (c_in < 1 || c_in > kMaxC || hidden < 1 || hidden > kMaxH) return SPX_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)b * (hi - lo);
  if (total == 0) return SPX_OK;
  if (!feat || !xyz || !vote || !mlp_ok(*mlp)) return SPX_ERR_INVALID_ARG;
  if (n_tiles(total) > INT32_MAX) return SPX_ERR_TOO_LARGE;
  VoteArgs a;
  a.mlp = *mlp;
  a.feat = feat;
  a.xyz = xyz;
  a.vote = vote;
  a.n = n;
  a.lo = lo;
  a.nv = hi - lo;
  a.total = total;
  a.c = c_in;
  a.h = hidden;
  for (int i = 0; i < 3; ++i) a.range[i] = range[i];
  hipLaunchKernelGGL(k_point_vote, dim3((unsigned)n_tiles(total)), dim3(kThreads), 0, spx_s(stream), a);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" int spx_point_head_predict(const float* feat, const float* stat, const float* vote_xyz, int32_t b, int32_t c,
                                      int64_t n, int32_t num_class, const spx_point_mlp* cls, int32_t cls_hidden,
                                      const spx_point_mlp* reg, int32_t reg_hidden, int32_t bins, float* cls_out,
                                      float* reg_out, float* box_out, spx_stream_t stream) {
  if (b < 0 || n < 0 || !cls || !reg) return SPX_ERR_INVALID_ARG;
  if (c < 1 || c > kMaxC || num_class < 1 || num_class > kMaxClass || cls_hidden < 1 || cls_hidden > kMaxH ||
      reg_hidden < 1 || reg_hidden > kMaxH || bins < 1 || bins > kMaxBins)
    return SPX_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)b * n;
  if (total == 0) return SPX_OK;
  if (!feat || !stat || !vote_xyz || !cls_out || !reg_out || !box_out || !mlp_ok(*reg)) return SPX_ERR_INVALID_ARG;
  for (int k = 0; k < num_class; ++k)
    if (!mlp_ok(cls[k])) return SPX_ERR_INVALID_ARG;
  if (n_tiles(total) > INT32_MAX) return SPX_ERR_TOO_LARGE;
  PredictArgs a = {};
  for (int k = 0; k < num_class; ++k) a.cls[k] = cls[k];
  a.reg = *reg;
  a.feat = feat;
  a.stat = stat;
  a.vxyz = vote_xyz;
  a.cls_out = cls_out;
  a.reg_out = reg_out;
  a.box_out = box_out;
  a.n = n;
  a.total = total;
  a.c = c;
  a.nc = num_class;
  a.hc = cls_hidden;
  a.hr = reg_hidden;
  a.bins = bins;
  a.angle_step = (float)(M_PI * 2.0 / (double)bins);
  hipLaunchKernelGGL(k_point_head_predict, dim3((unsigned)n_tiles(total)), dim3(kThreads), 0, spx_s(stream), a);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
