// pfn_layer.h — the one last-layer PFN core (13 feature slots -> Linear(C_in, 64, bias=False) -> BatchNorm1d -> ReLU ->
// max over a pillar's points) that pillar_vfe.hip (§23) and dyn_pillar_vfe.hip (§24) share.  The maths lives HERE, once;
// what differs between the two ops (how a pillar's points are stored, how the features and the statistics' partial sums
// are formed, which rows pad) stays in their files.  Workgroups are 256 threads: thread = (q = tid >> 6, ch = tid & 63).
//
// Slots.  Features live in 13 FIXED slots whatever the configuration: 0-2 xyz, 3-5 xyz - pillar mean, 6-8 xyz - pillar
// centre, 9 norm, 10-12 the raw columns past xyz.  A host table (make_cols; each op's Geo carries it as `int col[13]; int
// c_in;`, which is all the templates below ask of a Geo) maps every slot to its weight column (-1: absent, its weight
// reads as 0), so x = w.f is one 13-term fma chain in double (dot13) in every kernel of both ops.
//
// Statistics.  The linear layer is never evaluated for the batch statistics: with S1 = sum f and G = sum f f^T over the
// real points (stats[0, 169) = G, stats[169, 182) = S1) and N the BatchNorm row count, per channel
//   mean = w.S1 / N,   E[x^2] = w^T G w / N,   var = max(E[x^2] - mean^2, 0) (biased),   invstd = 1 / sqrt(var + eps),
//   scale = gamma invstd,   shift = beta - mean scale,   z = x scale + shift
// (stats_channel; fold_scale_shift gives the same pair from the running statistics in eval mode).  Rows whose features
// are all zero (padding) add nothing to S1 and G and only count in N.
//
// Weight gradient.  With g the gradient at the selected row of each (pillar, channel) where the output is positive, the
// train-mode BatchNorm gradient of the weight is, per channel,
//   dW = gamma invstd [ A - (d_beta / N) S1 - (d_gamma / N) invstd (G w - mean S1) ],
//   A = sum g f_sel,   d_beta = sum g,   d_gamma = sum g xhat_sel,   xhat = (x - mean) invstd,
// so the dense term needs only S1 and G of the forward; in eval mode dW = gamma invstd A.  Each op's k_bwd_gather takes
// A, d_beta, d_gamma (kAcc doubles per channel, one partial per block, the block's four pillar lanes added in the order
// q = 0, 1, 2, 3); pfn_k_bwd_final adds the partials in a fixed order and applies the formula.
//
// No float atomics, every sum in double in ONE fixed order: what a kernel computes does not depend on which op calls it.
#pragma once
#include "spx_common.h"

namespace {

constexpr int kSlots = 13;
constexpr int kCout = 64;
constexpr int kG = kSlots * kSlots;           // 169
constexpr int kStat = kG + kSlots;            // 182: G then S1
constexpr int kOffMean = kStat;               // stats[]: G, S1, mean[64], invstd[64], N
constexpr int kOffInv = kStat + kCout;
constexpr int kOffN = kStat + 2 * kCout;
constexpr int kStatsLen = kOffN + 2;          // 312 doubles
constexpr int kAcc = kSlots + 2;              // per (block, channel): d_beta, d_gamma, A[13]

struct BN {
  const float *weight, *gamma, *beta;
  float *running_mean, *running_var;
  int64_t* nbt;
  float momentum, eps;
};

template <typename Arg>
struct Bwd {
  const float *out, *d_out;       // [rows, 64]
  const Arg* arg;                 // [rows, 64]: the op's own index of the selected point
  const double* stats;            // forward's, training only
  int training;
};

// The c_in / c_out checks and the slot -> column table for c raw columns (3 <= c <= 6, checked by the caller).
inline int make_cols(int32_t c, int32_t c_in, int32_t c_out, int use_absolute_xyz, int with_distance, int* col) {
  const int base = use_absolute_xyz ? c : c - 3;
  if (c_in != base + 6 + (with_distance ? 1 : 0) || c_in > 16) return SPX_ERR_INVALID_ARG;
  if (c_out != kCout) return SPX_ERR_UNSUPPORTED;
  const int x0 = use_absolute_xyz ? 3 : 0;      // first column of the raw features past xyz
  for (int j = 0; j < 3; ++j) {
    col[j] = use_absolute_xyz ? j : -1;
    col[3 + j] = base + j;
    col[6 + j] = base + 3 + j;
    col[10 + j] = 3 + j < c ? x0 + j : -1;
  }
  col[9] = with_distance ? base + 6 : -1;
  return SPX_OK;
}

// A pillar centre in float32 with the product and the sum rounded separately, as the reference's two tensor ops round
// them (hipcc contracts a * b + c into one fma by default, also through __fmul_rn / __fadd_rn).
__device__ __forceinline__ float centre32(int32_t cell, float voxel, float offset) {
#pragma clang fp contract(off)
  const float prod = (float)cell * voxel;
  return prod + offset;
}

template <typename Geo>
__device__ __forceinline__ void load_w(const float* __restrict__ weight, const Geo& g, int ch, double* w) {
#pragma unroll
  for (int k = 0; k < kSlots; ++k) w[k] = g.col[k] >= 0 ? (double)weight[ch * g.c_in + g.col[k]] : 0.0;
}

__device__ __forceinline__ double dot13(const double* w, const double* __restrict__ f) {
  double x = 0.0;
#pragma unroll
  for (int k = 0; k < kSlots; ++k) x = fma(w[k], f[k], x);
  return x;
}

// (scale, shift) of channel ch.  ss: the folded pair of stats_channel, or nullptr: fold the running statistics (eval).
__device__ __forceinline__ void fold_scale_shift(const BN& bn, const double* __restrict__ ss, int ch, double& scale,
                                                 double& shift) {
  if (ss) {
    scale = ss[ch];
    shift = ss[kCout + ch];
  } else {
    const double invstd = 1.0 / sqrt((double)bn.running_var[ch] + (double)bn.eps);
    scale = (double)bn.gamma[ch] * invstd;
    shift = (double)bn.beta[ch] - (double)bn.running_mean[ch] * scale;
  }
}

// The per-channel body of k_stats_final, thread e = channel e < 64.  s: the summed G, S1 in LDS; n: the BatchNorm row
// count; update: whether the running statistics move (each op's policy; an op that allows n == 1 gets the biased variance
// there, as no unbiased one exists).  bn and b are taken by value in the two helpers that follow on purpose: by
// reference hipcc schedules the kernels around them differently (same results, another instruction order).
template <typename Geo>
__device__ __forceinline__ void stats_channel(const BN bn, const Geo& g, const double* s, double n, bool update, int e,
                                              double* stats, double* ss, float* save_mean, float* save_invstd) {
  double w[kSlots];
  load_w(bn.weight, g, e, w);
  double mean = 0.0, var = 0.0;
  if (n > 0.0) {
    double sx = 0.0, sxx = 0.0;
#pragma unroll
    for (int a = 0; a < kSlots; ++a) {
      sx = fma(w[a], s[kG + a], sx);
      double r = 0.0;
#pragma unroll
      for (int b = 0; b < kSlots; ++b) r = fma(s[a * kSlots + b], w[b], r);
      sxx = fma(w[a], r, sxx);
    }
    mean = sx / n;
    var = sxx / n - mean * mean;
    if (!(var > 0.0)) var = 0.0;
  }
  const double invstd = 1.0 / sqrt(var + (double)bn.eps);
  const double scale = (double)bn.gamma[e] * invstd;
  stats[kOffMean + e] = mean;
  stats[kOffInv + e] = invstd;
  save_mean[e] = (float)mean;
  save_invstd[e] = (float)invstd;
  ss[e] = scale;
  ss[kCout + e] = (double)bn.beta[e] - mean * scale;
  if (update && bn.running_mean && bn.running_var) {
    const double mo = (double)bn.momentum;
    const double unbiased = n > 1.0 ? var * (n / (n - 1.0)) : var;
    bn.running_mean[e] = (float)((1.0 - mo) * (double)bn.running_mean[e] + mo * mean);
    bn.running_var[e] = (float)((1.0 - mo) * (double)bn.running_var[e] + mo * unbiased);
  }
}

// mean and invstd of channel ch for the backward: the forward's batch statistics, or the running ones (eval)
template <typename Arg>
__device__ __forceinline__ void mean_invstd(const BN bn, const Bwd<Arg> b, int ch, double& mean, double& invstd) {
  if (b.training) {
    mean = b.stats[kOffMean + ch];
    invstd = b.stats[kOffInv + ch];
  } else {
    mean = (double)bn.running_mean[ch];
    invstd = 1.0 / sqrt((double)bn.running_var[ch] + (double)bn.eps);
  }
}

// Partials [n_part, kAcc, 64] -> d_weight, d_gamma, d_beta: lane q adds blocks q, q + 4, ... in that order, the four
// lanes are joined in the order 0, 1, 2, 3, then the dW formula of the header.  One block of 256 threads.
template <typename Geo, typename Arg>
static __global__ __launch_bounds__(256) void pfn_k_bwd_final(Geo g, BN bn, Bwd<Arg> b, const double* __restrict__ part,
                                                              int n_part, float* __restrict__ d_weight,
                                                              float* __restrict__ d_gamma, float* __restrict__ d_beta) {
  __shared__ double red[3 * kAcc * kCout];
  const int q = threadIdx.x >> 6, ch = threadIdx.x & 63;
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  for (int blk = q; blk < n_part; blk += 4) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) acc[k] += part[((int64_t)blk * kAcc + k) * kCout + ch];
  }
  if (q > 0) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) red[((q - 1) * kAcc + k) * kCout + ch] = acc[k];
  }
  __syncthreads();
  if (q != 0) return;
#pragma unroll
  for (int k = 0; k < kAcc; ++k)
    for (int r = 0; r < 3; ++r) acc[k] += red[(r * kAcc + k) * kCout + ch];
  const double db = acc[0], dg = acc[1];
  double w[kSlots];
  load_w(bn.weight, g, ch, w);
  const double gamma = (double)bn.gamma[ch];
  double dw[kSlots];
  if (b.training) {
    const double* __restrict__ s = b.stats;
    const double n = s[kOffN], mean = s[kOffMean + ch], invstd = s[kOffInv + ch];
    const double rn = n > 0.0 ? 1.0 / n : 0.0;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
      double gw = 0.0;
#pragma unroll
      for (int j = 0; j < kSlots; ++j) gw = fma(s[k * kSlots + j], w[j], gw);
      const double s1 = s[kG + k];
      dw[k] = gamma * invstd * (acc[2 + k] - db * rn * s1 - dg * rn * invstd * (gw - mean * s1));
    }
  } else {
    const double invstd = 1.0 / sqrt((double)bn.running_var[ch] + (double)bn.eps);
#pragma unroll
    for (int k = 0; k < kSlots; ++k) dw[k] = gamma * invstd * acc[2 + k];
  }
#pragma unroll
  for (int k = 0; k < kSlots; ++k)
    if (g.col[k] >= 0) d_weight[ch * g.c_in + g.col[k]] = (float)dw[k];
  d_gamma[ch] = (float)dg;
  d_beta[ch] = (float)db;
}

}  // namespace
