// center_loss.hip — the centre head's two losses AND their gradients for one head and the whole batch (include/spx.h §22).
//
// Restates CenterHead.get_loss for one head: neg_loss_cornernet(clamp(sigmoid(hm), 1e-4, 1 - 1e-4), heatmap) with
// mask=None, and _reg_loss over the rows that _transpose_and_gather_feat takes from the concatenated regression maps
// (pcdet_amd/utils/loss_utils.py, pcdet_amd/models/dense_heads/center_head.py; reference pcdet/utils/loss_utils.py:420-542).
// The composition runs some fifty element-wise, reduction, cat, permute and gather launches forward and as many
// backward, and its gather's backward is an index-add with float atomics.  Here: THREE launches per call,
//   1. k_count_zero: the number of heatmap cells equal to 1, one integer partial per block, and the zero-fill of every
//      regression gradient map;
//   2. k_focal_reg: blocks [0, nF) stream hm / heatmap once, write d_hm and one double partial of the focal terms per
//      block; blocks [nF, ...) take 256 slots of one frame each, find the owner of every live cell in LDS, write the
//      regression gradients at the live cells and one double partial per column;
//   3. k_final: one block adds the partials in a fixed order and writes losses[2] and reg_loss[D].
// No float atomics anywhere, no host read: the outputs are bitwise reproducible and the call captures in a graph.  A
// batch without positives takes no other path: the normalisers clamp to 1 on the device and the positive sum is empty.
//
// Normalisers: COUNT FIRST.  num_pos comes from launch 1; sum(masks) is counted over the whole batch by every regression
// block of launch 2 (b * k integers), so every gradient this file stores is already the gradient of the weighted loss.
//
// Duplicate cells: the live slot with the LOWEST index among those of a frame that share a cell owns it; it alone writes
// that cell, the sum of the slots' contributions added in slot order (an O(K) scan of the frame's cells in LDS per slot).
//
// Clamp: the gradient w.r.t. the logit is exactly 0 where sigmoid(x) lies outside [1e-4, 1 - 1e-4] and passes AT the
// bound, as torch.clamp does (the convention point_loss.hip documents).  sign(0) = 0 in the L1 gradient, as torch's abs.
// Precision: sigmoid(x) and sigmoid(-x) are each computed from exp(-|x|), and a log is taken of the smaller of the two
// directly and of the larger as log1p(-smaller), so neither tail loses digits to 1 - p; sums are double.  heatmap values are taken to lie in [0, 1]: a cell equal to 1 is a
// positive, every other cell a negative with weight (1 - gt)^4.
#include "block_ops.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxRegs = 5;       // center, center_z, dim, rot, vel
constexpr int kMaxD = 10;         // regression columns
constexpr int kMaxK = 2048;       // slots per frame (one int each in LDS)
constexpr int kCountBlocks = 256; // launch 1's grid cap: one partial per thread of a later block
constexpr int kPerBlock = 4 * kBlock;
constexpr float kLo = 1e-4f, kHi = 0.9999f;   // the clamp's bounds as float32, as torch.clamp takes the Python scalars

struct RegMaps {
  float* grad[kMaxRegs];          // [b, ch, h, w]
  int ch[kMaxRegs];
  int vec[kMaxRegs];              // grad is 16-byte aligned: float4 zero-fill
  int n;                          // maps
  int d;                          // columns = sum of ch
  const float* pcol[kMaxD];       // column -> its channel's plane of frame 0
  float* gcol[kMaxD];
  int64_t fstride[kMaxD];         // floats from one frame's plane to the next: the map's ch * h * w
  float cw[kMaxD];                // code weights
};

// ---------------------------------------------------------------------------------------------------------- launch 1
__global__ __launch_bounds__(kBlock) void k_count_zero(const float* __restrict__ heatmap, int64_t n, int hvec, RegMaps m,
                                                       int64_t bhw, int32_t* __restrict__ pos_part) {
  __shared__ int sm[4];
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
  int c = 0;
  const int64_t n4 = hvec ? n >> 2 : 0;
  for (int64_t i = tid; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(heatmap)[i];
    c += (v.x == 1.f) + (v.y == 1.f) + (v.z == 1.f) + (v.w == 1.f);
  }
  for (int64_t i = n4 * 4 + tid; i < n; i += stride) c += heatmap[i] == 1.f;
  for (int r = 0; r < m.n; ++r) {
    float* __restrict__ g = m.grad[r];
    const int64_t nr = bhw * m.ch[r], nr4 = m.vec[r] ? nr >> 2 : 0;
    for (int64_t i = tid; i < nr4; i += stride) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = nr4 * 4 + tid; i < nr; i += stride) g[i] = 0.f;
  }
  c = spx_block_sum_all(c, sm);
  if (threadIdx.x == 0) pos_part[blockIdx.x] = c;
}

// ---------------------------------------------------------------------------------------------------------- launch 2

// One cell: its focal term (log(p) (1 - p)^2 on a positive, log(1 - p) p^2 (1 - gt)^4 otherwise, p the clamped sigmoid)
// and *d = d(-term * gscale) / d(logit).
__device__ __forceinline__ float focal_cell(float x, float gt, float gscale, float* d) {
  const float e = expf(-fabsf(x));                  // in [0, 1]: no overflow at either end
  const float big = 1.f / (1.f + e), small = e / (1.f + e);
  float p = x >= 0.f ? big : small, q = x >= 0.f ? small : big;     // sigmoid(x), sigmoid(-x)
  const bool inside = p >= kLo && p <= kHi;
  if (p < kLo) {
    p = kLo;
    q = kHi;
  } else if (p > kHi) {
    p = kHi;
    q = kLo;
  }
  float term, dterm;
  if (gt == 1.f) {
    const float lp = p < 0.5f ? logf(p) : log1pf(-q);     // the smaller of p, q carries the digits
    term = lp * q * q;
    dterm = q * q * (q - 2.f * p * lp);
  } else {
    const float w1 = 1.f - gt, w2 = w1 * w1, w = w2 * w2;
    const float lq = q < 0.5f ? logf(q) : log1pf(-p);
    term = lq * p * p * w;
    dterm = w * p * p * (2.f * q * lq - p);
  }
  *d = inside ? -dterm * gscale : 0.f;
  return term;
}

struct LossArgs {
  const float *hm, *heatmap;
  float* d_hm;
  int64_t n;                      // b c h w
  int hvec;                       // hm, heatmap and d_hm are 16-byte aligned
  int n_focal;                    // focal blocks
  int n_count;                    // blocks of launch 1
  const float* tb;                // [b, k, d]
  const int64_t *inds, *masks;    // [b, k]
  int b, k, split;                // split = regression blocks per frame
  int64_t hw;
  float cls_weight, loc_weight;
  const int32_t* pos_part;
  double *foc_part, *reg_part;    // [n_focal], [b * split, kMaxD]
  int32_t* num;                   // sum(masks) for launch 3
};

__global__ __launch_bounds__(kBlock) void k_focal_reg(LossArgs a, RegMaps m) {
  __shared__ int sm_i[4];
  __shared__ double sm_d[4];
  __shared__ int s_ind[kMaxK];
  __shared__ int s_last;
  const int t = threadIdx.x;
  if ((int)blockIdx.x < a.n_focal) {
    const int np = spx_block_sum_all(t < a.n_count ? a.pos_part[t] : 0, sm_i);
    const float gscale = a.cls_weight / fmaxf((float)np, 1.f);
    const int64_t base = (int64_t)blockIdx.x * kPerBlock;
    double s = 0.0;
    if (a.hvec && base + kPerBlock <= a.n) {
      const int64_t i4 = (base >> 2) + t;
      const float4 x = reinterpret_cast<const float4*>(a.hm)[i4];
      const float4 g = reinterpret_cast<const float4*>(a.heatmap)[i4];
      float4 d;
      float l = focal_cell(x.x, g.x, gscale, &d.x);
      l += focal_cell(x.y, g.y, gscale, &d.y);
      l += focal_cell(x.z, g.z, gscale, &d.z);
      l += focal_cell(x.w, g.w, gscale, &d.w);
      reinterpret_cast<float4*>(a.d_hm)[i4] = d;
      s = (double)l;
    } else {
      for (int j = 0; j < 4; ++j) {
        const int64_t i = base + j * kBlock + t;
        if (i < a.n) {
          float d;
          s += (double)focal_cell(a.hm[i], a.heatmap[i], gscale, &d);
          a.d_hm[i] = d;
        }
      }
    }
    s = spx_block_sum_all(s, sm_d);
    if (t == 0) a.foc_part[blockIdx.x] = s;
    return;
  }

  // ---- regression: this block owns slots [part * kBlock, (part + 1) * kBlock) of frame f
  const int rb = (int)blockIdx.x - a.n_focal, f = rb / a.split, part = rb % a.split;
  int c = 0;
  for (int64_t i = t; i < (int64_t)a.b * a.k; i += kBlock) c += a.masks[i] == 1;
  const int num = spx_block_sum_all(c, sm_i);
  if (rb == 0 && t == 0) a.num[0] = num;
  if (t == 0) s_last = -1;
  __syncthreads();
  for (int j = t; j < a.k; j += kBlock) {
    // a dead slot is never dereferenced; neither is a live one whose cell lies outside the map
    const bool live = a.masks[(int64_t)f * a.k + j] == 1;
    int64_t ind = live ? a.inds[(int64_t)f * a.k + j] : -1;
    if (ind < 0 || ind >= a.hw) ind = -1;
    s_ind[j] = (int)ind;
    if (ind >= 0) atomicMax(&s_last, j);
  }
  __syncthreads();
  const int last = s_last;
  const float inv = a.loc_weight / fmaxf((float)num, 1.f);
  double l[kMaxD];
#pragma unroll
  for (int col = 0; col < kMaxD; ++col) l[col] = 0.0;
  const int j = part * kBlock + t;
  const int ind = j < a.k ? s_ind[j] : -1;
  bool owner = ind >= 0;
  for (int i = 0; i < j && owner; ++i) owner = s_ind[i] != ind;
  if (owner) {
    float pred[kMaxD], g[kMaxD];
#pragma unroll
    for (int col = 0; col < kMaxD; ++col) {
      g[col] = 0.f;
      pred[col] = 0.f;
      if (col < m.d) pred[col] = m.pcol[col][f * m.fstride[col] + ind];
    }
    for (int i = j; i <= last; ++i) {
      if (s_ind[i] != ind) continue;
      const float* __restrict__ row = a.tb + ((int64_t)f * a.k + i) * m.d;
#pragma unroll
      for (int col = 0; col < kMaxD; ++col) {
        if (col < m.d) {
          const float diff = pred[col] - row[col];
          const float gs = m.cw[col] * inv;
          l[col] += (double)fabsf(diff);          // a NaN target makes the column NaN, as in the composition
          g[col] += diff > 0.f ? gs : (diff < 0.f ? -gs : 0.f);
        }
      }
    }
#pragma unroll
    for (int col = 0; col < kMaxD; ++col)
      if (col < m.d) m.gcol[col][f * m.fstride[col] + ind] = g[col];
  }
#pragma unroll
  for (int col = 0; col < kMaxD; ++col) {
    const double s = spx_block_sum_all(l[col], sm_d);
    if (t == 0) a.reg_part[(int64_t)rb * kMaxD + col] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------- launch 3
__global__ __launch_bounds__(kBlock) void k_final(LossArgs a, RegMaps m, float* __restrict__ losses,
                                                  float* __restrict__ reg_loss) {
  __shared__ int sm_i[4];
  __shared__ double sm_d[4];
  __shared__ double s_col[kMaxD];
  const int t = threadIdx.x;
  const int np = spx_block_sum_all(t < a.n_count ? a.pos_part[t] : 0, sm_i);
  double s = 0.0;
  for (int i = t; i < a.n_focal; i += kBlock) s += a.foc_part[i];
  s = spx_block_sum_all(s, sm_d);
  if (t == 0) losses[0] = (float)(-s / (double)(np > 1 ? np : 1) * (double)a.cls_weight);
  if (t < m.d) {
    double r = 0.0;
    int num = 0;
    if (a.k > 0) {
      num = a.num[0];
      for (int i = 0; i < a.b * a.split; ++i) r += a.reg_part[(int64_t)i * kMaxD + t];
    }
    r /= (double)(num > 1 ? num : 1);
    reg_loss[t] = (float)r;
    s_col[t] = r * (double)m.cw[t];
  }
  __syncthreads();
  if (t == 0) {
    double loc = 0.0;
    for (int col = 0; col < m.d; ++col) loc += s_col[col];
    losses[1] = (float)(loc * (double)a.loc_weight);
  }
}

inline int64_t focal_blocks(int64_t n) { return (n + kPerBlock - 1) / kPerBlock; }
inline int reg_split(int64_t k) { return (int)((k + kBlock - 1) / kBlock); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" size_t spx_center_head_loss_ws_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int64_t k) {
  if (b <= 0 || c <= 0 || h <= 0 || w <= 0 || k < 0) return spx_align(0) + 256;
  const int64_t n = (int64_t)b * c * h * w;
  return spx_align((size_t)focal_blocks(n) * 8) + spx_align((size_t)b * reg_split(k) * kMaxD * 8 + 8) +
         spx_align(kCountBlocks * 4) + spx_align(4);
}

extern "C" int spx_center_head_loss(const float* hm, const float* heatmap, const float* const* regs,
                                    const int32_t* reg_channels, int32_t n_regs, const float* target_boxes,
                                    const int64_t* inds, const int64_t* masks, int32_t b, int32_t c, int32_t h, int32_t w,
                                    int64_t k, const float* code_weights, float cls_weight, float loc_weight,
                                    float* losses, float* reg_loss, float* d_hm, float* const* d_regs, void* ws,
                                    size_t ws_bytes, spx_stream_t stream) {
  if (!hm || !heatmap || !regs || !reg_channels || !code_weights || !losses || !reg_loss || !d_hm || !d_regs || b < 0 ||
      c <= 0 || h <= 0 || w <= 0 || k < 0 || n_regs <= 0)
    return SPX_ERR_INVALID_ARG;
  if (k > 0 && (!target_boxes || !inds || !masks)) return SPX_ERR_INVALID_ARG;
  if (n_regs > kMaxRegs || k > kMaxK) return SPX_ERR_UNSUPPORTED;
  const int64_t hw = (int64_t)h * w;
  RegMaps m;
  m.n = n_regs;
  m.d = 0;
  for (int r = 0; r < kMaxRegs; ++r) {
    m.grad[r] = nullptr;
    m.ch[r] = 0;
    m.vec[r] = 0;
  }
  for (int r = 0; r < n_regs; ++r) {
    if (!regs[r] || !d_regs[r] || reg_channels[r] <= 0) return SPX_ERR_INVALID_ARG;
    if (m.d + (int64_t)reg_channels[r] > kMaxD) return SPX_ERR_UNSUPPORTED;
    m.grad[r] = d_regs[r];
    m.ch[r] = reg_channels[r];
    m.vec[r] = aligned16(d_regs[r]);
    for (int cc = 0; cc < reg_channels[r]; ++cc, ++m.d) {
      m.pcol[m.d] = regs[r] + cc * hw;
      m.gcol[m.d] = d_regs[r] + cc * hw;
      m.fstride[m.d] = reg_channels[r] * hw;
    }
  }
  for (int col = 0; col < kMaxD; ++col) {
    m.cw[col] = col < m.d ? code_weights[col] : 0.f;
    if (col >= m.d) {
      m.pcol[col] = nullptr;
      m.gcol[col] = nullptr;
      m.fstride[col] = 0;
    }
  }
  const int64_t cmax = c > kMaxD ? c : kMaxD;
  if (hw >= (1ll << 31) || (int64_t)b * cmax * hw >= (1ll << 31) || (int64_t)b * k >= (1ll << 31)) return SPX_ERR_TOO_LARGE;
  if (b == 0) return SPX_OK;
  if (!ws || ws_bytes < spx_center_head_loss_ws_bytes(b, c, h, w, k)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  const int64_t n = (int64_t)b * c * hw;
  LossArgs a;
  a.hm = hm;
  a.heatmap = heatmap;
  a.d_hm = d_hm;
  a.n = n;
  a.hvec = aligned16(hm) && aligned16(heatmap) && aligned16(d_hm);
  a.n_focal = (int)focal_blocks(n);
  a.tb = target_boxes;
  a.inds = inds;
  a.masks = masks;
  a.b = b;
  a.k = (int)k;
  a.split = reg_split(k);
  a.hw = hw;
  a.cls_weight = cls_weight;
  a.loc_weight = loc_weight;
  char* p = reinterpret_cast<char*>(ws);
  a.foc_part = reinterpret_cast<double*>(p);
  p += spx_align((size_t)a.n_focal * 8);
  a.reg_part = reinterpret_cast<double*>(p);
  p += spx_align((size_t)b * a.split * kMaxD * 8 + 8);
  int32_t* pos_part = reinterpret_cast<int32_t*>(p);
  a.pos_part = pos_part;
  p += spx_align(kCountBlocks * 4);
  a.num = reinterpret_cast<int32_t*>(p);
  int64_t work = n > (int64_t)b * m.d * hw ? n : (int64_t)b * m.d * hw;
  int64_t nb = (work + kPerBlock - 1) / kPerBlock;
  a.n_count = (int)(nb < kCountBlocks ? nb : kCountBlocks);
  hipLaunchKernelGGL(k_count_zero, dim3((unsigned)a.n_count), dim3(kBlock), 0, s, heatmap, n, a.hvec, m, (int64_t)b * hw,
                     pos_part);
  hipLaunchKernelGGL(k_focal_reg, dim3((unsigned)(a.n_focal + b * a.split)), dim3(kBlock), 0, s, a, m);
  hipLaunchKernelGGL(k_final, dim3(1), dim3(kBlock), 0, s, a, m, losses, reg_loss);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
