// point_loss.hip — the fast_cpc point head's losses AND their gradients in one pass (include/spx.h §17).
//
// Restates PointHeadVoteSASAStatisticDistillation.get_vote_layer_loss / get_cls_layer_loss / get_box_layer_loss with
// generate_centerness_label, get_rdiou and get_corner_loss_lidar, normalised as get_loss does (reference
// pcdet/models/dense_heads/point_head_vote_sasa_statistic_distillation.py:570-1011), with WeightedSmoothL1Loss (no code
// weights) and WeightedBinaryCrossEntropyLoss (pcdet/utils/loss_utils.py:141-203, 339-362), and
// PointSASALoss.loss_forward (loss_utils.py:706-753).  The reference runs several hundred element-wise, reduction and
// boolean-mask launches forward and backward on B x 512 .. B x 3072 rows, with host reads in between; here one thread per
// row computes its loss terms and d(loss)/d(prediction) at once.  Three launches per call, as anchor_loss.hip: the
// normaliser counts, the rows with one partial sum per block, and a last block that adds the partials in fixed order (no
// float atomics: bitwise reproducible).  Nothing is read back; a batch without positives takes no other path, its
// normalisers clamp to 1 and every positive-only term is skipped per row.
//
// Ties: where the reference takes min / max / clamp of two equal operands (measure zero in real data) torch splits the
// gradient between them; here the FIRST operand takes it, and clamp passes the gradient at its bound as torch does.
#include "block_ops.h"

namespace {

constexpr int kMaxC = 8;    // classes
constexpr int kMaxK = 32;   // angle bins
constexpr int kBlock = 256;
constexpr float kPi = 3.14159265358979323846f;

struct HeadArgs {
  const float *vote, *cls, *reg, *box;            // student [N,3] [N,C] [N,6+2K] [N,7]
  const float *t_cls, *t_reg, *t_box;             // teacher
  const int64_t *vote_lab, *cls_lab;              // [N]
  const float *vote_tgt, *reg_lab, *box_lab;      // [N,3] [N,6+2K] [N,7]
  int64_t n;
  int C, K;
  float w_vote, w_cls, w_off, w_acls, w_areg, w_iou, w_corner;
  float beta, cmin, cmax;
  int with_centerness, rdiou, corner;
};

// counts[0] = #vote_lab > 0, counts[1] = #cls_lab >= 0, counts[2] = #cls_lab > 0; one block
__global__ __launch_bounds__(1024) void k_head_counts(const int64_t* __restrict__ vote_lab,
                                                      const int64_t* __restrict__ cls_lab, int64_t n,
                                                      int32_t* __restrict__ counts) {
  __shared__ int s[3][16];
  int c0 = 0, c1 = 0, c2 = 0;
  for (int64_t r = threadIdx.x; r < n; r += 1024) {
    c0 += vote_lab[r] > 0;
    const int64_t l = cls_lab[r];
    c1 += l >= 0;
    c2 += l > 0;
  }
  for (int d = 32; d > 0; d >>= 1) {
    c0 += __shfl_down(c0, d, 64);
    c1 += __shfl_down(c1, d, 64);
    c2 += __shfl_down(c2, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s[0][threadIdx.x >> 6] = c0;
    s[1][threadIdx.x >> 6] = c1;
    s[2][threadIdx.x >> 6] = c2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int t = 0;
    for (int i = 0; i < 16; ++i) t += s[threadIdx.x][i];
    counts[threadIdx.x] = t;
  }
}

// smooth L1 of diff and its derivative (WeightedSmoothL1Loss.smooth_l1_loss; beta < 1e-5: L1)
__host__ __device__ __forceinline__ float sl1(float diff, float beta, float* d) {
  const float n = fabsf(diff);
  if (beta < 1e-5f) {
    *d = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
    return n;
  }
  if (n < beta) {
    *d = diff / beta;
    return 0.5f * n * n / beta;
  }
  *d = diff > 0.f ? 1.f : -1.f;
  return n - 0.5f * beta;
}

// WeightedSmoothL1Loss.forward's element: a NaN target is replaced by the input
__host__ __device__ __forceinline__ float sl1_target(float pred, float tgt, float beta, float* d) {
  return sl1(tgt != tgt ? 0.f : pred - tgt, beta, d);
}

__host__ __device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// binary cross entropy with logits: max(x, 0) - x t + log(1 + exp(-|x|)); d/dx = sigmoid(x) - t, d/dt = -x
__host__ __device__ __forceinline__ float bce_logits(float x, float t) {
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

// generate_centerness_label of one row (no gradient)
__host__ __device__ inline float centerness(const float* p, const float* b) {
  const float cx = p[0] - b[0], cy = p[1] - b[1], cz = p[2] - b[2];
  float sa, ca;
  sincosf(-b[6], &sa, &ca);
  const float lx = cx * ca - cy * sa, ly = cx * sa + cy * ca;
  const float loc[3] = {lx, ly, cz};
  float prod = 1.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = b[3 + k] / 2 - loc[k], hi = b[3 + k] / 2 + loc[k];
    prod *= (lo <= hi ? lo : hi) / (lo >= hi ? lo : hi);
  }
  return powf(prod < 1e-6f ? 1e-6f : prod, 1.f / 3.f);      // NaN (0 / 0) falls through, as torch.clamp lets it
}

// get_rdiou's rdiou of (b1 = prediction, b2 = constant) and g[7] = d rdiou / d b1
__host__ __device__ inline float rdiou_grad(const float* b1, const float* b2, float* g) {
  float s1, c1, s2, c2;
  sincosf(b1[6], &s1, &c1);
  sincosf(b2[6], &s2, &c2);
  const float t1 = s1 * c2, t2 = c1 * s2;
  const float dt1 = c1 * c2, dt2 = -s1 * s2;                // d/d b1[6]
  float sz[3], dsz[3];
  for (int k = 0; k < 3; ++k) {
    dsz[k] = b1[3 + k] <= 10.f ? 1.f : 0.f;
    sz[k] = b1[3 + k] <= 10.f ? b1[3 + k] : 10.f;
  }
  // per axis: edge e = clamp(min(hi1, hi2) - max(lo1, lo2), 0), de/d centre, de/d size
  float e[4], dep[3], des[3], det;
  for (int k = 0; k < 3; ++k) {
    const float lo1 = b1[k] - sz[k] / 2, hi1 = b1[k] + sz[k] / 2;
    const float lo2 = b2[k] - b2[3 + k] / 2, hi2 = b2[k] + b2[3 + k] / 2;
    const bool lo_first = lo1 >= lo2, hi_first = hi1 <= hi2;
    const float raw = (hi_first ? hi1 : hi2) - (lo_first ? lo1 : lo2);
    const float live = raw >= 0.f ? 1.f : 0.f;
    e[k] = raw >= 0.f ? raw : 0.f;
    dep[k] = live * ((hi_first ? 1.f : 0.f) - (lo_first ? 1.f : 0.f));
    des[k] = live * 0.5f * ((hi_first ? 1.f : 0.f) + (lo_first ? 1.f : 0.f)) * dsz[k];
  }
  {
    const float lo1 = t1 - 0.5f, hi1 = t1 + 0.5f, lo2 = t2 - 0.5f, hi2 = t2 + 0.5f;
    const bool lo_first = lo1 >= lo2, hi_first = hi1 <= hi2;
    const float raw = (hi_first ? hi1 : hi2) - (lo_first ? lo1 : lo2);
    e[3] = raw >= 0.f ? raw : 0.f;
    det = raw >= 0.f ? (hi_first ? dt1 : dt2) - (lo_first ? dt1 : dt2) : 0.f;
  }
  const float inter = e[0] * e[1] * e[2] * e[3];
  const float v1 = sz[0] * sz[1] * sz[2];
  const float uni = v1 + b2[3] * b2[4] * b2[5] - inter;
  // d(inter / uni) = d inter (uni + inter) / uni^2 - inter d v1 / uni^2
  const float a = (uni + inter) / (uni * uni), b = inter / (uni * uni);
  const float di[4] = {e[1] * e[2] * e[3], e[0] * e[2] * e[3], e[0] * e[1] * e[3], e[0] * e[1] * e[2]};
  const float dv[3] = {sz[1] * sz[2] * dsz[0], sz[0] * sz[2] * dsz[1], sz[0] * sz[1] * dsz[2]};
  for (int k = 0; k < 3; ++k) {
    g[k] = a * di[k] * dep[k];
    g[3 + k] = a * di[k] * des[k] - b * dv[k];
  }
  g[6] = a * di[3] * det;
  return inter / uni;
}

// get_corner_loss_lidar of (pred, gt): mean over the corners of the smaller of the smooth-L1 (beta 1) corner distances to
// gt and to gt turned by pi; g[7] += scale * d loss / d pred
__host__ __device__ inline float corner_loss_grad(const float* p, const float* q, float scale, float* g) {
  float sp, cp, sq, cq, sf, cf;
  sincosf(p[6], &sp, &cp);
  sincosf(q[6], &sq, &cq);
  sincosf(q[6] + kPi, &sf, &cf);
  float loss = 0.f;
  for (int i = 0; i < 8; ++i) {
    // corner order of boxes_to_corners_3d (the order only pairs the corners of the two boxes)
    const float tx = (i & 3) < 2 ? 0.5f : -0.5f, ty = ((i + 1) & 3) < 2 ? 0.5f : -0.5f, tz = i < 4 ? -0.5f : 0.5f;
    const float px = p[3] * tx, py = p[4] * ty;
    const float rx = px * cp - py * sp, ry = px * sp + py * cp;
    const float pc[3] = {rx + p[0], ry + p[1], p[5] * tz + p[2]};
    const float qx = q[3] * tx, qy = q[4] * ty, qz = q[5] * tz + q[2];
    const float a[3] = {qx * cq - qy * sq + q[0], qx * sq + qy * cq + q[1], qz};
    const float b[3] = {qx * cf - qy * sf + q[0], qx * sf + qy * cf + q[1], qz};
    float la = 0.f, lb = 0.f, da[3], db[3];
    for (int k = 0; k < 3; ++k) {
      la += sl1(pc[k] - a[k], 1.f, &da[k]);
      lb += sl1(pc[k] - b[k], 1.f, &db[k]);
    }
    const bool first = la <= lb;
    loss += first ? la : lb;
    const float* d = first ? da : db;
    const float w = scale * 0.125f;
    // d pc / d (x, y, z, dx, dy, dz, rz)
    g[0] += w * d[0];
    g[1] += w * d[1];
    g[2] += w * d[2];
    g[3] += w * (d[0] * tx * cp + d[1] * tx * sp);
    g[4] += w * (-d[0] * ty * sp + d[1] * ty * cp);
    g[5] += w * d[2] * tz;
    g[6] += w * (-d[0] * ry + d[1] * rx);
  }
  return loss * 0.125f;
}

// One row: writes its gradients (every element), returns its three loss terms already divided by their normalisers'
// clamp and multiplied by their weights.  inv_* = 1 / clamp(count, 1).
__host__ __device__ inline void head_row(const HeadArgs& g, int64_t r, float inv_nv, float inv_nc, float inv_np,
                                         float* __restrict__ d_vote, float* __restrict__ d_cls,
                                         float* __restrict__ d_reg, float* __restrict__ d_box, float out[3]) {
  const int C = g.C, K = g.K, W = 6 + 2 * g.K;
  float l_vote = 0.f, l_cls = 0.f, l_box = 0.f;
  // ---- vote: smooth L1 to the box centre on the vote positives
  const bool vpos = g.vote_lab[r] > 0;
  for (int k = 0; k < 3; ++k) {
    float d = 0.f;
    if (vpos) l_vote += sl1_target(g.vote[r * 3 + k], g.vote_tgt[r * 3 + k], g.beta, &d);
    d_vote[r * 3 + k] = vpos ? d * g.w_vote * inv_nv : 0.f;
  }
  l_vote *= g.w_vote * inv_nv;

  const int64_t label = g.cls_lab[r];
  const bool pos = label > 0, counted = label >= 0;
  float gbox[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float bp[7], bl[7], bt[7], cen = 0.f, rd = 0.f, grd[7];
  if (pos) {
    for (int k = 0; k < 7; ++k) {
      bp[k] = g.box[r * 7 + k];
      bl[k] = g.box_lab[r * 7 + k];
      bt[k] = g.t_box[r * 7 + k];
    }
    if (g.with_centerness || g.rdiou) {
      cen = centerness(&g.vote[r * 3], bl);
      rd = rdiou_grad(bp, bl, grd);
    }
  }
  // ---- cls: BCE against the (soft) one-hot, and against the teacher at temperature 3; mean over the classes
  {
    const float scale = counted ? g.w_cls * inv_nc / (float)C : 0.f;
    float soft = 1.f, dsoft = 0.f;     // the positive column's target and d target / d rdiou
    if (pos && g.with_centerness) {
      const float base = cen * rd + 1e-8f;
      const float q = powf(base, 0.25f);
      soft = g.cmin + (g.cmax - g.cmin) * q;
      dsoft = (g.cmax - g.cmin) * 0.25f * q / base * cen;
    }
    for (int c = 0; c < C; ++c) {
      const float x = g.cls[r * C + c];
      if (!counted) {
        d_cls[r * C + c] = 0.f;
        continue;
      }
      const bool hot = pos && label == c + 1;
      const float t = hot ? soft : 0.f;
      const float ts = sigmoidf(g.t_cls[r * C + c] / 3.f);
      l_cls += 0.5f * bce_logits(x, t) + 0.5f * bce_logits(x / 3.f, ts);
      d_cls[r * C + c] = scale * (0.5f * (sigmoidf(x) - t) + 0.5f * (sigmoidf(x / 3.f) - ts) / 3.f);
      if (hot && g.with_centerness) {
        const float dt = scale * 0.5f * -x * dsoft;
        for (int k = 0; k < 7; ++k) gbox[k] += dt * grd[k];
      }
    }
    l_cls *= scale;
  }
  // ---- box, positives only
  if (!pos) {
    for (int k = 0; k < W; ++k) d_reg[r * W + k] = 0.f;
    for (int k = 0; k < 7; ++k) d_box[r * 7 + k] = 0.f;
  } else {
    const float* rp = g.reg + r * W;
    const float* rl = g.reg_lab + r * W;
    const float* rt = g.t_reg + r * W;
    float* dr = d_reg + r * W;
    for (int k = 0; k < 6; ++k) {       // offsets against the labels and against the teacher
      float d0, d1;
      l_box += g.w_off * (0.5f * sl1_target(rp[k], rl[k], g.beta, &d0) + 0.5f * sl1_target(rp[k], rt[k], g.beta, &d1));
      dr[k] = g.w_off * 0.5f * (d0 + d1) * inv_np;
    }
    // angle bin: cross entropy against the first maximum of the label's bin columns
    int bin = 0;
    float mx = rp[6], lmx = rl[6];
    for (int j = 1; j < K; ++j) {
      if (rl[6 + j] > lmx) {
        lmx = rl[6 + j];
        bin = j;
      }
      mx = fmaxf(mx, rp[6 + j]);
    }
    float se = 0.f;
    for (int j = 0; j < K; ++j) se += expf(rp[6 + j] - mx);
    const float lse = mx + logf(se);
    l_box += g.w_acls * (lse - rp[6 + bin]);
    // bin residual: smooth L1 of the label-weighted sums
    float pr = 0.f, lr = 0.f;
    for (int j = 0; j < K; ++j) {
      dr[6 + j] = g.w_acls * (expf(rp[6 + j] - lse) - (j == bin ? 1.f : 0.f)) * inv_np;
      pr += rp[6 + K + j] * rl[6 + j];
      lr += rl[6 + K + j] * rl[6 + j];
    }
    float dres;
    l_box += g.w_areg * sl1_target(pr, lr, g.beta, &dres);
    for (int j = 0; j < K; ++j) dr[6 + K + j] = g.w_areg * dres * rl[6 + j] * inv_np;
    if (g.rdiou) {
      // 1 - (rdiou * centerness + 1e-8)^(1/4) against the labels and against the teacher's boxes, 0.5 / 0.5
      const float base = rd * cen + 1e-8f, q = powf(base, 0.25f);
      float grt[7];
      const float tcen = centerness(&g.vote[r * 3], bt);
      const float trd = rdiou_grad(bp, bt, grt);
      const float tbase = trd * tcen + 1e-8f, tq = powf(tbase, 0.25f);
      l_box += g.w_iou * (0.5f * (1.f - q) + (1.f - tq) * 0.5f);
      const float dq = -g.w_iou * 0.5f * 0.25f * q / base * cen * inv_np;
      const float dtq = -g.w_iou * 0.5f * 0.25f * tq / tbase * tcen * inv_np;
      for (int k = 0; k < 7; ++k) gbox[k] += dq * grd[k] + dtq * grt[k];
    }
    if (g.corner) {
      l_box += g.w_corner * 0.3f * corner_loss_grad(bp, bl, g.w_corner * 0.3f * inv_np, gbox);
      l_box += g.w_corner * 0.7f * corner_loss_grad(bp, bt, g.w_corner * 0.7f * inv_np, gbox);
    }
    l_box *= inv_np;
    for (int k = 0; k < 7; ++k) d_box[r * 7 + k] = gbox[k];
  }
  out[0] = l_vote;
  out[1] = l_cls;
  out[2] = l_box;
}

__global__ __launch_bounds__(kBlock) void k_head_rows(HeadArgs g, const int32_t* __restrict__ counts,
                                                      float* __restrict__ partial, float* __restrict__ d_vote,
                                                      float* __restrict__ d_cls, float* __restrict__ d_reg,
                                                      float* __restrict__ d_box) {
  __shared__ float sm[4];
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float l[3] = {0.f, 0.f, 0.f};
  if (r < g.n) {
    const float inv_nv = 1.f / fmaxf((float)counts[0], 1.f);
    const float inv_nc = 1.f / fmaxf((float)counts[1], 1.f);
    const float inv_np = 1.f / fmaxf((float)counts[2], 1.f);
    head_row(g, r, inv_nv, inv_nc, inv_np, d_vote, d_cls, d_reg, d_box, l);
  }
  for (int c = 0; c < 3; ++c) {
    const float s = spx_block_sum(l[c], sm);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * 3 + c] = s;
  }
}

// out[c] = sum over the blocks of partial[blk * ncomp + c], in a fixed order
__global__ __launch_bounds__(kBlock) void k_sum_partials(const float* __restrict__ partial, int64_t nblk, int ncomp,
                                                         float* __restrict__ out) {
  __shared__ float sm[4];
  for (int c = 0; c < ncomp; ++c) {
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < nblk; i += kBlock) s += partial[i * ncomp + c];
    const float t = spx_block_sum(s, sm);
    if (threadIdx.x == 0) out[c] = t;
  }
}

// ------------------------------------------------------------------------------------------------ SASA layer loss

__global__ __launch_bounds__(1024) void k_seg_count(const int64_t* __restrict__ labels, int64_t n,
                                                    int32_t* __restrict__ count) {
  __shared__ int s[16];
  int c = 0;
  for (int64_t r = threadIdx.x; r < n; r += 1024) c += labels[r] >= 0;
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int i = 0; i < 16; ++i) t += s[i];
    count[0] = t;
  }
}

// one row of PointSASALoss.loss_forward: the loss term (already scaled) and d_scores[r][0..S)
__host__ __device__ inline float seg_row(const float* __restrict__ scores, const int64_t* __restrict__ labels, int64_t r,
                                         int S, int num_class, int func, float scale, float* __restrict__ d_scores) {
  const int64_t label = labels[r];
  float loss = 0.f, dsum = 0.f;
  for (int c = 0; c < num_class; ++c) {
    const float x = scores[r * S + (S == 1 ? 0 : c)];
    const float t = (label > 0 && label == c + 1) ? 1.f : 0.f;
    const float p = sigmoidf(x);
    const float bce = bce_logits(x, t);
    float l, d;
    if (func == 0) {      // BCE, mean over the classes
      l = bce / (float)num_class;
      d = (p - t) / (float)num_class;
    } else {              // sigmoid focal, alpha 0.25, gamma 2, summed over the classes
      const float aw = t * 0.25f + (1.f - t) * 0.75f;
      const float pt = t * (1.f - p) + (1.f - t) * p;
      const float dpt = (1.f - 2.f * t) * p * (1.f - p);
      l = aw * pt * pt * bce;
      d = aw * (2.f * pt * dpt * bce + pt * pt * (p - t));
    }
    if (label < 0) l = d = 0.f;
    loss += l;
    if (S == 1)
      dsum += d;
    else
      d_scores[r * S + c] = d * scale;
  }
  if (S == 1) d_scores[r] = dsum * scale;
  return loss * scale;
}

__global__ __launch_bounds__(kBlock) void k_seg_rows(const float* __restrict__ scores, const int64_t* __restrict__ labels,
                                                     int64_t n, int S, int num_class, int func, float layer_weight,
                                                     const int32_t* __restrict__ count, float* __restrict__ partial,
                                                     float* __restrict__ d_scores) {
  __shared__ float sm[4];
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float l = 0.f;
  if (r < n) l = seg_row(scores, labels, r, S, num_class, func, layer_weight / fmaxf((float)count[0], 1.f), d_scores);
  const float s = spx_block_sum(l, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

inline int64_t n_blocks(int64_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

extern "C" size_t spx_point_head_loss_ws_bytes(int64_t n) {
  if (n < 0) n = 0;
  return spx_align((size_t)n_blocks(n) * 3 * 4) + spx_align(3 * 4);
}

extern "C" int spx_point_head_loss(const float* vote_coords, const float* cls_preds, const float* reg_preds,
                                   const float* box_preds, const float* t_cls_preds, const float* t_reg_preds,
                                   const float* t_box_preds, const int64_t* vote_cls_labels, const float* vote_reg_labels,
                                   const int64_t* cls_labels, const float* reg_labels, const float* box_labels, int64_t n,
                                   int32_t num_class, int32_t angle_bin_num, const float* params,
                                   int with_centerness, int rdiou, int corner, float* losses, float* d_vote, float* d_cls,
                                   float* d_reg, float* d_box, void* ws, size_t ws_bytes, spx_stream_t stream) {
  if (!vote_coords || !cls_preds || !reg_preds || !box_preds || !t_cls_preds || !t_reg_preds || !t_box_preds ||
      !vote_cls_labels || !vote_reg_labels || !cls_labels || !reg_labels || !box_labels || !params || !losses || !d_vote ||
      !d_cls || !d_reg || !d_box || n < 0 || num_class <= 0 || angle_bin_num <= 0)
    return SPX_ERR_INVALID_ARG;
  if (num_class > kMaxC || angle_bin_num > kMaxK) return SPX_ERR_UNSUPPORTED;
  if (n == 0) return SPX_OK;
  if (!ws || ws_bytes < spx_point_head_loss_ws_bytes(n)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  const int64_t nblk = n_blocks(n);
  float* partial = reinterpret_cast<float*>(ws);
  int32_t* counts = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + spx_align((size_t)nblk * 3 * 4));
  HeadArgs g;
  g.vote = vote_coords;
  g.cls = cls_preds;
  g.reg = reg_preds;
  g.box = box_preds;
  g.t_cls = t_cls_preds;
  g.t_reg = t_reg_preds;
  g.t_box = t_box_preds;
  g.vote_lab = vote_cls_labels;
  g.cls_lab = cls_labels;
  g.vote_tgt = vote_reg_labels;
  g.reg_lab = reg_labels;
  g.box_lab = box_labels;
  g.n = n;
  g.C = num_class;
  g.K = angle_bin_num;
  g.w_vote = params[0];
  g.w_cls = params[1];
  g.w_off = params[2];
  g.w_acls = params[3];
  g.w_areg = params[4];
  g.w_iou = params[6];        // params[5], point_similarity_weight, belongs to a loss get_loss does not call
  g.w_corner = params[7];
  g.beta = params[8];
  g.cmin = params[9];
  g.cmax = params[10];
  g.with_centerness = with_centerness != 0;
  g.rdiou = rdiou != 0;
  g.corner = corner != 0;
  hipLaunchKernelGGL(k_head_counts, dim3(1), dim3(1024), 0, s, vote_cls_labels, cls_labels, n, counts);
  hipLaunchKernelGGL(k_head_rows, dim3((unsigned)nblk), dim3(kBlock), 0, s, g, counts, partial, d_vote, d_cls, d_reg,
                     d_box);
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kBlock), 0, s, partial, nblk, 3, losses);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}

extern "C" size_t spx_point_seg_loss_ws_bytes(int64_t n) {
  if (n < 0) n = 0;
  return spx_align((size_t)n_blocks(n) * 4) + spx_align(4);
}

extern "C" int spx_point_seg_loss(const float* scores, const int64_t* labels, int64_t n, int32_t score_cols,
                                  int32_t num_class, int32_t func, float layer_weight, float* loss, float* d_scores,
                                  void* ws, size_t ws_bytes, spx_stream_t stream) {
  if (!scores || !labels || !loss || !d_scores || n < 0 || num_class <= 0 || (func != 0 && func != 1) ||
      (score_cols != 1 && score_cols != num_class))
    return SPX_ERR_INVALID_ARG;
  if (num_class > kMaxC) return SPX_ERR_UNSUPPORTED;
  if (n == 0) return SPX_OK;
  if (!ws || ws_bytes < spx_point_seg_loss_ws_bytes(n)) return SPX_ERR_WORKSPACE;
  hipStream_t s = spx_s(stream);
  const int64_t nblk = n_blocks(n);
  float* partial = reinterpret_cast<float*>(ws);
  int32_t* count = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + spx_align((size_t)nblk * 4));
  hipLaunchKernelGGL(k_seg_count, dim3(1), dim3(1024), 0, s, labels, n, count);
  hipLaunchKernelGGL(k_seg_rows, dim3((unsigned)nblk), dim3(kBlock), 0, s, scores, labels, n, (int)score_cols,
                     (int)num_class, (int)func, layer_weight, count, partial, d_scores);
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kBlock), 0, s, partial, nblk, 1, loss);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
