// roi_grid_pool.hip — rotated RoI bilinear pooling of a BEV feature map (include/spx.h §25).
//
// Replaces SECONDHead.roi_grid_pool (reference pcdet/models/roi_heads/second_head.py:53-110): a Python loop over frames,
// each with affine_grid + grid_sample on a (num_rois, C, H, W) expanded view of the frame's map.  One launch for the
// batch, one block per RoI.
//
// A block first works out, once per grid cell, the four bilinear taps (element offset into the map or -1, and weight) and
// keeps them in LDS; the C channels then reuse them.  The per-cell arithmetic is double: theta is formed from the fp32 RoI
// in double and rounded to fp32 (the reference's .float()), everything after it is double and the output is rounded once,
// so the result is the correctly rounded value of the float64 restatement (tests/proposal_targets_ref.py) up to the
// double roundings.  The op is bandwidth bound; the double work is G*G values per RoI plus four FMAs per output.
//
// Two channel loops, chosen by the map's channel stride:
//   channels_last (stride_c == 1): a wave reads 64 consecutive channels of one tap, 256 B per load.  The output order is
//     (C, G, G), so the 64 x G*G tile goes through LDS (row stride odd: ds_write_b32 banks are (a / 4) % 32 over 32-lane
//     groups, so a group's column writes lane * odd + cell hit 32 different banks) and leaves as one contiguous run of
//     64 * G*G floats.
//   any other layout (NCHW): lanes run over (channel, cell) in output order, so stores are contiguous and the gathers of
//     neighbouring lanes fall on neighbouring pixels of one channel plane.
#include "spx_common.h"

namespace {

constexpr int kMaxG = 12;                 // G * G <= 144 cells: taps + tile stay under 48 KiB of LDS
constexpr int kThreads = 256;
constexpr int kChunk = 64;                // channels per LDS tile on the channels_last path

struct Taps {
  int64_t off[4];                         // y * stride_h + x * stride_w, or -1: outside the map
  double w[4];
};

__device__ __forceinline__ void cell_taps(const float* __restrict__ roi, int i, int j, int g, int h, int w, double min_x,
                                          double min_y, double sx, double sy, int64_t stride_h, int64_t stride_w,
                                          Taps* t) {
  const double cx = roi[0], cy = roi[1], dx = roi[3], dy = roi[4], ang = roi[6];
  const double x1 = (cx - dx / 2 - min_x) / sx, x2 = (cx + dx / 2 - min_x) / sx;
  const double y1 = (cy - dy / 2 - min_y) / sy, y2 = (cy + dy / 2 - min_y) / sy;
  const double ca = cos(ang), sa = sin(ang);
  // theta, rounded to fp32 as the reference's .float() does
  const double t00 = (double)(float)((x2 - x1) / (w - 1) * ca), t01 = (double)(float)((x2 - x1) / (w - 1) * (-sa));
  const double t02 = (double)(float)((x1 + x2 - w + 1) / (w - 1));
  const double t10 = (double)(float)((y2 - y1) / (h - 1) * sa), t11 = (double)(float)((y2 - y1) / (h - 1) * ca);
  const double t12 = (double)(float)((y1 + y2 - h + 1) / (h - 1));
  const double bx = (2.0 * j + 1.0) / g - 1.0, by = (2.0 * i + 1.0) / g - 1.0;
  const double gx = t00 * bx + t01 * by + t02, gy = t10 * bx + t11 * by + t12;
  const double ix = ((gx + 1.0) * w - 1.0) / 2.0, iy = ((gy + 1.0) * h - 1.0) / 2.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    t->off[k] = -1;
    t->w[k] = 0.0;
  }
  // a sample with a tap inside the map has -1 < ix < w and -1 < iy < h; NaN and infinities fail the comparisons
  if (!(ix > -1.0 && ix < (double)w && iy > -1.0 && iy < (double)h)) return;
  const double fx = floor(ix), fy = floor(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const double wx1 = ix - fx, wx0 = 1.0 - wx1, wy1 = iy - fy, wy0 = 1.0 - wy1;
  const int xs[4] = {x0, x0 + 1, x0, x0 + 1}, ys[4] = {y0, y0, y0 + 1, y0 + 1};
  const double ws[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (xs[k] >= 0 && xs[k] < w && ys[k] >= 0 && ys[k] < h) {
      t->off[k] = (int64_t)ys[k] * stride_h + (int64_t)xs[k] * stride_w;
      t->w[k] = ws[k];
    }
}

__device__ __forceinline__ float sample(const float* __restrict__ plane, const Taps& t, int64_t c_off) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (t.off[k] >= 0) acc += t.w[k] * (double)plane[t.off[k] + c_off];
  return (float)acc;
}

template <bool CHANNELS_LAST>
__global__ __launch_bounds__(kThreads) void k_roi_grid_pool(const float* __restrict__ rois, int64_t n_rois_per_frame,
                                                            int roi_stride, int64_t total, const int64_t* __restrict__ d_n,
                                                            const float* __restrict__ feat, int c, int h, int w,
                                                            int64_t stride_b, int64_t stride_c, int64_t stride_h,
                                                            int64_t stride_w, int g, double min_x, double min_y, double sx,
                                                            double sy, float* __restrict__ out) {
  extern __shared__ double lds[];         // Taps[G * G], then on the channels_last path float[kChunk * (G * G | 1)]
  const int gg = g * g;
  Taps* taps = reinterpret_cast<Taps*>(lds);
  float* tile = reinterpret_cast<float*>(taps + gg);
  const int64_t r = blockIdx.x;
  if (r >= total) return;
  float* o = out + r * (int64_t)c * gg;
  const int64_t n_out = (int64_t)c * gg;
  if (r >= spx_live_n(d_n, total)) {       // a dead row: zeros, its RoI is not read
    for (int64_t e = threadIdx.x; e < n_out; e += kThreads) o[e] = 0.f;
    return;
  }
  const float* roi = rois + r * roi_stride;
  const float* plane = feat + (r / n_rois_per_frame) * stride_b;
  for (int cell = threadIdx.x; cell < gg; cell += kThreads)
    cell_taps(roi, cell / g, cell % g, g, h, w, min_x, min_y, sx, sy, stride_h, stride_w, &taps[cell]);
  __syncthreads();
  if (CHANNELS_LAST) {
    const int ld = gg | 1;                 // odd row stride: the 32 lanes of a write group fall on 32 banks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c0 = 0; c0 < c; c0 += kChunk) {
      const int nc = min(kChunk, c - c0);
      if (lane < nc)
        for (int cell = wave; cell < gg; cell += kThreads / 64) tile[lane * ld + cell] = sample(plane, taps[cell], c0 + lane);
      __syncthreads();
      float* oc = o + (int64_t)c0 * gg;
      for (int e = threadIdx.x; e < nc * gg; e += kThreads) oc[e] = tile[(e / gg) * ld + e % gg];
      __syncthreads();
    }
  } else {
    for (int64_t e = threadIdx.x; e < n_out; e += kThreads) {
      const int ch = (int)(e / gg), cell = (int)(e % gg);
      o[e] = sample(plane, taps[cell], (int64_t)ch * stride_c);
    }
  }
}

}  // namespace

extern "C" int spx_roi_grid_pool_bev(const float* rois, int32_t batch, int64_t n_rois, int32_t roi_stride,
                                     const int64_t* d_n, const float* features, int32_t c, int32_t h, int32_t w,
                                     int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                                     int32_t grid_size, double min_x, double min_y, double step_x, double step_y,
                                     float* out, spx_stream_t stream) {
  if (batch < 0 || n_rois < 0 || roi_stride < 7 || c < 1 || h < 2 || w < 2 || grid_size < 1) return SPX_ERR_INVALID_ARG;
  if (!(step_x > 0.0) || !(step_y > 0.0) || stride_b < 0 || stride_c < 1 || stride_h < 1 || stride_w < 1)
    return SPX_ERR_INVALID_ARG;
  if (grid_size > kMaxG) return SPX_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)batch * n_rois;
  if (total == 0) return SPX_OK;
  if (!rois || !features || !out) return SPX_ERR_INVALID_ARG;
  if (total >= (int64_t(1) << 31) || (int64_t)c * grid_size * grid_size >= (int64_t(1) << 31)) return SPX_ERR_TOO_LARGE;
  hipStream_t s = spx_s(stream);
  const int gg = grid_size * grid_size;
  const size_t lds_taps = (size_t)gg * sizeof(Taps), lds_tile = (size_t)kChunk * (gg | 1) * sizeof(float);
  if (stride_c == 1)
    hipLaunchKernelGGL((k_roi_grid_pool<true>), dim3((unsigned)total), dim3(kThreads), lds_taps + lds_tile, s, rois, n_rois, roi_stride, total,
                       d_n, features, c, h, w, stride_b, stride_c, stride_h, stride_w, grid_size, min_x, min_y, step_x,
                       step_y, out);
  else
    hipLaunchKernelGGL((k_roi_grid_pool<false>), dim3((unsigned)total), dim3(kThreads), lds_taps, s, rois, n_rois, roi_stride, total,
                       d_n, features, c, h, w, stride_b, stride_c, stride_h, stride_w, grid_size, min_x, min_y, step_x,
                       step_y, out);
  SPX_CHECK_LAUNCH();
  return SPX_OK;
}
