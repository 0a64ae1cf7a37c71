/*
 * spx.h — C ABI of libspx.so: the MI355X (gfx950) sparse-3D-convolution kernel library.
 *
 * This is the drop-in boundary "B3" of SURVEY.md §8(b).  The reference repository
 * (blindopen/TSM-Det-Pointcloud-, an OpenPCDet 0.5.2 fork) reaches all of this arithmetic through
 * the third-party `spconv.pytorch` / `spconv.utils` / `cumm.tensorview` Python packages
 * (pinned spconv_cu118==2.3.8, cumm_cu118==0.7.11, reference `requirements.txt:1,21`), which are
 * not vendored; every entry point below therefore cites the reference CALL SITE it serves.
 *
 * Conventions (all entry points):
 *   - plain C, `extern "C"`, no torch / C++ types in any signature;
 *   - every pointer named d_* or documented "device" is a device (HBM) pointer owned by the caller;
 *     the library never allocates, frees, or synchronises: all scratch comes in through (ws, ws_bytes),
 *     sized by the matching *_ws_bytes() query;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every kernel is enqueued on
 *     it and the call returns immediately (graph-capture safe);
 *   - data-dependent counts (number of voxels, number of active outputs) are RETURNED THROUGH DEVICE
 *     POINTERS and may be CONSUMED through device pointers (`d_n*` arguments, nullable): when a `d_n`
 *     argument is non-NULL the kernels read the live row count from it (it must be <= the host-side
 *     capacity `n` that sizes the launch); when NULL the host value `n` is exact.  This lets a caller
 *     chain voxelise -> rulebooks -> convolutions with no host synchronisation in between;
 *   - return value: 0 (SPX_OK) or a negative SPX_ERR_* code; never throws, never exits;
 *   - re-entrant; no global mutable state; one HIP context per process;
 *   - row indices are int32, linear voxel keys are 64-bit, features are fp32 row-major [rows, channels];
 *   - voxel indices are int32 [rows,4] = (batch, z, y, x), spatial shapes are (D,H,W) = (z,y,x) extents.
 */
#ifndef SPX_H_
#define SPX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPX_ABI_VERSION 3

#define SPX_OK 0
#define SPX_ERR_INVALID_ARG (-1)  /* null pointer, non-positive extent, kernel volume > SPX_MAX_KVOL ... */
#define SPX_ERR_WORKSPACE (-2)    /* ws == NULL or ws_bytes smaller than the *_ws_bytes() answer          */
#define SPX_ERR_UNSUPPORTED (-3)  /* channel count / mode this build has no kernel for                     */
#define SPX_ERR_LAUNCH (-4)       /* hipGetLastError() != hipSuccess after a launch                        */
#define SPX_ERR_TOO_LARGE (-5)    /* rows >= 2^31 or grid cells >= 2^40                                    */
#define SPX_ERR_CAPACITY (-7)     /* DEVICE-side: a strided rule table found more active outputs than the caller's row
                                     capacity (static-capacity mode); rows beyond it were dropped; via d_status          */
#define SPX_ERR_TABLE_FULL (-6)   /* DEVICE-side: a hash probe sequence found no free slot (stale workspace declared
                                     pre-cleared); reported through a d_status word, see spx_read_status()  */
#define SPX_ERR_RING_STALL (-8)   /* DEVICE-side: a wave of spx_conv_gemm_ring gave up a (bounded) wait on the weight ring:
                                     the launch's output is incomplete; via d_status.  Never seen; the exit exists so that a
                                     protocol fault ends as an error code and not as a hung GPU                            */
#define SPX_ERR_BATCH_STATS (-10) /* DEVICE-side: a training-mode forward of spx_dynamic_pillar_vfe_fwd met fewer than two
                                     kept points (torch raises there); the running statistics and the counter were left
                                     untouched                                                                           */
#define SPX_ERR_OUT_OF_GRID (-9)  /* DEVICE-side: spx_voxel_table_build met a live row whose (batch, z, y, x) lies outside the
                                     table; the row was skipped; via d_status                                               */

/* flags of the entry points that keep a hash table in their workspace (spx_voxelize, spx_subm_rulebook) */
#define SPX_WS_PRECLEARED 1 /* the caller has already initialised the workspace (hash keys = 0xFF bytes, values / point
                               slots = 0x7F bytes, e.g. by one bulk fill for several calls): the library skips its own
                               clearing launches.  A workspace that is NOT clean makes the kernels drop the rows they cannot
                               place and raise SPX_ERR_TABLE_FULL in d_status; every probe loop is bounded by the slot count */

#define SPX_ROWS_UNIQUE 2   /* spx_subm_rulebook: the caller guarantees one row per cell (a voxeliser's output; what spconv
                               requires of SparseConvTensor.indices).  The table is then symmetric and only half of it is probed,
                               every hit written twice.  With duplicate rows under this flag the result is undefined (without
                               it duplicates resolve to the smallest row)                                                  */

#define SPX_MAX_KVOL 32 /* largest kernel volume kz*ky*kx supported (27 = 3x3x3 is the reference's max) */

typedef void *spx_stream_t;

/* Human-readable text for an SPX_ERR_* code (static storage). */
const char *spx_strerror(int code);
/* Returns SPX_ABI_VERSION of the loaded library. */
int spx_abi_version(void);

/* Device status word.  Errors that only a kernel can detect (SPX_ERR_TABLE_FULL) are written with atomicMin into a
 * caller-owned device int32 (`d_status`, nullable, initialised to 0 by the caller, sticky across calls).
 * spx_read_status copies it to the host — the ONE entry point that synchronises `stream` — and returns it (0 or a negative
 * SPX_ERR_* code).  A caller that reads a row count back anyway can fetch the word with the same copy instead. */
int spx_read_status(const int32_t *d_status, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 1. Hard voxelisation (+ fused MeanVFE)
 *    replaces: spconv.utils.Point2VoxelCPU3d(...).point_to_voxel(tv.from_numpy(points))
 *      reference call site pcdet/datasets/processor/data_processor.py:37-43,55 (VoxelGeneratorWrapper),
 *      driven by DataProcessor.transform_points_to_voxels, data_processor.py:127-155, and the batch
 *      concatenation of DatasetTemplate.collate_batch, pcdet/datasets/dataset.py:161-229;
 *    and (mean != NULL) MeanVFE.forward, pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31.
 *
 *    Semantics: for each point in input order, c_j = floor((p_j-lo_j)/vsize_j)
 *    in fp32 with a true division; the point is dropped if any c_j is outside [0, grid_j).  Voxels are
 *    numbered in first-occurrence order per frame; a new voxel is created only while the frame has
 *    fewer than max_voxels; a point is appended to its voxel only while the voxel holds fewer than
 *    max_points points.  Frames are processed independently and emitted batch-major.
 *
 *    points     device [n_points, point_stride] fp32.  xyz = columns xyz_col..xyz_col+2; the `c`
 *               features copied to the voxel are columns feat_col..feat_col+c-1.
 *    batch_col  column holding the frame index as a float (collate_batch's leading column), or -1
 *               for a single frame.  Points of one frame must be contiguous, frames ascending.
 *    range      host float[6] = (x0,y0,z0,x1,y1,z1); vsize host float[3] = (vx,vy,vz);
 *    grid       host int32[3] = (gx,gy,gz) = round((hi-lo)/vsize), data_processor.py:129-130.
 *    voxels     device [cap, max_points, c] fp32, zero padded (may be NULL when only `mean` is wanted)
 *    coords     device [cap, 4] int32 (b,z,y,x)
 *    num_points device [cap] int32
 *    mean       device [cap, c] fp32 = sum over kept points / max(num,1)  (NULL to skip)
 *    d_num_voxels device int64[1]: total voxels M written (rows [0,M) of every output are valid)
 *    cap        rows available in the outputs; must be >= min(n_points, batch*max_voxels)
 *    flags      0 or SPX_WS_PRECLEARED;  d_status: device status word (nullable), see spx_read_status()
 * ---------------------------------------------------------------------------------------------- */
size_t spx_voxelize_ws_bytes(int64_t n_points, int batch, int max_points);
int spx_voxelize(const float *points, int64_t n_points, int point_stride, int xyz_col, int feat_col, int c,
                 int batch_col, int batch, const float *range, const float *vsize, const int32_t *grid,
                 int max_points, int max_voxels, float *voxels, int32_t *coords, int32_t *num_points,
                 float *mean, int64_t *d_num_voxels, int64_t cap, int flags, int32_t *d_status, void *ws,
                 size_t ws_bytes, spx_stream_t stream);

/* Stand-alone MeanVFE for voxels produced elsewhere (e.g. by CPU dataloader workers):
 * out[v,:] = sum_t voxels[v,t,:] / max(num[v],1); replaces mean_vfe.py:26-29. */
int spx_mean_vfe(const float *voxels, const int32_t *num_points, int64_t n, const int64_t *d_n, int max_points,
                 int c, float *out, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 1b. Dynamic voxelisation + mean (SURVEY.md §8a row a5')
 *    replaces: DynamicMeanVFE.forward, pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py:38-76
 *      (torch.floor((xyz - range_min) / voxel_size).int(), in-range mask, merge key, torch.unique, scatter_mean).
 *    Every in-range point is kept (no per-voxel / per-frame caps).  Voxels = unique cells in ASCENDING key
 *      ((b*X + cx)*Y + cy)*Z + cz  (the order torch.unique yields in the reference).
 *      points          device [n_points, stride] f32; column batch_col = frame index (or -1: single frame), columns
 *                      [xyz_col, xyz_col + num_features) = x, y, z, extra features
 *      voxel_features  device [cap, num_features] f32 : mean of those columns over the voxel's points, summed in point
 *                      order (the reference sums with float atomics; this is bitwise reproducible)
 *      voxel_coords    device [cap, 4] int32 (b, z, y, x)  -- the column order the reference returns (:72)
 *      point_to_voxel  device [n_points] int32 : voxel row of every point (torch.unique's inverse), -1 if dropped
 *      d_num_voxels    device int64 : number of voxels (may exceed cap: rows beyond cap are dropped)
 *      grid3 = (X, Y, Z) cells; range6 = (xmin, ymin, zmin, xmax, ymax, zmax); voxel_size3 = (vx, vy, vz)
 * ---------------------------------------------------------------------------------------------- */
size_t spx_dynamic_voxelize_ws_bytes(int64_t n_points, int batch, const int32_t *grid3, int64_t cap);
int spx_dynamic_voxelize(const float *points, int64_t n_points, int stride, int batch_col, int xyz_col, int num_features,
                         const float *range6, const float *voxel_size3, const int32_t *grid3, int batch,
                         float *voxel_features, int32_t *voxel_coords, int32_t *point_to_voxel, int64_t *d_num_voxels,
                         int64_t cap, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 2. Submanifold rulebook (hash insert + kernel-offset probe)
 *    replaces: the indice-pair build inside spconv.pytorch.SubMConv3d.forward, reference call sites
 *      pcdet/models/backbones_3d/spconv_backbone.py:86,93,99-100,106-107,113-114 (indice_key subm1..4).
 *    pair[k*pair_ld + o] = row of the active voxel at coord(o) + (k - ksize/2)*dil in the same batch
 *    element, or -1;  k = (kz*KH + ky)*KW + kx.   Output rows == input rows (same order).
 *    The backward (dgrad) table of a submanifold conv is the same table read at K-1-k.
 *    cnt    device int32[K]: number of valid pairs per offset (may be NULL).
 *    flags  0 or SPX_WS_PRECLEARED;  d_status: device status word (nullable), see spx_read_status().
 * ---------------------------------------------------------------------------------------------- */
size_t spx_subm_rulebook_ws_bytes(int64_t n);
int spx_subm_rulebook(const int32_t *idx, int64_t n, const int64_t *d_n, int batch, const int32_t *shape,
                      const int32_t *ksize, const int32_t *dil, int32_t *pair, int64_t pair_ld, int32_t *cnt,
                      int flags, int32_t *d_status, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 3. Regular (strided) sparse-convolution rulebook
 *    replaces: the indice-pair build inside spconv.pytorch.SparseConv3d.forward, reference call sites
 *      spconv_backbone.py:98,105,112 (k3 s2, keys spconv2..4) and :121-122 (k(3,1,1) s(2,1,1), spconv_down2).
 *    Candidate outputs o = (i + pad - k*dil)/stride where divisible and 0 <= o < out_shape;
 *    out_idx = unique candidates in ASCENDING linear key ((b*D+z)*H+y)*W+x (canonical order).
 *      out_shape  host int32[3] = floor((in + 2*pad - dil*(k-1) - 1)/stride) + 1  (caller computes; checked)
 *      out_idx    device [cap,4] int32
 *      pair_fwd   device [K, cap]  int32 : pair_fwd[k*cap + o] = input row feeding output o at offset k, or -1
 *      pair_bwd   device [K, n_in] int32 : pair_bwd[k*n_in + i] = output row fed by input i at offset k, or -1
 *      cnt        device int32[K] (nullable);  d_n_out device int64[1] = number of active outputs
 *      cap        output-row capacity.  spx_conv_out_cap() = min(prod(ceil(k/s)) * n_in, batch*out cells) can never
 *                 overflow; a smaller static capacity is allowed (graph mode): rows beyond cap are dropped and
 *                 *d_n_out still reports the true count, so *d_n_out > cap signals overflow, and the status word
 *                 d_status (nullable, see spx_read_status) receives SPX_ERR_CAPACITY
 *      subm_pair  (nullable) device [Ks, cap] int32: the SUBMANIFOLD table of the output level (section 2 semantics over
 *                 out_idx, kernel subm_ksize / subm_dil, leading dimension cap) built from the same rank bitmap in the
 *                 same call — the reference's stages are a strided conv followed by submanifold convs on its output
 *                 (spconv_backbone.py:98-100,105-107,112-114), and the output rows are in rank order, so a neighbour
 *                 lookup is one bitmap word + a popcount: no hash is built for that level.  subm_cnt: int32[Ks], nullable
 * ---------------------------------------------------------------------------------------------- */
int64_t spx_conv_out_cap(int64_t n_in, int batch, const int32_t *out_shape, const int32_t *ksize,
                         const int32_t *stride);
size_t spx_conv_rulebook_ws_bytes(int64_t n_in, int batch, const int32_t *out_shape);
int spx_conv_rulebook(const int32_t *idx, int64_t n_in, const int64_t *d_n_in, int batch, const int32_t *in_shape,
                      const int32_t *out_shape, const int32_t *ksize, const int32_t *stride, const int32_t *pad,
                      const int32_t *dil, int32_t *out_idx, int32_t *pair_fwd, int32_t *pair_bwd, int32_t *cnt,
                      int64_t *d_n_out, int64_t cap, const int32_t *subm_ksize, const int32_t *subm_dil,
                      int32_t *subm_pair, int32_t *subm_cnt, int32_t *d_status, void *ws, size_t ws_bytes,
                      spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 4. Sparse convolution arithmetic
 *    replaces: spconv.pytorch.{SubMConv3d,SparseConv3d}.forward and their autograd backward, the 12
 *      call sites spconv_backbone.py:86,93,98-100,105-107,112-114,121; backward is triggered by
 *      loss.backward() at tools/train_utils/train_utils.py:53.
 *
 *    Weights arrive in the reference parameter layout  w[Cout][K][Cin]  (= spconv 2.x
 *    weight[Cout,kz,ky,kx,Cin], detector3d_template.py:547-562) and are re-laid for the MFMA operand
 *    order by spx_pack_weight (mode 0: forward operand W_k[ci][co]; mode 1: dgrad operand W_k^T; mode 2: both in one
 *    launch, forward operand first).  packed size = K*Cin*Cout floats (twice that for mode 2).
 *
 *    forward : out[o,co] = sum_k sum_ci in[pair[k*ld+o], ci] * w[co][k][ci]          (pair = forward table)
 *    dgrad   : din[i,ci] = sum_k sum_co dout[pairT[k*ld+i], co] * w[co][k][ci]       (pairT = backward table;
 *              for a submanifold conv pass the forward table and flip_k = 1)
 *      -> both are spx_conv_gemm: "rows of `src` gathered through `pair`, contracted with packed weights".
 *    Optional fused epilogue:  y = acc*scale[c] + shift[c] (both nullable), then ReLU if relu != 0.
 *    wgrad   : dw[co][k][ci] = sum_o dout[o,co] * in[pair[k*ld+o], ci]                (reference layout, fp32)
 *              (fixed summation order: bitwise reproducible from run to run)
 * ---------------------------------------------------------------------------------------------- */
int spx_pack_weight(const float *w, int cout, int kvol, int cin, int mode, float *packed, spx_stream_t stream);

/* All weights of a network in one launch: d_desc = device int64[n][6] = {w (device pointer, contiguous [Cout][K][Cin]), packed
 * (device pointer, 2*K*Cin*Cout floats: forward operand then dgrad operand, as mode 2), Cout, K, Cin, first block}; weight i
 * owns blocks [first block_i, first block_{i+1}) with ceil(2*K*Cin*Cout / 256) blocks each; total_blocks = their sum. */
int spx_pack_weight_batched(const int64_t *d_desc, int n, int64_t total_blocks, spx_stream_t stream);

int spx_conv_gemm(const float *src, int c_src, const float *w_packed, int c_dst, int kvol, int flip_k,
                  const int32_t *pair, int64_t pair_ld, int64_t n_dst, const int64_t *d_n_dst,
                  const float *scale, const float *shift, int relu, float *dst, spx_stream_t stream);

/* MFMA-work-balanced schedule of the same product (csrc/conv_balanced.hip): spx_conv_plan counts the non-empty
 * (16-row tile, offset) units of a rule table once and cuts them into equal ranges for a persistent grid; the plan
 * depends only on (pair, n_dst), so it is reused by every convolution that reads the table (forward, dgrad with
 * flip_k, the second layer of a submanifold pair).  spx_conv_gemm_balanced = spx_conv_gemm under that schedule;
 * returns SPX_ERR_UNSUPPORTED for channel pairs it does not cover (use spx_conv_gemm).  Same reference call sites.
 * Super-tiles whose offsets are split between workgroups are combined inside the launch (arrival counters kept in `plan`,
 * which is therefore not const: one launch per plan at a time — stream order is enough); partial sums are added in a fixed
 * order, so results are bitwise reproducible. */
/* Optional row order for that schedule (csrc/conv_group.hip): a 16-row MFMA tile multiplies offset k for all its rows
 * as soon as one of them has it, so tiles whose rows share the same offsets issue fewer wasted MFMAs.  spx_conv_group orders
 * the destination rows of a rule table by (window, group key) — windows = contiguous ranges of at most 4096 live rows, at
 * least eight of them (one XCD's L2 then serves one part of the feature matrix); group key = an 11-bit digest of the row's
 * offset mask (3x3x3: the nine in-plane offsets bit by bit, any offset in the plane below, any in the plane above) — stable
 * (equal keys keep the table order; rows beyond the live count keep their place), with a hand-written counting sort, and
 * writes perm[n_dst] (position -> table row) and pair_grouped[kvol][n_dst] = pair[k][perm[j]] (-1 beyond the live rows).
 * Build the plan over pair_grouped (ld = n_dst) and pass pair_grouped + perm to spx_conv_gemm_balanced: position j is
 * written to dst row perm[j].  Results do not depend on the row order (every row is the same sum over k).  kvol <= 30. */
size_t spx_conv_group_ws_bytes(int64_t n_dst);
int spx_conv_group(const int32_t *pair, int64_t pair_ld, int kvol, int64_t n_dst, const int64_t *d_n_dst, int32_t *perm,
                   int32_t *pair_grouped, void *ws, size_t ws_bytes, spx_stream_t stream);
/* perm (below): NULL = rows in table order */
size_t spx_conv_plan_bytes(int64_t n_dst);
int spx_conv_plan(const int32_t *pair, int64_t pair_ld, int kvol, int64_t n_dst, const int64_t *d_n_dst, int32_t *plan,
                  spx_stream_t stream);
size_t spx_conv_gemm_balanced_ws_bytes(int c_dst, int64_t n_dst);
int spx_conv_gemm_balanced(const float *src, int c_src, const float *w_packed, int c_dst, int kvol, int flip_k,
                           const int32_t *pair, int64_t pair_ld, int64_t n_dst, const int64_t *d_n_dst,
                           const float *scale, const float *shift, int relu, int32_t *plan, const int32_t *perm,
                           float *dst, void *ws, size_t ws_bytes, spx_stream_t stream);

/* Round-3 schedule of the same product (csrc/conv_ring.hip): every 16-row tile belongs to ONE wave for the whole launch
 * (no tile is split between workgroups: no partial-sum slabs, no tickets), the K weight slices stream through an LDS ring
 * filled by a loader wave, consumers run barrier-free.  spx_conv_ring_plan (cached per rule table, like spx_conv_plan) deals
 * the tiles to the chip's 1024 SIMDs by their number of non-empty offsets; the plan is written by the planning kernels only
 * (one debug counter aside), so any number of launches may share it.  pair / perm: exactly as spx_conv_gemm_balanced
 * (a table grouped by spx_conv_group, or the plain table with perm = NULL).  n_src = rows of `src` (entries are bounds-checked
 * against it by the buffer hardware: an entry of -1 reads zeros).  stats (nullable): [spx_conv_ring_stat_rows()][2][c_dst]
 * floats, row b = column sums of the written values and of their squares over the rows workgroup b wrote — the statistics
 * pass of the training-mode BatchNorm1d that follows (reference spconv_backbone.py:26-27,81), consumed by
 * spx_bn_relu_fwd_from_sums.  Every output row is the same sum over k in ascending order whatever the plan: bitwise
 * reproducible.  Channel pairs: (32|64) x (32|64); others SPX_ERR_UNSUPPORTED.  kvol <= 31.  d_status (nullable, see
 * spx_read_status) receives SPX_ERR_RING_STALL if a wave's bounded wait on the ring gave up. */
/* spx_conv_ring_tiles_per_wave(set): tuning knob of spx_conv_ring_plan, process-wide.  0 (default): by size — a wave holds one
 * 16-row tile per turn of the weight ring while one turn covers all live rows, two tiles (sharing the ring protocol of every
 * offset) beyond that; 1 / 2: always that many (environment SPX_RING_TM presets it; tests and A/B runs).  Returns the
 * setting; any other `set` only queries.  The plan records what it was dealt for and spx_conv_gemm_ring follows the plan. */
size_t spx_conv_ring_plan_bytes(int64_t n_dst);
int spx_conv_ring_stat_rows(void);
int spx_conv_ring_tiles_per_wave(int set);
int spx_conv_ring_plan(const int32_t *pair, int64_t pair_ld, int kvol, int64_t n_dst, const int64_t *d_n_dst, int32_t *plan,
                       spx_stream_t stream);
int spx_conv_gemm_ring(const float *src, int64_t n_src, int c_src, const float *w_packed, int c_dst, int kvol, int flip_k,
                       const int32_t *pair, int64_t pair_ld, int64_t n_dst, const int64_t *d_n_dst, const float *scale,
                       const float *shift, int relu, int32_t *plan, const int32_t *perm, float *dst, float *stats,
                       int32_t *d_status, spx_stream_t stream);

size_t spx_conv_wgrad_ws_bytes(int cin, int cout, int kvol, int64_t n_out);
/* counts (nullable): the table's pair counts from spx_conv_wgrad_counts (device, spx_conv_wgrad_counts_bytes); they depend on
 * the rule table only, so a table that serves several layers / steps of a replayed graph is counted once.  NULL: counted
 * inside the call. */
size_t spx_conv_wgrad_counts_bytes(int kvol, int64_t n_out);
int spx_conv_wgrad_counts(const int32_t *pair, int64_t pair_ld, int kvol, int64_t n_out, const int64_t *d_n_out,
                          int32_t *counts, spx_stream_t stream);
int spx_conv_wgrad(const float *in, int cin, const float *dout, int cout, int kvol, const int32_t *pair,
                   int64_t pair_ld, int64_t n_out, const int64_t *d_n_out, const int32_t *counts, float *dw, void *ws,
                   size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 5. Densify (BEV collapse feed)
 *    replaces: spconv.pytorch.SparseConvTensor.dense(), reference call site
 *      pcdet/models/backbones_2d/map_to_bev/height_compression.py:21 (followed by the view at :22-23).
 *    layout 0: dense[b][c][z][y][x]  (contiguous NCDHW, what .dense() returns)
 *    layout 1: dense[b][y][x][c][z]  (the same logical [B,C,D,H,W] tensor stored so that
 *              view(B, C*D, H, W) is channels_last: BEV channel c*D+z is the fastest axis)
 *    The caller zero-fills `dense` (hipMemsetAsync) before spx_densify; spx_densify_bwd gathers
 *    dfeat[row,c] = ddense[...] (autograd of .dense()).
 * ---------------------------------------------------------------------------------------------- */
int spx_densify(const float *feat, const int32_t *idx, int64_t n, const int64_t *d_n, int c, int batch,
                const int32_t *shape, int layout, float *dense, spx_stream_t stream);
int spx_densify_bwd(const float *ddense, const int32_t *idx, int64_t n, const int64_t *d_n, int c, int batch,
                    const int32_t *shape, int layout, float *dfeat, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 6. Rotated-BEV IoU and NMS  (post-processing)
 *    replaces: iou3d_nms_cuda.boxes_overlap_bev_gpu / boxes_iou_bev_gpu / nms_gpu / nms_normal_gpu, reference
 *      pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:236-325, src/iou3d_nms.cpp:53-190, called from
 *      pcdet/ops/iou3d_nms/iou3d_nms_utils.py:48-118 by model_nms_utils.py:6-87.
 *    boxes are device [n,7] fp32 (x,y,z,dx,dy,dz,heading).
 *    spx_boxes_iou_bev : out[n,m] = BEV IoU (overlap_only != 0: intersection AREA) of every pair.  The IoU is at
 *                        most 1 (csrc/box_iou.h).  n * m == 0 is a no-op and `out` may then be NULL.
 *    spx_nms_bev       : boxes must already be sorted by descending score; keep[0..*d_num_keep) receives the kept
 *                        positions in ascending order (greedy: a box is kept iff no earlier kept box has IoU > thresh).
 *                        axis_aligned != 0 uses the heading-less IoU of nms_normal_gpu.  The suppression mask and its
 *                        reduction stay on the device (the reference copies the mask to the host and reduces there).
 * ---------------------------------------------------------------------------------------------- */
int spx_boxes_iou_bev(const float *boxes_a, int64_t n, const float *boxes_b, int64_t m, int overlap_only, float *out,
                      spx_stream_t stream);
size_t spx_nms_ws_bytes(int64_t n);
int spx_nms_bev(const float *boxes, int64_t n, float thresh, int axis_aligned, int64_t *keep, int64_t *d_num_keep,
                void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 7. Anchor target assignment (training)
 *    replaces: AxisAlignedTargetAssigner.assign_targets, reference
 *      pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:36-210 (per-sample / per-class python
 *      loops over torch ops), incl. boxes3d_nearest_bev_iou (pcdet/utils/box_utils.py:249-298) and
 *      ResidualCoder.encode_torch (pcdet/utils/box_coder_utils.py:13-43); SECOND settings only
 *      (POS_FRACTION < 0, NORM_BY_NUM_EXAMPLES False, MATCH_HEIGHT False, single head).
 *    anchors   device [n_sets][anchors_per_set][7], every set laid out (z=1, y, x, size, rot) as AnchorGenerator emits
 *    gt_boxes  device [batch][max_gt][8] = (x,y,z,dx,dy,dz,heading,class 1..n_classes), zero padded
 *    d_set_class device int32[n_sets]: 0-based class index each anchor set is matched against
 *    outputs in the head's anchor order (y, x, set, within-location), A_total = n_sets * anchors_per_set:
 *      labels int32 [batch][A_total] (class id / 0 background / -1 ignored), targets fp32 [batch][A_total][7],
 *      weights fp32 [batch][A_total] (1 where labels > 0)
 * ---------------------------------------------------------------------------------------------- */
size_t spx_assign_targets_ws_bytes(int batch, int n_sets, int max_gt);
int spx_assign_targets(const float *anchors, int n_sets, int64_t anchors_per_set, int per_location,
                       const float *gt_boxes, int batch, int max_gt, const int32_t *d_set_class, int n_classes,
                       const float *d_matched, const float *d_unmatched, int32_t *labels, float *targets,
                       float *weights, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 8. Anchor-head losses, forward + gradient in one pass (training)
 *    replaces: AnchorHeadTemplate.get_cls_layer_loss / get_box_reg_layer_loss and their autograd, reference
 *      pcdet/models/dense_heads/anchor_head_template.py:101-224 with the loss classes of
 *      pcdet/utils/loss_utils.py:9-77 (sigmoid focal, alpha/gamma=2), :140-209 (smooth L1, beta, unit code weights,
 *      after add_sin_difference) and :310-338 (weighted cross entropy on direction bins).
 *    cls_preds [batch][A][num_class], box_preds [batch][A][7], dir_preds [batch][A][num_dir_bins] (NULL: no direction
 *    classifier), labels int32 [batch][A], reg_targets [batch][A][7], anchors [A][7] — all device, anchor order of the head.
 *    losses  device fp32[3] = (cls, loc, dir), each already divided by batch and multiplied by its weight
 *    dcls/dbox/ddir  device, same shapes as the predictions: d(weighted loss)/d(prediction)
 * ---------------------------------------------------------------------------------------------- */
size_t spx_anchor_loss_ws_bytes(int batch, int64_t n_anchors);
int spx_anchor_loss(const float *cls_preds, const float *box_preds, const float *dir_preds, const int32_t *labels,
                    const float *reg_targets, const float *anchors, int batch, int64_t n_anchors, int num_class,
                    int num_dir_bins, float dir_offset, float cls_weight, float loc_weight, float dir_weight,
                    float beta, float alpha, float *losses, float *dcls, float *dbox, float *ddir, void *ws,
                    size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 9. BatchNorm1d (+ReLU) over sparse feature rows, training mode
 *    replaces: nn.BatchNorm1d(C, eps=1e-3, momentum=0.01) + nn.ReLU applied to SparseConvTensor.features by
 *      SparseSequential, reference pcdet/models/backbones_3d/spconv_backbone.py:81,24-33 (three torch launches forward,
 *      three backward per layer).  C must divide 1024 and be a multiple of 4.
 *    fwd: batch mean / biased variance over the n rows -> save_mean, save_invstd; running_mean/var (nullable) updated
 *         with `momentum` (unbiased variance), y = relu?((x-mean)*invstd*gamma + beta)
 *    bwd: dx, dgamma, dbeta from dy (ReLU mask taken from y when relu != 0)
 * ---------------------------------------------------------------------------------------------- */
size_t spx_bn_relu_ws_bytes(int c);
int spx_bn_relu_fwd(const float *x, int64_t n, const int64_t *d_n, int c, const float *gamma, const float *beta,
                    float *running_mean, float *running_var, float momentum, float eps, int relu, float *y,
                    float *save_mean, float *save_invstd, void *ws, size_t ws_bytes, spx_stream_t stream);
/* backward: the ReLU mask is recomputed from x (same instruction sequence as the forward), y is not needed; d_n (nullable)
 * = device-side live row count as in the forward */
int spx_bn_relu_bwd(const float *x, const float *dy, int64_t n, const int64_t *d_n, int c, const float *gamma, const float *beta,
                    const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma, float *dbeta,
                    void *ws, size_t ws_bytes, spx_stream_t stream);

/* y = relu(bn(x) + res): the tail of SparseBasicBlock (reference spconv_backbone.py:56-72: bn2, `out.features +
 * identity.features`, ReLU; SURVEY.md §8 row f-3 "fused residual add epilogue").  res [n, c] or NULL (= spx_bn_relu_*);
 * backward also writes dres [n, c] (may be NULL) = dy masked by the ReLU, the gradient of the identity branch.
 * num_batches_tracked: nn.BatchNorm's int64 counter, incremented by one inside the kernels (NULL: not touched).
 * y_ld / dy_ld: row stride in floats of y / dy (0 = c): a layer can write its output straight into a channel slice of a
 * wider [n, y_ld] matrix (the channel concatenation of the BEV up-sampling branches, reference
 * base_bev_backbone.py:99-106) and read its gradient from the same slice; multiples of 4, 16-byte aligned base. */
int spx_bn_add_relu_fwd(const float *x, const float *res, int64_t n, const int64_t *d_n, int c, const float *gamma,
                        const float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                        float momentum, float eps, int relu, float *y, int64_t y_ld, float *save_mean, float *save_invstd,
                        void *ws, size_t ws_bytes, spx_stream_t stream);
int spx_bn_add_relu_bwd(const float *x, const float *res, const float *dy, int64_t dy_ld, int64_t n, const int64_t *d_n,
                        int c, const float *gamma, const float *beta, const float *save_mean, const float *save_invstd, int relu,
                        float *dx, float *dres, float *dgamma, float *dbeta, void *ws, size_t ws_bytes,
                        spx_stream_t stream);

/* Inference-mode BatchNorm (+ residual) (+ ReLU) with GIVEN statistics, one pass: y = relu?((x - mean) * invstd * gamma + beta
 * (+ res)).  replaces: nn.BatchNorm2d (eval) + nn.ReLU of the BEV backbone, reference
 * pcdet/models/backbones_2d/base_bev_backbone.py:35-44,60-73 (two elementwise passes in torch), applied to the channels_last
 * map as [B*H*W, C] rows; y_ld as in spx_bn_add_relu_fwd (a channel slice of the concatenated map, :99-106). */
int spx_bn_apply(const float *x, const float *res, int64_t n, const int64_t *d_n, int c, const float *mean,
                 const float *invstd, const float *gamma, const float *beta, int relu, float *y, int64_t y_ld,
                 spx_stream_t stream);

/* Training-mode BatchNorm (+ReLU) from per-block sums taken by the producer of x (spx_conv2d_wino's stat_partials):
 * partial[nblk][2][c] = sums of x and x*x; finalize + apply, no statistics pass over x.  replaces: the same nn.BatchNorm2d
 * (train) + nn.ReLU as spx_bn_add_relu_fwd for the 3x3 layers of the BEV backbone, base_bev_backbone.py:38-49, and (with the
 * sums of spx_conv_gemm_ring's epilogue) the nn.BatchNorm1d + nn.ReLU of the 64-channel sparse blocks,
 * spconv_backbone.py:26-27,81.  d_n (nullable): device-side live row count of a static-capacity row matrix. */
int spx_bn_relu_fwd_from_sums(const float *x, int64_t n, const int64_t *d_n, int c, const float *partial, int64_t nblk,
                              const float *gamma,
                              const float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                              float momentum, float eps, int relu, float *y, int64_t y_ld, float *save_mean,
                              float *save_invstd, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 9b. Dense 3x3 / stride 1 / pad 1 convolution of the BEV backbone, Winograd F(2x2, 3x3) on the exact-fp32 MFMA
 *    replaces: nn.Conv2d(c, c, kernel_size=3, padding=1, bias=False) forward and its data gradient, reference
 *    pcdet/models/backbones_2d/base_bev_backbone.py:38-49 (cuDNN / MIOpen implicit GEMM: 9 multiplies per (pixel, ci, co)
 *    against 4 here).  Maps are channels-last: pixel p = (n*H + y)*W + x, channel c at x[p * x_ld + c].
 *
 * spx_wino_weight: weight element (co, ci, a, b) at w[co*s_o + ci*s_i + a*s_a + b*s_b] (strides in floats: OIHW or
 *    channels_last) -> the transformed, fragment-ordered image u (spx_wino_weight_floats(cin, cout) floats).
 *    flip = 0: forward filter, cin/cout = the layer's.  flip = 1: filter of the data gradient — pass cin = the layer's
 *    Cout and cout = the layer's Cin; taps are rotated by 180 degrees and the channel roles swapped inside.
 *    cin % 32 == 0 and cout % 128 == 0, else SPX_ERR_INVALID_ARG.
 * spx_conv2d_wino: y = conv3x3(x) with optional epilogue y = relu?(y * scale[co] + shift[co]) (eval BatchNorm folded to
 *    scale/shift; null = identity).  x_ld >= cin, y_ld >= cout, both multiples of 4; x, y 16-byte aligned.
 *    stat_partials (or null): [spx_wino_stat_rows(n, h, w)][2][cout] floats, row b = the sums of y and of y*y over the pixels
 *    of tile block b — the statistics pass of the training-mode BatchNorm that follows, taken where y is produced
 *    (spx_bn_relu_fwd_from_sums consumes them). */
int64_t spx_wino_stat_rows(int32_t n, int32_t h, int32_t w);
int64_t spx_wino_weight_floats(int32_t cin, int32_t cout);
int spx_wino_weight(const float *w, int64_t s_o, int64_t s_i, int64_t s_a, int64_t s_b, int32_t cin, int32_t cout, int flip,
                    float *u, spx_stream_t stream);
int spx_conv2d_wino(const float *x, int64_t x_ld, const float *u, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout,
                    const float *scale, const float *shift, int relu, float *y, int64_t y_ld, float *stat_partials,
                    spx_stream_t stream);

/* spx_conv2d_wino_wgrad: weight gradient of the same convolution in the Winograd domain (csrc/wino_wgrad.hip):
 *    dw[co*s_o + ci*s_i + a*s_a + b*s_b] = sum over pixels of x[.., ci] (shifted by the tap) * dy[.., co]  — the weight half
 *    of convolution_backward for the layers of 9b.  cin % 128 == 0 and cout % 128 == 0 (else SPX_ERR_INVALID_ARG), map at
 *    least 15 pixels wide (else SPX_ERR_UNSUPPORTED: callers keep the vendor kernel).  ws: spx_wino_wgrad_ws_bytes bytes
 *    (per-split partial sums, summed in a fixed order: deterministic, no atomics). */
size_t spx_wino_wgrad_ws_bytes(int32_t cin, int32_t cout);
int spx_conv2d_wino_wgrad(const float *x, int64_t x_ld, const float *dy, int64_t dy_ld, int32_t n, int32_t h, int32_t w,
                          int32_t cin, int32_t cout, float *dw, int64_t s_o, int64_t s_i, int64_t s_a, int64_t s_b, void *ws,
                          size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 10. Voxel query (consumers of multi_scale_3d_features)
 *    replaces: pointnet2_stack_cuda.voxel_query_wrapper, reference
 *      pcdet/ops/pointnet2/pointnet2_stack/src/voxel_query_gpu.cu:10-122 (python side voxel_query_utils.py:12-50).
 *      new_xyz [m,3] f32 query centres; xyz [n,3] f32 positions of the rows; new_coords [m,4] int32 (b, z, y, x);
 *      point_indices [batch, Z, Y, X] int32 = row at each cell or -1 (generate_voxel2pinds); shape3 = (Z, Y, X);
 *      range3 = (z_range, y_range, x_range) cells scanned each way; idx [m, nsample] int32 out (slot 0 = -1 for an
 *      empty ball, exactly as the reference kernel leaves it); cnt_unique [m] = occupied cells scanned.
 *    The reservoir step that applies once more than nsample neighbours lie within the radius uses cuRAND's XORWOW
 *    algorithm seeded with the query index like the reference; that stream is parity-unpinned here (csrc/voxel_query.hip).
 * ---------------------------------------------------------------------------------------------- */
int spx_voxel_query(const float *new_xyz, const float *xyz, const int32_t *new_coords, const int32_t *point_indices,
                    int64_t m, int batch, const int32_t *shape3, int nsample, float radius, const int32_t *range3,
                    int32_t *idx, int32_t *cnt_unique, spx_stream_t stream);

/* replaces: pointnet2_stack_cuda.voxel_query_dilated_wrapper, reference voxel_query_gpu.cu:125-236 (python side
 *   voxel_query_utils.py:117-158).  As spx_voxel_query, with the scan stepping by stride3 = (z, y, x) cells, neighbours
 *   closer than former_radius dropped as well, and idx_cnt [m] = number of slots filled before padding (<= nsample). */
int spx_voxel_query_dilated(const float *new_xyz, const float *xyz, const int32_t *new_coords,
                            const int32_t *point_indices, int64_t m, int batch, const int32_t *shape3, int nsample,
                            float former_radius, float radius, const int32_t *range3, const int32_t *stride3,
                            int32_t *idx, int32_t *cnt_unique, int32_t *idx_cnt, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 11. Point sampling and grouping (the fork's 3DSSD-style SA layers; csrc/pointnet2.hip)
 *    replaces: the pointnet2_batch extension, reference pcdet/ops/pointnet2/pointnet2_batch/src/ (sampling, ball_query,
 *      group_points, interpolate _gpu.cu), reached from
 *      pointnet2_utils.py and _VoxelPointnetSAModuleFSDistillationBase (pointnet2_modules.py:1140-1230, 1514-1540).
 *    All tensors fp32 / int32, contiguous, batch-major; b frames.  Distances are ((dx*dx)+(dy*dy))+(dz*dz) rounded after
 *    every operation (no FMA contraction).  Indices outside [0, N) are a caller error; the kernels skip them (forward:
 *    read as 0, backward: dropped) and never access memory out of bounds.
 * ---------------------------------------------------------------------------------------------- */

/* replaces: furthest_point_sampling_wrapper / farthest_point_sampling_wrapper (sampling_gpu.cu, python side
 *   pointnet2_utils.py:21-38, 85-111) and, with weights, furthest_point_sampling_weights_wrapper (:62-81).
 *   xyz [b, n, 3]; weights [b, n] or NULL; idx [b, npoint] out.  Unweighted: idx[0] = 0; weighted: round 0 picks the
 *   arg-max of the weights.  Later rounds: temp[k] = min(temp[k], |p_k - p_old|^2) (temp starts at 1e10), next pick =
 *   arg-max of temp[k] (weighted: of (float)((double)temp[k] * max((double)w_k, 1e-12))).  Ties resolve exactly as the
 *   reference's thread layout does (csrc/pointnet2.hip).  npoint > n is legal.  n <= 16384 runs with points and temp in
 *   registers (ws unused, ws_bytes() = 0); larger n keeps temp in ws. */
size_t spx_furthest_point_sample_ws_bytes(int32_t b, int64_t n);
int spx_furthest_point_sample(const float *xyz, const float *weights, int32_t b, int64_t n, int32_t npoint, int32_t *idx,
                              void *ws, size_t ws_bytes, spx_stream_t stream);

/* replaces: furthest_point_sampling_matrix_wrapper, furthest_point_sampling_with_dist_wrapper and (weights non-NULL)
 *   furthest_point_sampling_with_weighted_dist_wrapper (pointnet2_utils.py:42-58, 114-169).  matrix [b, n, n]: the
 *   distance of round r is matrix[old][k]; otherwise as spx_furthest_point_sample.  ws: temp, b*n floats. */
size_t spx_furthest_point_sample_matrix_ws_bytes(int32_t b, int64_t n);
int spx_furthest_point_sample_matrix(const float *matrix, const float *weights, int32_t b, int64_t n, int32_t npoint,
                                     int32_t *idx, void *ws, size_t ws_bytes, spx_stream_t stream);

/* replaces: ball_query_wrapper (r_in = 0) and ball_query_dilated_wrapper (ball_query_gpu.cu:75-198, python side
 *   pointnet2_utils.py:414-457).  xyz [b, n, 3]; new_xyz [b, m, 3] centres; hits are the k (ascending) with
 *   r_in^2 <= d2 < r_out^2, the first nsample kept; idx_cnt [b, m] = hits kept; idx [b, m, nsample]: the hits, then the
 *   hits repeated cyclically; an empty ball is all 0.  Every slot is written (no pre-zeroing needed). */
int spx_ball_query(const float *xyz, const float *new_xyz, int32_t b, int64_t n, int64_t m, float r_in, float r_out,
                   int32_t nsample, int32_t *idx_cnt, int32_t *idx, spx_stream_t stream);

/* replaces: group_points_wrapper (group_points_gpu.cu, pointnet2_utils.py:340-361) and, with nsample = 1,
 *   gather_points_wrapper (sampling_gpu.cu:15-50, pointnet2_utils.py:223-244).  features [b, c, n]; idx [b, m, nsample];
 *   out [b, c, m, nsample] = features[.., idx]. */
int spx_group_points(const float *features, const int32_t *idx, int32_t b, int32_t c, int64_t n, int64_t m,
                     int32_t nsample, float *out, spx_stream_t stream);

/* replaces: group_points_grad_wrapper / gather_points_grad_wrapper (atomicAdd there).  grad_features [b, c, n] (fully
 *   written) = sum of grad_out over the entries that point at each feature, DETERMINISTIC: sorted runs by target
 *   b * n + k, added in ascending entry order (the contract is stated once, in csrc/sorted_runs.h). */
size_t spx_group_points_bwd_ws_bytes(int32_t b, int64_t n, int64_t m, int32_t nsample);
int spx_group_points_bwd(const float *grad_out, const int32_t *idx, int32_t b, int32_t c, int64_t n, int64_t m,
                         int32_t nsample, float *grad_features, void *ws, size_t ws_bytes, spx_stream_t stream);

/* replaces: three_nn_wrapper (interpolate_gpu.cu:16-75, pointnet2_utils.py:260-289).  unknown [b, n, 3], known [b, m, 3];
 *   dist2 [b, n, 3] squared distances and idx [b, n, 3] of the three nearest known points (strict-< insertion in
 *   ascending k: the first index wins ties; m < 3 leaves inf and index 0 in the unfilled slots). */
int spx_three_nn(const float *unknown, const float *known, int32_t b, int64_t n, int64_t m, float *dist2, int32_t *idx,
                 spx_stream_t stream);

/* replaces: three_interpolate_wrapper / three_interpolate_grad_wrapper (interpolate_gpu.cu, pointnet2_utils.py:292-334).
 *   features [b, c, m]; idx, weight [b, n, 3]; out [b, c, n] = ((w0*f0) + (w1*f1)) + (w2*f2).  The backward writes all
 *   of grad_features [b, c, m], deterministically as spx_group_points_bwd does. */
int spx_three_interpolate(const float *features, const int32_t *idx, const float *weight, int32_t b, int32_t c, int64_t m,
                          int64_t n, float *out, spx_stream_t stream);
size_t spx_three_interpolate_bwd_ws_bytes(int32_t b, int64_t m, int64_t n);
int spx_three_interpolate_bwd(const float *grad_out, const int32_t *idx, const float *weight, int32_t b, int32_t c,
                              int64_t m, int64_t n, float *grad_features, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 12. Points in boxes and RoI-aware pooling (the fork's point-head target assignment, PartA2-style RoI heads;
 *     csrc/roiaware_pool3d.hip)
 *    replaces: the roiaware_pool3d extension, reference pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu, reached
 *      from roiaware_pool3d_utils.py (point_head_template.py:119-126, loss_utils.py:602-612).
 *    Boxes / RoIs are fp32 [.., 7] = (cx, cy, cz, dx, dy, dz, heading).  Inside test: |z - cz| > dz / 2 (in double)
 *    rejects (a point on a z face is inside); then with (sx, sy) = (x - cx, y - cy), cosa = (float)cos(-(double)heading)
 *    and sina likewise, local_x = (sx*cosa) + (sy*(-sina)) and local_y = (sx*sina) + (sy*cosa) in float without FMA
 *    contraction, and the point is inside iff |local_x| < (double)dx / 2.0 + (double)1e-5f and the same for y.
 * ---------------------------------------------------------------------------------------------- */

/* replaces: points_in_boxes_gpu (roiaware_pool3d_kernel.cu:290-335, python side roiaware_pool3d_utils.py:29-42).
 *   pts [b, m, 3], boxes [b, t, 7] -> box_idx [b, m] = the first k (ascending) whose box contains the point, else -1.
 *   Every element is written; t = 0 is legal (all -1).  Zero-padded boxes take part like any other box. */
int spx_points_in_boxes(const float *pts, const float *boxes, int32_t b, int64_t m, int64_t t, int32_t *box_idx,
                        spx_stream_t stream);

/* replaces: roiaware_pool3d_cuda.forward (roiaware_pool3d_kernel.cu:41-227).  rois [n, 7], pts [np, 3], feats [np, c];
 *   out size (ox, oy, oz), each in [1, 255]; max_pts >= 1 (each voxel keeps max_pts - 1 points); mode 0 = max, 1 = avg.
 *   Cell of an in-box point: x_res = dx / ox, i = (int)((local_x + dx / 2) / x_res) in float (saturating, NaN -> 0),
 *   taken as unsigned and clamped to ox - 1 (a negative index lands in the LAST cell); y, z likewise (local_z = z - cz).
 *   Each voxel keeps the first max_pts - 1 in-box points in ascending point index.  Outputs, every element written:
 *     pooled [n, ox, oy, oz, c]: max = the first maximum (strict >, from -inf) in point order, 0 when nothing beats -inf;
 *       avg = (sum in point order from 0) / count, 0 when empty;
 *     argmax [n, ox, oy, oz, c] (mode 0 only, NULL allowed for avg): point index of the maximum, -1 when none;
 *     pt_cell [n, np]: cell (x*oy + y)*oz + z of point p in RoI r when the point is kept there, else -1;
 *     vox_cnt [n, ox, oy, oz]: points kept per voxel.
 *   pt_cell and vox_cnt are the record spx_roiaware_pool3d_bwd reads.  ws: spx_roiaware_pool3d_ws_bytes bytes. */
size_t spx_roiaware_pool3d_ws_bytes(int64_t n, int64_t np, int32_t ox, int32_t oy, int32_t oz);
int spx_roiaware_pool3d_fwd(const float *rois, const float *pts, const float *feats, int64_t n, int64_t np, int32_t c,
                            int32_t ox, int32_t oy, int32_t oz, int32_t max_pts, int32_t mode, float *pooled,
                            int32_t *argmax, int32_t *pt_cell, int32_t *vox_cnt, void *ws, size_t ws_bytes,
                            spx_stream_t stream);

/* replaces: roiaware_pool3d_cuda.backward (atomicAdd there, roiaware_pool3d_kernel.cu:230-287).  grad_out
 *   [n, ox, oy, oz, c]; argmax (mode 0) / vox_cnt (mode 1) and pt_cell from the forward.  grad_in [np, c], fully written,
 *   DETERMINISTIC: grad_in[p, ch] starts at 0.0f and adds the RoIs' contributions in ASCENDING RoI order r = 0, 1, ...;
 *   RoI r contributes, for the voxel v = pt_cell[r, p] (none when -1), max: grad_out[r, v, ch] if argmax[r, v, ch] == p;
 *   avg: grad_out[r, v, ch] * (1.0f / fmaxf((float)vox_cnt[r, v], 1.0f)), a float product. */
int spx_roiaware_pool3d_bwd(const float *grad_out, const int32_t *argmax, const int32_t *pt_cell, const int32_t *vox_cnt,
                            int64_t n, int64_t np, int32_t c, int32_t ox, int32_t oy, int32_t oz, int32_t mode,
                            float *grad_in, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 13. Gather-project: a set-abstraction grouper's first 1x1 conv fused with the grouping that feeds it (the fork's
 *     voxel-point SA modules; csrc/group_project.hip)
 *    replaces: the grouped tensor (B, 3 + C, npoint, nsample) that the reference builds with grouping_operation, a
 *      centre subtraction, torch.cat, empty-ball zeroing and a permute, followed by Conv2d(k=1) (pointnet2_modules.py,
 *      _VoxelPointnetSAModuleFSDistillationBase.forward, point and voxel branches).
 *    Queries m = bi * npoint + pi; slot s; source row r = idx[m, s] (GLOBAL rows, the caller adds frame offsets).
 *    A column (m, s) is EMPTY when empty[m] != 0 (empty may be NULL: none) or r is outside [0, n_src).
 * ---------------------------------------------------------------------------------------------- */

/* p [n_src, c_out] = F · Wf^T (the feature half of the conv, per source row; NULL: no feature term), wx [c_out, 3]
 *   (NULL: no xyz term; at least one of p, wx), xyz [n_src, 3], ctr [b * npoint, 3], idx [b * npoint, nsample] int32,
 *   empty [b * npoint] bytes.  y [b, c_out, npoint, nsample] (NCHW), every element written:
 *     y[bi, o, pi, s] = empty column ? 0 : p[r, o] + ((wx[o,0]*(xyz[r,0]-ctr[m,0]) + wx[o,1]*(..1)) + wx[o,2]*(..2)).
 *   The xyz term is evaluated relative to the centre (never folded into p). */
int spx_group_project(const float *p, const float *wx, const float *xyz, const float *ctr, const int32_t *idx,
                      const uint8_t *empty, int32_t c_out, int64_t n_src, int32_t b, int64_t npoint, int32_t nsample,
                      float *y, spx_stream_t stream);

/* Backward of spx_group_project.  dy [b, c_out, npoint, nsample].  Either output may be NULL (not computed):
 *   dpt [c_out, n_src] (TRANSPOSED, fully written): dP^T[o, r] = sum of dy[.., o, ..] over the non-empty columns with
 *     idx = r, DETERMINISTIC: sorted runs by r (csrc/sorted_runs.h), added in ascending column order (dF = dP · Wf and
 *     dWf = dP^T · F are the caller's GEMMs);
 *   dwx [c_out, 3]: sum over non-empty columns of dy * (xyz[r] - ctr[m]), DETERMINISTIC: fixed-order per-block partials
 *     over chunks of 2048 columns, then a fixed-order sum of the partials.
 *   No gradient flows to xyz or ctr.  ws: spx_group_project_bwd_ws_bytes bytes. */
size_t spx_group_project_bwd_ws_bytes(int32_t c_out, int64_t n_src, int32_t b, int64_t npoint, int32_t nsample);
int spx_group_project_bwd(const float *dy, const float *xyz, const float *ctr, const int32_t *idx, const uint8_t *empty,
                          int32_t c_out, int64_t n_src, int32_t b, int64_t npoint, int32_t nsample, float *dpt,
                          float *dwx, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 14. Point head: the eval tail of the fork's fast_cpc point head (PointHeadVoteSASAStatisticDistillation, student
 *     branch; csrc/point_head.hip)
 *    replaces: s_vote_layers + clamp + add (~8 launches), and after s_shared_fc_layer the per-class statistic-modulated
 *      s_cls_block, s_reg_layers, permutes and the PointBinResidualCoder decode (~40 launches).
 *    One workgroup owns a tile of 32 points; both 1x1-conv layers and the decode run from LDS in one launch, on the
 *    VALU.  Inference only: no gradient is computed and the outputs carry no autograd history.
 * ---------------------------------------------------------------------------------------------- */

/* One Conv1d(k=1, no bias) -> BatchNorm1d (eval affine) -> ReLU -> Conv1d(k=1, bias) stack, as DEVICE pointers to the
 * module's own tensors (read at the call, passed to the kernel by value; nothing is folded or cached):
 *   w1 [hidden, c_in]; bn_mean, bn_var, bn_weight, bn_bias [hidden]; bn_eps; w2 [c_out, hidden]; b2 [c_out].
 *   hidden = ReLU((w1 . x - bn_mean) / sqrt(bn_var + bn_eps) * bn_weight + bn_bias), y = w2 . hidden + b2. */
typedef struct spx_point_mlp {
  const float *w1;
  const float *bn_mean;
  const float *bn_var;
  const float *bn_weight;
  const float *bn_bias;
  float bn_eps;
  const float *w2;
  const float *b2;
} spx_point_mlp;

/* feat [b, c_in, n] (NCW), xyz [b, n, 3]; the candidates are the columns [lo, hi).  mlp: c_in -> hidden -> 3 (host
 *   pointer to one descriptor), range: HOST float[3].  vote [b, hi - lo, 3], every element written:
 *     vote = xyz[., lo + i] + min(max(offset, -range), range), NaN offsets propagating (torch.max / torch.min).
 *   c_in <= 256 and hidden <= 128, else SPX_ERR_UNSUPPORTED. */
int spx_point_vote(const float *feat, const float *xyz, int32_t b, int32_t c_in, int64_t n, int64_t lo, int64_t hi,
                   const spx_point_mlp *mlp, int32_t hidden, const float *range, float *vote, spx_stream_t stream);

/* feat [b, c, n] (after the shared FC), stat [num_class, c] (the teacher's object_statistic_features), vote_xyz
 *   [b * n, 3]; cls: HOST array of num_class descriptors (c -> cls_hidden -> 1, applied to feat * stat[k]); reg: one
 *   descriptor (c -> reg_hidden -> 6 + 2 * bins).  Points m = bi * n + i.  Every element written:
 *     cls_out [b * n, num_class] logits; reg_out [b * n, 6 + 2 * bins] raw regression;
 *     box_out [b * n, 7] = PointBinResidualCoder decode with use_mean_size False: xyz = reg[0:3] + vote_xyz,
 *       sizes = expf(reg[3:6]), angle = ((float)bin + reg[6 + bins + bin]) * (float)(2 pi / bins) with bin the FIRST
 *       maximum of reg[6 : 6 + bins] (torch.argmax: NaN counts as the maximum).
 *   c <= 256, num_class <= 8, hidden widths <= 128, bins <= 32, else SPX_ERR_UNSUPPORTED. */
int spx_point_head_predict(const float *feat, const float *stat, const float *vote_xyz, int32_t b, int32_t c, int64_t n,
                           int32_t num_class, const spx_point_mlp *cls, int32_t cls_hidden, const spx_point_mlp *reg,
                           int32_t reg_hidden, int32_t bins, float *cls_out, float *reg_out, float *box_out,
                           spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 15. Point-head post-processing without a host read (csrc/post_process.hip)
 *    replaces: the per-frame, per-class mask / nonzero / topk / gather / NMS / count read of
 *      Detector3DTemplate.post_processing with model_nms_utils.multi_thresh (fork) or class_agnostic_nms (upstream),
 *      reference detector3d_template.py:207-349, and generate_recall_record (:501-542).
 *    Two launches for the whole batch (one workgroup per frame and class, then one per frame), static capacity, the
 *    live count stays on the device.  The pair test is the one of spx_nms_bev (csrc/box_iou.h).
 * ---------------------------------------------------------------------------------------------- */

/* Rows of the outputs per frame: min(n, n_thresh * post_max) per class, min(n, post_max) agnostic. */
int64_t spx_point_post_process_capacity(int64_t n, int32_t n_thresh, int64_t post_max, int per_class);
size_t spx_point_post_process_ws_bytes(int32_t b, int64_t n, int32_t n_thresh, int64_t post_max);

/* scores [b * n] (already normalised), labels [b * n] int32 (1-based), boxes [b * n, 7]; frame f owns the rows
 *   [f * n, (f + 1) * n).  thresholds: HOST float[n_thresh].  n <= 4096 else SPX_ERR_TOO_LARGE; n_thresh <= 8 else
 *   SPX_ERR_UNSUPPORTED; pre_max, post_max >= 1.
 * per_class != 0 (fork, n_thresh = number of classes), per frame, class c ascending:
 *     members = rows with label == c + 1 and score >= thresholds[c], ordered by score descending, EQUAL SCORES LOWER ROW
 *     FIRST; the first pre_max; greedy NMS (box j goes iff an earlier kept box i has iou(i, j) > nms_thresh; rotated BEV
 *     IoU, or the axis-aligned one when axis_aligned != 0); the first post_max.  The classes' survivors together are
 *     ordered again by the same rule and reduced by one more greedy NMS, with no limit.
 * per_class == 0 (upstream, n_thresh = 1): score >= thresholds[0], order, pre_max, NMS, post_max.
 * Outputs, K = the capacity above, EVERY element written on every call:
 *     sel [b, K] int64 row in [0, b * n), -1 past the frame's count; count [b] int32;
 *     out_boxes [b, K, 7], out_scores [b, K], out_labels [b, K] int64: the selected rows' values, 0 past the count.
 * ws: spx_point_post_process_ws_bytes bytes. */
int spx_point_post_process(const float *scores, const int32_t *labels, const float *boxes, int32_t b, int64_t n,
                           const float *thresholds, int32_t n_thresh, float nms_thresh, int64_t pre_max, int64_t post_max,
                           int axis_aligned, int per_class, int64_t *sel, int32_t *count, float *out_boxes,
                           float *out_scores, int64_t *out_labels, void *ws, size_t ws_bytes, spx_stream_t stream);

/* Recall record of the kept boxes (generate_recall_record, rcnn_* and gt): out_boxes [b, cap, 7] and count [b] as
 *   written above, gt_boxes [b, g, gt_ld] (gt_ld >= 7, the first 7 columns are the box), thresholds: HOST
 *   float[n_thresh], n_thresh <= 8.  The live gt rows of a frame are [0, k], k found by stepping back from row g - 1
 *   while k > 0 and the row (all gt_ld columns, added in column order in fp32) sums to 0; a row of non-zero entries
 *   that cancel to exactly 0 in one summation order and not in another may be counted differently from torch's sum.  recalled [b, n_thresh] int32 = live gt rows whose largest
 *   3-D IoU (BEV overlap x height overlap / max(vol_a + vol_b - overlap, 1e-6)) over the frame's first count boxes is
 *   > threshold, 0 with no kept box; num_gt [b] int32 = k + 1 (0 when g = 0). */
int spx_recall_count(const float *out_boxes, const int32_t *count, int32_t b, int64_t cap, const float *gt_boxes, int64_t g,
                     int32_t gt_ld, const float *thresholds, int32_t n_thresh, int32_t *recalled, int32_t *num_gt,
                     spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 16. Point-head target assignment without a host read (csrc/point_targets.hip)
 *    replaces: the per-frame loops of the fork's point head and SASA loss (assign_stack_targets_mask,
 *      assign_stack_targets_simple, PointSASALoss.assign_target, generate_centerness_label): points_in_boxes_gpu once
 *      or twice per frame, boolean-mask indexing with its count reads, PointBinResidualCoder.encode_torch on the
 *      compacted rows and a scatter back.
 *    One launch for the whole batch, outputs of the static shape b * n, deterministic (no atomics).
 * ---------------------------------------------------------------------------------------------- */

/* points [b, n, 3]; gt_boxes [b, m, ld], ld >= 8, columns [x, y, z, dx, dy, dz, rz, class, ...] (zero-padded rows are
 *   scanned like any other box; may be NULL when m == 0); extra_width: HOST float[3], added to (dx, dy, dz) in float to
 *   make the enlarged boxes.  The inside test is the one of spx_points_in_boxes.
 * mode 0 (plain): hit = the first enlarged box holding the point; label = class(hit), 0 without a hit.
 * mode 1 (ignore ring): hit = the first gt box holding the point; label = class(hit); without a hit -1 when some
 *   enlarged box holds the point, else 0.
 * mode 2 (ball): hit = the first gt box holding the point; label = class(hit) when ||centre(hit) - point|| <
 *   central_radius (float, strict), else -1; 0 without a hit.
 * class(k) = 1 when num_class == 1, else (int64)gt_boxes[k][7].  A point is foreground when its label is > 0.
 * angle_bin_num 0: no regression code; 1..32, else SPX_ERR_UNSUPPORTED; mode outside 0..2: SPX_ERR_UNSUPPORTED.
 * Outputs, rows r = frame * n + point, EVERY element written; the float outputs may be NULL (skipped):
 *   cls_labels [b * n] int64; box_idx [b * n] int32 = hit or -1;
 *   box_labels [b * n, 7] = the hit's box as stored (not enlarged), center_labels [b * n, 3] = its xyz,
 *   reg_labels [b * n, 6 + 2 * angle_bin_num] = PointBinResidualCoder.encode_torch (use_mean_size False) of the hit's
 *     box against the point as torch evaluates it on the CPU in float, centerness [b * n] =
 *     generate_centerness_label with the point as point_base: all zero for points that are not foreground. */
int spx_point_assign_targets(const float *points, const float *gt_boxes, int32_t b, int64_t n, int64_t m, int32_t ld,
                             const float *extra_width, int32_t mode, float central_radius, int32_t num_class,
                             int32_t angle_bin_num, int64_t *cls_labels, int32_t *box_idx, float *box_labels,
                             float *center_labels, float *reg_labels, float *centerness, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 17. Point-head losses, forward + gradient in one pass, without a host read (csrc/point_loss.hip)
 *    replaces: PointHeadVoteSASAStatisticDistillation.get_vote_layer_loss / get_cls_layer_loss / get_box_layer_loss with
 *      generate_centerness_label, get_rdiou and get_corner_loss_lidar, normalised as get_loss does, and their autograd
 *      (reference pcdet/models/dense_heads/point_head_vote_sasa_statistic_distillation.py:570-1011, with
 *      WeightedSmoothL1Loss without code weights and WeightedBinaryCrossEntropyLoss, pcdet/utils/loss_utils.py:141-203,
 *      339-362), and PointSASALoss.loss_forward (loss_utils.py:706-753).
 *    Three launches per call (normaliser counts, one thread per row with a partial sum per block, a fixed-order sum of
 *    the partials); no float atomics, so the results are bitwise reproducible; a batch without positives takes the same
 *    path.  Where the reference takes min / max of equal operands the first one gets the gradient (torch halves it).
 * ---------------------------------------------------------------------------------------------- */

/* Rows r = frame * n_per_frame + point, n rows in all; all device fp32 unless noted.
 *   student (the gradients are w.r.t. these): vote_coords [n, 3], cls_preds [n, C] logits, reg_preds [n, 6 + 2K],
 *     box_preds [n, 7]; teacher, constants: t_cls_preds [n, C], t_reg_preds [n, 6 + 2K] (columns 0..5 are read),
 *     t_box_preds [n, 7]; targets: vote_cls_labels [n] int64 (> 0: vote positive), vote_reg_labels [n, 3],
 *     cls_labels [n] int64 (> 0 foreground = class, 0 background, -1 ignored), reg_labels [n, 6 + 2K] (PointBinResidualCoder
 *     code, use_mean_size False), box_labels [n, 7].  C = num_class <= 8, K = angle_bin_num <= 32, else
 *     SPX_ERR_UNSUPPORTED.
 *   params: HOST float[11] = LOSS_WEIGHTS (vote_reg, point_cls, point_offset_reg, point_angle_cls, point_angle_reg,
 *     point_similarity (not read), point_iou, point_corner), smooth-L1 beta (< 1e-5: L1), centerness_min, centerness_max.
 *   with_centerness: the cls target of a positive's class column is cmin + (cmax - cmin) * (centerness * rdiou + 1e-8)^(1/4)
 *     (centerness of vote_coords in box_labels, no gradient; rdiou of box_preds against box_labels, WITH gradient into
 *     box_preds), else 1.  rdiou / corner: RDIOU_REGRESS_REGULARIZATION / CORNER_LOSS_REGULARIZATION.
 *   vote = w * sum over vote positives of smoothL1(vote_coords - vote_reg_labels) / max(#vote positives, 1)
 *   cls  = w * sum over rows with label >= 0 of mean_c [0.5 BCE(x, target) + 0.5 BCE(x / 3, sigmoid(t / 3))]
 *          / max(#label >= 0, 1)
 *   box  = sum over positives of [w_off * (0.5 smoothL1(reg - label) + 0.5 smoothL1(reg - teacher)) over columns 0..5
 *          + w_acls * CE(bin logits, first maximum of the label's bin columns) + w_areg * smoothL1 of the label-weighted
 *          residual sums + w_iou * (0.5 (1 - q(box_labels)) + 0.5 (1 - q(t_box_preds))), q(b) = (rdiou(box_preds, b) *
 *          centerness(vote_coords, b) + 1e-8)^(1/4) + w_corner * (0.3 corner(box_preds, box_labels) + 0.7
 *          corner(box_preds, t_box_preds))] / max(#positives, 1); NaN targets of a smooth L1 count as the input.
 *   The counts are taken over all n rows.
 * Outputs: losses [3] = (vote, cls, box); d_vote [n, 3], d_cls [n, C], d_reg [n, 6 + 2K], d_box [n, 7] =
 *   d(vote + cls + box)/d(input), EVERY element written: exact zeros on rows that are not vote positives (d_vote),
 *   ignored rows (d_cls) and rows that are not positives (d_reg, d_box).  n == 0: nothing is written.
 * ws: spx_point_head_loss_ws_bytes(n) bytes. */
size_t spx_point_head_loss_ws_bytes(int64_t n);
int spx_point_head_loss(const float *vote_coords, const float *cls_preds, const float *reg_preds, const float *box_preds,
                        const float *t_cls_preds, const float *t_reg_preds, const float *t_box_preds,
                        const int64_t *vote_cls_labels, const float *vote_reg_labels, const int64_t *cls_labels,
                        const float *reg_labels, const float *box_labels, int64_t n, int32_t num_class,
                        int32_t angle_bin_num, const float *params, int with_centerness, int rdiou, int corner,
                        float *losses, float *d_vote, float *d_cls, float *d_reg, float *d_box, void *ws, size_t ws_bytes,
                        spx_stream_t stream);

/* One layer of PointSASALoss.loss_forward: scores [n, score_cols] logits, score_cols = 1 or num_class (<= 8, else
 *   SPX_ERR_UNSUPPORTED); labels [n] int64 (> 0 the class, 0 background, -1 ignored).  The target of column c is
 *   (label == c + 1); a one-column score meets every one of the num_class target columns.  func 0: BCE with logits, mean
 *   over the num_class columns; func 1: sigmoid focal loss, alpha 0.25, gamma 2, summed over them.
 * loss [1] = layer_weight * sum over rows with label >= 0 / max(#label >= 0, 1); d_scores [n, score_cols] = its
 *   gradient, EVERY element written (exact zeros on ignored rows).  ws: spx_point_seg_loss_ws_bytes(n) bytes. */
size_t spx_point_seg_loss_ws_bytes(int64_t n);
int spx_point_seg_loss(const float *scores, const int64_t *labels, int64_t n, int32_t score_cols, int32_t num_class,
                       int32_t func, float layer_weight, float *loss, float *d_scores, void *ws, size_t ws_bytes,
                       spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 18. Stacked (ragged-batch) point ops (PV-RCNN-style set abstraction over (N1 + N2 + ..., C) tensors;
 *     csrc/pointnet2_stack.hip)
 *    replaces: the rest of the pointnet2_stack extension (§10 holds its voxel query), reference
 *      pcdet/ops/pointnet2/pointnet2_stack/src/ (ball_query, group_points, sampling, interpolate _gpu.cu), reached from
 *      pointnet2_utils.py, pointnet2_modules.py and voxel_pool_modules.py.
 *    All tensors fp32 / int32, contiguous, row-major; b frames, 1 <= b <= 256 (more: SPX_ERR_UNSUPPORTED).  Every
 *    *_batch_cnt is an int32 DEVICE array of b counts that no call reads on the host: the row counts (n_rows, m_rows)
 *    are the tensors' shapes, frame starts are exclusive prefix sums taken on the device (negative counts count as 0, sums
 *    are clamped to the row count).  Rows past the sum of the counts are DEAD (static capacity for graph capture): a dead
 *    query row gets the fill stated below, a dead output row is 0, a dead source row is never read and gets a zero
 *    gradient.  No kernel reads or writes outside the given row counts, whatever the indices or counts hold: a bad index
 *    reads as 0 in a forward pass and is dropped in a backward pass (the §11 convention).  Distances are
 *    ((dx*dx)+(dy*dy))+(dz*dz), dx = a - b, rounded after every operation (no FMA contraction).
 * ---------------------------------------------------------------------------------------------- */

/* replaces: ball_query_wrapper (ball_query_gpu.cu:16-66) and the empty-ball fix-up of BallQuery.forward
 *   (pointnet2_utils.py:8-38).  xyz [n_rows, 3]; new_xyz [m_rows, 3] centres.  The hits of a query are the frame-local
 *   k (ascending) of its frame's points with d2 < radius*radius (the product in fp32); the first nsample are kept and
 *   the unfilled slots hold the FIRST hit.  idx [m_rows, nsample]; empty [m_rows] bytes: 1 for a ball without a hit,
 *   whose idx is all 0.  Dead rows: idx 0, empty 1.  Every slot is written.  One thread per query; a workgroup's
 *   queries lie in one frame (device-side map of workgroups to (frame, tile) pairs) and share its points through LDS. */
int spx_stack_ball_query(const float *xyz, const int32_t *xyz_batch_cnt, const float *new_xyz,
                         const int32_t *new_xyz_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows, float radius,
                         int32_t nsample, int32_t *idx, uint8_t *empty, spx_stream_t stream);

/* replaces: group_points_wrapper (group_points_gpu.cu, pointnet2_utils.py:48-82).  features [n_rows, c]; idx
 *   [m_rows, nsample] frame-local rows; out [m_rows, c, nsample] = features[start(frame of m) + idx[m, s], c]; an index
 *   outside its frame reads as 0; dead rows are 0. */
int spx_stack_group_points(const float *features, const int32_t *features_batch_cnt, const int32_t *idx,
                           const int32_t *idx_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows, int32_t c,
                           int32_t nsample, float *out, spx_stream_t stream);

/* replaces: group_points_grad_wrapper (atomicAdd there).  grad_out [m_rows, c, nsample] -> grad_features [n_rows, c],
 *   every element written, DETERMINISTIC and without float atomics: sorted runs by global target row
 *   (csrc/sorted_runs.h), each run added in ascending entry order in pieces of at most 128 sorted positions, and the
 *   pieces of a run that crosses such a border added in ascending order afterwards. */
size_t spx_stack_group_points_bwd_ws_bytes(int64_t n_rows, int64_t m_rows, int32_t c, int32_t nsample);
int spx_stack_group_points_bwd(const float *grad_out, const int32_t *features_batch_cnt, const int32_t *idx,
                               const int32_t *idx_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows, int32_t c,
                               int32_t nsample, float *grad_features, void *ws, size_t ws_bytes, spx_stream_t stream);

/* replaces: three_nn_wrapper (interpolate_gpu.cu, pointnet2_utils.py:224-257).  unknown [n_rows, 3], known [m_rows, 3];
 *   dist2 [n_rows, 3] squared distances and idx [n_rows, 3] GLOBAL known rows (frame start + k) of the three nearest
 *   known points of the same frame (strict-< insertion in ascending k).  Unfilled slots (a frame with fewer than 3 known
 *   points) hold inf and the frame start; dead rows hold inf and 0. */
int spx_stack_three_nn(const float *unknown, const int32_t *unknown_batch_cnt, const float *known,
                       const int32_t *known_batch_cnt, int32_t b, int64_t n_rows, int64_t m_rows, float *dist2,
                       int32_t *idx, spx_stream_t stream);

/* replaces: three_interpolate_wrapper / three_interpolate_grad_wrapper (interpolate_gpu.cu, pointnet2_utils.py:260-299).
 *   features [m_rows, c]; idx (global rows), weight [n_rows, 3]; out [n_rows, c] = ((w0*f0) + (w1*f1)) + (w2*f2).
 *   batch_cnt [b]: the counts of the n side, or NULL (b ignored): every row is live.  Dead rows are 0 (their weights,
 *   0 / 0 from the infinite distances, are not read).  The backward writes all of grad_features [m_rows, c],
 *   deterministically as spx_stack_group_points_bwd does, the products grad_out * weight being the contributions. */
int spx_stack_three_interpolate(const float *features, const int32_t *idx, const float *weight, const int32_t *batch_cnt,
                                int32_t b, int64_t m_rows, int64_t n_rows, int32_t c, float *out, spx_stream_t stream);
size_t spx_stack_three_interpolate_bwd_ws_bytes(int64_t m_rows, int64_t n_rows, int32_t c);
int spx_stack_three_interpolate_bwd(const float *grad_out, const int32_t *idx, const float *weight,
                                    const int32_t *batch_cnt, int32_t b, int64_t m_rows, int64_t n_rows, int32_t c,
                                    float *grad_features, void *ws, size_t ws_bytes, spx_stream_t stream);

/* replaces: stack_farthest_point_sampling_wrapper (sampling_gpu.cu:187-349, pointnet2_utils.py:187-221).  xyz
 *   [n_rows, 3]; npoint [b] DEVICE int32 picks per frame; idx [out_rows] GLOBAL rows, frame f writing npoint[f] picks at
 *   the prefix sum of npoint (clamped to out_rows; the caller sizes out_rows to the sum).  The first pick of a frame is
 *   its first row; later picks as spx_furthest_point_sample, unweighted, with the tie priority of the reference's fixed
 *   1024 threads: (bitrev10(k mod 1024), k div 1024), whatever the frame's size.  npoint above the frame's size is
 *   legal; a frame without points picks its frame start every time and reads nothing.  Frames of up to 16384 points run
 *   from registers; ws (n_rows floats) is needed only when n_rows is larger. */
size_t spx_stack_furthest_point_sample_ws_bytes(int64_t n_rows);
int spx_stack_furthest_point_sample(const float *xyz, const int32_t *xyz_batch_cnt, const int32_t *npoint, int32_t b,
                                    int64_t n_rows, int64_t out_rows, int32_t *idx, void *ws, size_t ws_bytes,
                                    spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 19. Voxel rows at static capacity (csrc/voxel_rows.hip)
 *    replaces: generate_voxel2pinds (reference pcdet/utils/common_utils.py:257-265) for a sparse tensor whose live row
 *      count is on the device, and the aggregation chain of the voxel-point SA modules' sparse update
 *      (_unet_update, reference pointnet2_modules.py: get_voxel_indices -> get_centroid_per_voxel ->
 *      get_nonempty_voxel_feature_indices -> masked assignment; two host reads there).
 *    No host read, no atomics on data, bitwise reproducible.  Arguments are checked on the host before any launch.
 * ---------------------------------------------------------------------------------------------- */

/* indices [cap, 4] (b, z, y, x); d_n: live rows (NULL = all cap rows); table [batch, Z, Y, X] int32, shape3 = (Z, Y, X):
 *   -1 everywhere, then table[cell of row r] = r for every LIVE row r.  Rows at or beyond the live count are never read.
 *   A live row outside the table is skipped and d_status (nullable, see spx_read_status) receives SPX_ERR_OUT_OF_GRID.
 *   Two launches (fill, scatter).  cap >= 2^31 or batch * Z * Y * X >= 2^40: SPX_ERR_TOO_LARGE. */
int spx_voxel_table_build(const int32_t *indices, int64_t cap, const int64_t *d_n, int32_t batch, const int32_t *shape3,
                          int32_t *table, int32_t *d_status, spx_stream_t stream);

/* new_xyz [batch, m, 3]; feats [batch, c, m] (channels first, read in place); table / shape3 as above; range_lo3,
 *   voxel_size3: HOST float[3] (x, y, z).  A point's cell is trunc((p - lo) / vs) per axis, in fp32 with a correctly
 *   rounded division; a point outside the grid is dropped.  For every distinct cell among a frame's m points the mean
 *   of each feature column over the cell's points — the sum from 0 in ascending point order, times 1 / count, the
 *   rounded operations of spx_dynamic_voxelize — goes to out[table[cell]] when that entry is a live row.  out [cap, c]:
 *   every other row below the live count (d_n_rows, NULL = cap) is 0; rows at or beyond it are not written.
 *   Two launches.  m <= 4096 (a frame's cell keys sit in LDS) and Z * Y * X < 2^31, else SPX_ERR_TOO_LARGE.
 *   ws: spx_voxel_rows_mean_ws_bytes bytes. */
size_t spx_voxel_rows_mean_ws_bytes(int32_t batch, int64_t m);
int spx_voxel_rows_mean(const float *new_xyz, const float *feats, int32_t batch, int32_t c, int64_t m,
                        const int32_t *table, const int32_t *shape3, const float *range_lo3, const float *voxel_size3,
                        const int64_t *d_n_rows, int64_t cap, float *out, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 20. Centre-head target assignment without a host read (csrc/center_targets.hip)
 *    replaces: CenterHead.assign_targets / assign_target_of_single_head (reference
 *      pcdet/models/dense_heads/center_head.py:103-219) with gaussian_radius and draw_gaussian_to_heatmap
 *      (pcdet/models/model_utils/centernet_utils.py:9-69): a Python loop over heads x frames x boxes with a copy of every
 *      frame's boxes to the host, radius[k].item() per box and a numpy Gaussian per box.
 *    Two launches for the whole batch and every head, on the given stream; EVERY output element is written, each by one
 *    thread, and overlapping Gaussians combine by max: no atomics, bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */

/* gt_boxes [b, m, ld], ld >= 8, columns [x, y, z, dx, dy, dz, rz, (extra ...), class]; the class is the LAST column,
 *   1-based over the detector's classes, 0 on padding rows (may be NULL when m == 0).  gt_boxes is never written.
 * class_to_head_slot: DEVICE int32 [num_class + 1, 2] = (head, 1-based class within the head) of a global class id, -1
 *   for a class no head owns; (int)class outside 1..num_class owns nothing.  head_channels: HOST int32 [n_heads], the
 *   classes of each head; n_heads <= 16 else SPX_ERR_UNSUPPORTED.  range_lo2, voxel_size2: HOST float[2] (x, y).
 * Slot k of (head, frame) = the k-th of the frame's boxes owned by the head, in input order; boxes at k >= num_max_objs
 *   are dropped.  coord = ((x - lo) / vs) / stride in float, rounded after every operation, clamped to [0, w - 0.5] and
 *   [0, h - 0.5]; cell = (int)coord.  radius = max((int)gaussian_radius((dx / vs0) / stride, (dy / vs1) / stride,
 *   gaussian_overlap), min_radius) in float in the reference's operation order, sqrt correctly rounded.  A slot whose
 *   scaled dx or dy is not > 0 keeps its place with mask 0 and zeros and draws nothing.
 * Outputs, head after head in one buffer each (c_j = head_channels[j], off_j = c_0 + ... + c_(j-1), K = num_max_objs):
 *   heatmaps: head j at b * h * w * off_j floats, [b, c_j, h, w]: the maximum over the live slots of the (frame, head)
 *     with class channel c of exp(-(ddx^2 + ddy^2) / (2 s^2)), s = (2 r + 1) / 6, inside the window |ddx|, |ddy| <= r
 *     around the cell, evaluated in double and rounded once (the centre is exactly 1), 0 elsewhere;
 *   target_boxes [n_heads, b, K, ld] = [coord - cell (2), z, logf(dx, dy, dz), cosf(rz), sinf(rz), columns 7 .. ld - 2];
 *   inds [n_heads, b, K] int64 = cell_y * w + cell_x; masks [n_heads, b, K] int64 = 1 on live slots; zeros elsewhere.
 * ws: spx_center_assign_targets_ws_bytes bytes. */
size_t spx_center_assign_targets_ws_bytes(int32_t b, int32_t n_heads, int64_t num_max_objs);
int spx_center_assign_targets(const float *gt_boxes, int32_t b, int64_t m, int32_t ld, const int32_t *class_to_head_slot,
                              int32_t num_class, int32_t n_heads, const int32_t *head_channels, const float *range_lo2,
                              const float *voxel_size2, float feature_map_stride, int32_t w, int32_t h,
                              int64_t num_max_objs, double gaussian_overlap, int32_t min_radius, float *heatmaps,
                              float *target_boxes, int64_t *inds, int64_t *masks, void *ws, size_t ws_bytes,
                              spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 21. Centre-head box decoding without a host read (csrc/center_decode.hip)
 *    replaces, for one head and the whole batch: the sigmoid / exp over full maps, _topk (torch.topk per class, then
 *      over C x K), the six _transpose_and_gather_feat passes and the masks of decode_bbox_from_heatmap (reference
 *      pcdet/models/model_utils/centernet_utils.py:118-216, called from center_head.py:288-321).
 *    1 launch when c h w <= 8192, 2 when ceil(c h w / 8192) <= floor(8192 / k) (both yamls), one more per further
 *    factor floor(8192 / k).  No float atomics; bit-identical from call to call for every input bit pattern.
 * ---------------------------------------------------------------------------------------------- */

/* Inputs, fp32 NCHW on the device: hm [b, c, h, w], center [b, 2, h, w], center_z [b, 1, h, w], dim [b, 3, h, w],
 *   rot [b, 2, h, w] (cos in channel 0, sin in channel 1), vel [b, 2, h, w] or NULL.  voxel_size2, range_lo2: HOST
 *   float[2] (x, y); post_center_limit_range6: HOST float[6].
 * Selection: per frame the k largest of the c h w values of hm AS GIVEN, by float value descending (-0 equals +0), equal
 *   values lower flat index ci h w + y w + x first; output row j of a frame is the j-th of that order.  Which cells a
 *   NaN selects is unspecified; every gather index is in range whatever hm holds.
 * Decode of a selected cell, fp32, no contraction: xs = ((x + center_x) * stride) * voxel_size2[0] + range_lo2[0], ys
 *   likewise; z and vel copied; dims = expf(dim) if raw else dim; angle = atan2f(sin, cos); score = 1 / (1 + expf(-v))
 *   if raw else v.  keep = xs, ys, z >= limit[0:3] and <= limit[3:6] (inclusive), and score > score_thresh (strict) when
 *   has_score_thresh.  raw == 0 is decode_bbox_from_heatmap itself; raw != 0 takes the head's logits and log sizes.
 * Outputs, every element written on every call: boxes [b, k, 7 (9 with vel)], scores [b, k], labels [b, k] int32
 *   (0-based channel), cells [b, k] int64 (y w + x), keep [b, k] uint8, count [b] int32 (rows kept).  Rows that are not
 *   kept hold their decoded values.
 * 1 <= k <= h w else SPX_ERR_INVALID_ARG; k > 1024, c h w >= 2^31 or b > 65535: SPX_ERR_TOO_LARGE.
 * ws: spx_center_decode_ws_bytes bytes. */
size_t spx_center_decode_ws_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t k);
int spx_center_decode(const float *hm, const float *center, const float *center_z, const float *dim, const float *rot,
                      const float *vel, int32_t b, int32_t c, int32_t h, int32_t w, int32_t k, float feature_map_stride,
                      const float *voxel_size2, const float *range_lo2, const float *post_center_limit_range6,
                      float score_thresh, int has_score_thresh, int raw, float *boxes, float *scores, int32_t *labels,
                      int64_t *cells, uint8_t *keep, int32_t *count, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 22. Centre-head losses, forward + gradient, without a host read (csrc/center_loss.hip)
 *    replaces, for one head and the whole batch: CenterHead.get_loss's sigmoid / clamp / neg_loss_cornernet, the cat
 *      of the regression maps, _transpose_and_gather_feat and _reg_loss with the code and loss weights, and their
 *      autograd (reference pcdet/utils/loss_utils.py:420-542, pcdet/models/dense_heads/center_head.py:221-251): some
 *      fifty launches forward and as many backward, the gather's backward an index-add with float atomics.
 *    Three launches per call (positive count + zero-fill of the regression gradients; the focal stream and the
 *    regression slots with one double partial per block; a fixed-order sum of the partials).  No float atomics: the
 *    outputs are bitwise reproducible.  The normalisers are counted on the device BEFORE the gradients are stored, so
 *    the stored gradients are final; a batch without positives or without live slots takes the same path.
 * ---------------------------------------------------------------------------------------------- */

/* Inputs, device fp32 unless noted: hm [b, c, h, w] heatmap LOGITS; heatmap [b, c, h, w] the target, values in [0, 1],
 *   1 exactly at the live centres; regs: HOST array of n_regs device pointers, map i [b, reg_channels[i], h, w]
 *   (reg_channels: HOST int32[n_regs]), in HEAD_ORDER; D = sum of reg_channels; n_regs <= 5, D <= 10 and k <= 2048, else
 *   SPX_ERR_UNSUPPORTED.  target_boxes [b, k, D], inds [b, k] int64 (y w + x), masks [b, k] int64 (1 live, 0 dead); all
 *   three may be NULL when k == 0.  code_weights: HOST float[D].
 * Focal term: p = clamp(sigmoid(x), 1e-4, 1 - 1e-4); a cell with heatmap == 1 adds log(p) (1 - p)^2, every other cell
 *   log(1 - p) p^2 (1 - heatmap)^4; num_pos = #(heatmap == 1) over the batch; hm_loss = -(sum) / max(num_pos, 1) (with
 *   num_pos == 0 the positive sum is empty: the reference's -neg_loss branch, selected on the device).
 *   d_hm = d(hm_loss * cls_weight) / d(hm): exactly 0 where sigmoid(x) lies outside the clamp, passing AT a bound.
 * Regression term: per live slot and column |regs[b, d, inds[b, k]] - target_boxes[b, k, d]|, summed per column and
 *   divided by num = max(#(masks == 1) over the batch, 1).  d_regs = d(loc_loss * loc_weight) / d(regs): sign(pred -
 *   target) * code_weights[d] * loc_weight / num at the live cells, sign(0) = 0, exact zeros everywhere else.  Several
 *   live slots of a frame on one cell: the lowest slot writes the sum of their contributions, added in slot order.
 *   A dead slot is never dereferenced: its inds and target_boxes influence nothing.  A live slot whose index lies
 *   outside [0, h w) is skipped (it still counts in num).  A NaN target in a live slot makes its column of reg_loss (and
 *   losses[1]) NaN; the gradient of that element is unspecified.
 * Outputs, EVERY element written by the call's own launches: losses [2] = (hm_loss * cls_weight, sum_d(reg_loss[d] *
 *   code_weights[d]) * loc_weight); reg_loss [D], unweighted; d_hm [b, c, h, w]; d_regs: HOST array of n_regs device
 *   pointers, shaped like regs.  b == 0: SPX_OK, nothing launched, nothing written.  k == 0: the regression outputs are
 *   zeros.  Any map with 2^31 or more elements: SPX_ERR_TOO_LARGE.
 * ws: spx_center_head_loss_ws_bytes bytes. */
size_t spx_center_head_loss_ws_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int64_t k);
int spx_center_head_loss(const float *hm, const float *heatmap, const float *const *regs, const int32_t *reg_channels,
                         int32_t n_regs, const float *target_boxes, const int64_t *inds, const int64_t *masks, int32_t b,
                         int32_t c, int32_t h, int32_t w, int64_t k, const float *code_weights, float cls_weight,
                         float loc_weight, float *losses, float *reg_loss, float *d_hm, float *const *d_regs, void *ws,
                         size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 23. PillarVFE with one last-layer PFNLayer, forward + parameter gradients (csrc/pillar_vfe.hip, csrc/pfn_layer.h)
 *    replaces: PillarVFE.forward + PFNLayer.forward for NUM_FILTERS of length 1 with USE_NORM (reference
 *      pcdet/models/backbones_3d/vfe/pillar_vfe.py:29-123): the feature cat, the mask multiply, Linear(C_in, 64,
 *      bias=False), BatchNorm1d between two permutes, ReLU and the max over the T rows of a pillar, each a pass over
 *      an [M, T, 64] tensor, and their autograd.
 *    Training forward 3 launches (S1 = sum f and G = sum f f^T over the real points, one double partial per block; the
 *    fixed-order sum, the batch statistics from S1, G and the weight, the running statistics; the per-pillar max), eval
 *    forward 1, backward 2.  No float atomics, every sum in double in a fixed order: outputs and gradients are bitwise
 *    reproducible.  No host read: every launch shape depends on host values only.
 * ---------------------------------------------------------------------------------------------- */

/* Inputs, device: voxels [m, t, c] fp32 (x, y, z first), 1 <= t <= 32, 3 <= c <= 6; num_points [m] int32; coords
 *   [m, 4] int32 (b, z, y, x); d_n: device int64[1] live row count (clamped to m) or NULL = m; weight [c_out, c_in]
 *   fp32, c_in = (use_absolute_xyz ? c + 6 : c + 3) + (with_distance ? 1 : 0) else SPX_ERR_INVALID_ARG; c_out != 64:
 *   SPX_ERR_UNSUPPORTED; gamma, beta, running_mean, running_var [c_out] fp32, num_batches_tracked int64[1] (the three
 *   may be NULL in training: no running statistics are kept); geom6: HOST float[6] = voxel size (x, y, z), then the
 *   centre offsets voxel / 2 + range_lo (x, y, z).
 * Features of point t < n = min(max(num_points, 0), t) of a pillar, in weight-column order: [x, y, z if
 *   use_absolute_xyz | columns 3 .. c - 1 | xyz - (sum of xyz over the n real points) / n | xyz - centre | |xyz| if
 *   with_distance], centre = fl32(fl32(coord * voxel) + offset); differences, sums and products are taken in double.
 *   Rows t >= n are all-zero feature rows: their linear output is 0, they count in the statistics (sample count N =
 *   live rows * t) and their value relu(beta - mean * gamma * invstd) takes part in the max of a pillar with n < t.
 *   A live row with num_points <= 0 is all padding (the reference divides by 0 there).
 * training != 0: z = (x - mean) * invstd * gamma + beta with the biased batch variance, invstd = 1 / sqrt(var + eps);
 *   running_mean / running_var move by `momentum` towards the batch mean / UNBIASED variance, num_batches_tracked
 *   += 1; save_mean, save_invstd [c_out] fp32 and stats [spx_pillar_vfe_stats_len()] doubles (G, S1, mean, invstd, N:
 *   what the backward needs) are written.  training == 0: z from the running statistics; save_*, stats, ws unused.
 * Outputs: out [m, c_out] = max over the t rows of relu(z); arg [m, c_out] uint8 = the winning row's index, t when a
 *   padding row won; equal values take the lowest index (so a pillar whose values are all 0 reports its first row).
 *   Rows >= the live count are never read; their out and arg are exact zeros.  m == 0: SPX_OK, nothing launched.
 * ws: spx_pillar_vfe_ws_bytes(m) bytes (both entry points). */
size_t spx_pillar_vfe_stats_len(void);
size_t spx_pillar_vfe_ws_bytes(int64_t m);
int spx_pillar_vfe_fwd(const float *voxels, const int32_t *num_points, const int32_t *coords, int64_t m, const int64_t *d_n,
                       int32_t t, int32_t c, const float *weight, int32_t c_in, int32_t c_out, const float *gamma,
                       const float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                       float momentum, float eps, const float *geom6, int use_absolute_xyz, int with_distance,
                       int training, float *out, uint8_t *arg, float *save_mean, float *save_invstd, double *stats,
                       void *ws, size_t ws_bytes, spx_stream_t stream);

/* d_weight [c_out, c_in], d_gamma, d_beta [c_out] from d_out [m, c_out], every element written.  g = d_out at the row
 *   arg selects of each live (pillar, channel) with out > 0, 0 on every other of the N rows.  training != 0 (stats of
 *   the forward): the exact train-mode BatchNorm gradient, d_beta = sum g, d_gamma = sum g xhat, d_weight = gamma
 *   invstd [sum g f - (d_beta / N) S1 - (d_gamma / N) invstd (G w - mean S1)], without an [m, t, c_out] tensor.
 *   training == 0 (running statistics): d_weight = gamma invstd sum g f.  No gradient w.r.t. voxels exists. */
int spx_pillar_vfe_bwd(const float *voxels, const int32_t *num_points, const int32_t *coords, int64_t m, const int64_t *d_n,
                       int32_t t, int32_t c, const float *weight, int32_t c_in, int32_t c_out, const float *gamma,
                       const float *running_mean, const float *running_var, float eps, const float *geom6,
                       int use_absolute_xyz, int with_distance, int training, const float *out, const uint8_t *arg,
                       const float *d_out, const double *stats, float *d_weight, float *d_gamma, float *d_beta, void *ws,
                       size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 24. DynamicPillarVFE: sync-free pillarisation and one fused last-layer PFNLayerV2 (csrc/dyn_pillar_vfe.hip,
 *     csrc/pfn_layer.h)
 *    replaces: DynamicPillarVFE.forward + PFNLayerV2.forward for NUM_FILTERS of length 1 with USE_NORM (reference
 *      pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:88-146): torch.unique over the cell keys (a sort and a host
 *      read), scatter_mean / scatter_max through torch_scatter (float atomics), the gathers by unq_inv and an [N, 64]
 *      activation tensor written and read several times.
 *    Every in-range point is kept: no per-pillar or per-frame cap, no [M, T, C] buffer; a pillar is a ragged list.
 *    Pillarisation 10 launches, training forward 5, eval forward 3, backward 2.  Integer atomics only (bitmap OR, counts,
 *    a work list), no float atomics, every floating sum in double in a fixed order: all outputs are bitwise reproducible.  No
 *    host read: every launch shape depends on host values only.
 * ---------------------------------------------------------------------------------------------- */

/* points [n_points, stride] fp32, x and y at columns xyz_col, xyz_col + 1, the frame index at batch_col (< 0: frame 0).
 *   range_lo2 (xmin, ymin), voxel_size2, grid2 (X, Y): HOST arrays.  cx = floor(fl32(fl32(x - xmin) / vx)), cy likewise.
 * A point is kept iff 0 <= cx < X and 0 <= cy < Y; z is NOT tested (as in the reference); a NaN x or y drops the point.
 *   A point whose batch column is outside [0, batch) is dropped too: that is the padding convention for static capacity
 *   (pad a cloud with batch = -1 rows).  The reference does not check the batch column.
 * Pillars are the unique cells in ascending key (b X + cx) Y + cy, torch.unique's order.  Outputs, device:
 *   coords [cap, 4] int32 = (b, 0, cy, cx); point_to_pillar [n_points] int32 = torch.unique's inverse, -1 for a dropped
 *   point or a pillar row >= cap; count [cap] int32 (0 for a dead row); offset [cap + 1] int32 = the exclusive scan of
 *   count; order [n_points] int32 = point rows grouped by pillar, ascending point row inside a pillar (positions >=
 *   *d_num_points are not written); d_num_pillars int64[1] = the true pillar count, which may exceed cap (d_status,
 *   nullable, then receives SPX_ERR_CAPACITY); d_num_points int64[1] = the number of points with point_to_pillar >= 0.
 *   coords rows >= min(*d_num_pillars, cap) are not written.
 * batch * X * Y >= 2^31, n_points >= 2^31, cap >= 2^31 - 1: SPX_ERR_TOO_LARGE.  ws: spx_dynamic_pillarize_ws_bytes. */
size_t spx_dynamic_pillarize_ws_bytes(int64_t n_points, int batch, const int32_t *grid2, int64_t cap);
int spx_dynamic_pillarize(const float *points, int64_t n_points, int stride, int batch_col, int xyz_col,
                          const float *range_lo2, const float *voxel_size2, const int32_t *grid2, int batch,
                          int32_t *coords, int32_t *point_to_pillar, int32_t *count, int32_t *offset, int32_t *order,
                          int64_t *d_num_pillars, int64_t *d_num_points, int64_t cap, int32_t *d_status, void *ws,
                          size_t ws_bytes, spx_stream_t stream);

/* Inputs: points as above with the c raw feature columns (x, y, z first, 3 <= c <= 6) at xyz_col .. xyz_col + c - 1;
 *   coords, point_to_pillar, offset, order, d_num_pillars, d_num_points, cap: what spx_dynamic_pillarize wrote; weight
 *   [c_out, c_in] fp32, c_in = (use_absolute_xyz ? c + 6 : c + 3) + (with_distance ? 1 : 0) else SPX_ERR_INVALID_ARG;
 *   c_out != 64: SPX_ERR_UNSUPPORTED; gamma, beta, running_mean, running_var [c_out] fp32, num_batches_tracked int64[1]
 *   (the three may be NULL in training); geom5: HOST float[5] = voxel size (x, y), then the centre offsets voxel / 2 +
 *   range_lo (x, y, z).
 * Features of a kept point, in weight-column order: [x, y, z if use_absolute_xyz | columns 3 .. c - 1 | xyz - pillar
 *   mean | xyz - centre | |xyz| if with_distance]; the centre of x and y is fl32(fl32(cell * voxel) + offset), the centre
 *   of z is the constant offset z; the pillar mean is a double sum over `order` in a fixed order (written to pillar_mean
 *   [cap, 3] doubles, which the backward reads); differences, sums and products are taken in double.
 * training != 0: batch statistics over the N = *d_num_points kept points, z = (x - mean) * invstd * gamma + beta with the
 *   biased variance; running_mean / running_var move by `momentum` towards the batch mean / UNBIASED variance,
 *   num_batches_tracked += 1; save_mean, save_invstd [c_out] fp32 and stats [spx_dynamic_pillar_vfe_stats_len()] doubles
 *   (G, S1, mean, invstd, N) are written.  N < 2 (torch raises): nothing is divided by zero, the running statistics and
 *   the counter stay untouched and d_status (nullable) receives SPX_ERR_BATCH_STATS.  training == 0: z from the running
 *   statistics; save_*, stats unused.
 * Outputs: out [cap, c_out] = max over the pillar's points of relu(z); arg [cap, c_out] int32 = the winning point's row
 *   in `points`; equal values take the lowest position in `order`.  Rows >= min(*d_num_pillars, cap) are never
 *   dereferenced; their out is exact zeros and their arg -1.
 * ws: spx_dynamic_pillar_vfe_ws_bytes(n_points) bytes (both entry points). */
size_t spx_dynamic_pillar_vfe_stats_len(void);
size_t spx_dynamic_pillar_vfe_ws_bytes(int64_t n_points);
int spx_dynamic_pillar_vfe_fwd(const float *points, int64_t n_points, int stride, int xyz_col, int32_t c,
                               const int32_t *coords, const int32_t *point_to_pillar, const int32_t *offset,
                               const int32_t *order, int64_t cap, const int64_t *d_num_pillars,
                               const int64_t *d_num_points, const float *weight, int32_t c_in, int32_t c_out,
                               const float *gamma, const float *beta, float *running_mean, float *running_var,
                               int64_t *num_batches_tracked, float momentum, float eps, const float *geom5,
                               int use_absolute_xyz, int with_distance, int training, float *out, int32_t *arg,
                               double *pillar_mean, float *save_mean, float *save_invstd, double *stats,
                               int32_t *d_status, void *ws, size_t ws_bytes, spx_stream_t stream);

/* d_weight [c_out, c_in], d_gamma, d_beta [c_out] from d_out [cap, c_out], every element written.  g = d_out at the point
 *   arg selects of each live (pillar, channel) with out > 0, 0 on every other of the N points.  training != 0 (stats of
 *   the forward): d_beta = sum g, d_gamma = sum g xhat, d_weight = gamma invstd [sum g f - (d_beta / N) S1 - (d_gamma / N)
 *   invstd (G w - mean S1)].  training == 0: d_weight = gamma invstd sum g f on the running statistics.  Points are
 *   data: no gradient goes to them. */
int spx_dynamic_pillar_vfe_bwd(const float *points, int64_t n_points, int stride, int xyz_col, int32_t c,
                               const int32_t *coords, int64_t cap, const int64_t *d_num_pillars, const float *weight,
                               int32_t c_in, int32_t c_out, const float *gamma, const float *running_mean,
                               const float *running_var, float eps, const float *geom5, int use_absolute_xyz,
                               int with_distance, int training, const float *out, const int32_t *arg, const float *d_out,
                               const double *pillar_mean, const double *stats, float *d_weight, float *d_gamma,
                               float *d_beta, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 25. Rotated RoI bilinear pooling of a BEV map (csrc/roi_grid_pool.hip)
 *    replaces: SECONDHead.roi_grid_pool (reference pcdet/models/roi_heads/second_head.py:53-110): a loop over frames
 *      with affine_grid + grid_sample on a (num_rois, C, H, W) expanded view.  One launch, forward only: the reference
 *      detaches both the RoIs and the map, so no gradient exists.  No host read, no atomics.
 * ---------------------------------------------------------------------------------------------- */

/* rois [batch, n_rois, roi_stride] fp32 (x, y, z, dx, dy, dz, heading, ...), roi_stride >= 7; features: fp32 map of
 *   batch x c x h x w elements addressed by the four element strides (dense NCHW, channels_last, or any view), h, w >= 2;
 *   d_n: device int64[1] live row count over the batch * n_rois rows (clamped) or NULL = all; min_x, min_y: the range's
 *   lower corner; step_x, step_y > 0: metres per map pixel (voxel size * downsample ratio).
 * Per RoI, in double: x1 = (x - dx / 2 - min_x) / step_x, x2 = (x + dx / 2 - min_x) / step_x, y1, y2 likewise; theta =
 *   [(x2 - x1) / (w - 1) cos a, -(x2 - x1) / (w - 1) sin a, (x1 + x2 - w + 1) / (w - 1); (y2 - y1) / (h - 1) sin a,
 *   (y2 - y1) / (h - 1) cos a, (y1 + y2 - h + 1) / (h - 1)], each entry ROUNDED TO fp32.  Cell (i, j) of the grid_size^2
 *   grid has base coordinates bx = (2 j + 1) / G - 1, by = (2 i + 1) / G - 1, sample point g = theta (bx, by, 1) and
 *   pixel coordinates ((gx + 1) w - 1) / 2, ((gy + 1) h - 1) / 2 (affine_grid and grid_sample with align_corners =
 *   False), bilinear, taps outside the map contribute 0: a cell whose four taps are all outside is exactly 0.
 * out [batch * n_rois, c, G, G] fp32, contiguous; every element is written; rows >= the live count are zeros and their
 *   RoIs are not read.  grid_size > 12: SPX_ERR_UNSUPPORTED.  batch * n_rois == 0: SPX_OK, nothing launched. */
int spx_roi_grid_pool_bev(const float *rois, int32_t batch, int64_t n_rois, int32_t roi_stride, const int64_t *d_n,
                          const float *features, int32_t c, int32_t h, int32_t w, int64_t stride_b, int64_t stride_c,
                          int64_t stride_h, int64_t stride_w, int32_t grid_size, double min_x, double min_y,
                          double step_x, double step_y, float *out, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 26. Second-stage proposal sampling: RoI / GT matching and fg / bg sampling (csrc/proposal_targets.hip)
 *    replaces: ProposalTargetLayer.sample_rois_for_rcnn, subsample_rois, sample_bg_inds, get_max_iou_with_same_class
 *      (reference pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:64-228): loops over frames and
 *      classes with nonzero / numel / item host reads and numpy / CPU-torch random numbers.
 *    Two launches for the batch.  The random draws are inputs.  One integer LDS atomic, no float atomics, no host read:
 *    the outputs are a pure function of the inputs, bitwise reproducible.
 * ---------------------------------------------------------------------------------------------- */

/* rois [batch, r, roi_stride] fp32, roi_stride >= 7; roi_labels [batch, r] int64; gt_boxes [batch, gmax, gt_stride] fp32,
 *   gt_stride >= 8, the class in the LAST column; 1 <= r <= 2048 else SPX_ERR_TOO_LARGE; gmax >= 1.
 *   fg_keys [batch, r] fp32: one sort key per RoI; slot_u [batch, m] fp32 in [0, 1): one draw per output slot.
 * Per frame: trailing GT rows whose fp32 column sum (in column order) is 0 are dropped; row 0 always stays, interior zero
 *   rows stay.  The 3-D IoU of a pair is BEV overlap (box_iou.h overlap_area(roi, gt)) x height overlap / max(union
 *   volume, 1e-6), in fp32.  A RoI takes the GT row of largest IoU, the lowest row on ties; with by_class only rows
 *   whose class, truncated to an integer, equals its label count, a RoI with no such row gets overlap 0 and row 0, and
 *   one whose rows all have IoU 0 gets the first of them.
 * Candidates, by overlap o: fg o >= min(reg_fg, cls_fg); hard bg bg_lo <= o < reg_fg; easy bg o < bg_lo (fg and hard
 *   overlap when reg_fg > cls_fg), each list in ascending RoI order, sizes n_fg, n_hard, n_easy.  Output slots:
 *   n_fg > 0 and bg exists: the first min(fg_per_image, n_fg) fg candidates in ascending (fg_keys, RoI index) order, then
 *     the bg slots; no fg: m bg slots.  bg slots: hard first, min((int)(slots * hard_bg_ratio), n_hard) of them when both
 *     kinds exist (the product in double), all of them when only hard exists, then easy.
 *   n_fg > 0 and no bg: m fg slots with replacement.
 *   A slot with replacement at position s takes entry min(floor(slot_u[s] * n), n - 1) of its list of n (in double).
 * Outputs [batch, m]: sampled_inds int64 (RoI row in the frame), roi_ious fp32, gt_inds int64 (GT row in the frame).
 * ws: spx_proposal_sample_ws_bytes(batch, r, gmax) bytes.  batch == 0: SPX_OK, nothing launched. */
size_t spx_proposal_sample_ws_bytes(int32_t batch, int32_t r, int32_t gmax);
int spx_proposal_sample(const float *rois, const int64_t *roi_labels, const float *gt_boxes, int32_t batch, int32_t r,
                        int32_t roi_stride, int32_t gmax, int32_t gt_stride, int32_t m, int32_t fg_per_image,
                        float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh_lo, double hard_bg_ratio,
                        int by_class, const float *fg_keys, const float *slot_u, int64_t *sampled_inds, float *roi_ious,
                        int64_t *gt_inds, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 27. Voxel-grid max pooling: the tail of NeighborVoxelSAModuleMSG after the voxel query (csrc/voxel_pool.hip)
 *    replaces: the gather of (M, C, nsample) features, masked_fill, the position Conv2d + BatchNorm2d on the
 *      (M, 3, nsample) offsets, the add, ReLU and max over the slots (reference
 *      pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py, max_pool), forward and backward.  BatchNorm is NOT in
 *      here: the caller folds it into the affine map (a, b) from the moments below.
 *    Queries m in [0, m); slots s in [0, nsample); source row r = idx[m, s] (GLOBAL rows); e = empty[m] != 0 (empty may
 *    be NULL: none).  d(m, s) = xyz[r] - new_xyz[m], three fp32 subtractions, or (0, 0, 0) when e.  idx of an empty
 *    query is never read.  A slot whose r is outside [0, n_src) is SKIPPED, never dereferenced; a query whose slots are
 *    all skipped behaves as empty.  Any c >= 1, nsample >= 1.  No host read, no float atomics, bitwise reproducible,
 *    capturable.  m * nsample, m * c >= 2^31 - 1: SPX_ERR_TOO_LARGE.
 * ---------------------------------------------------------------------------------------------- */

/* xyz [n_src, 3], new_xyz [m, 3], idx [m, nsample] int32, empty [m] bytes -> moments double[9] on the device:
 *   (sum dx, sum dy, sum dz, sum dx dx, dx dy, dx dz, dy dy, dy dz, dz dz) over all m * nsample columns, d promoted to
 *   double after the fp32 subtraction; empty queries and skipped slots are zero columns, repeated slots count every time.
 *   DETERMINISTIC: per-block partials over chunks of 2048 columns, then a fixed-order sum of the partials.
 *   ws: spx_voxel_pool_moments_ws_bytes bytes. */
size_t spx_voxel_pool_moments_ws_bytes(int64_t m, int32_t nsample);
int spx_voxel_pool_moments(const float *xyz, const float *new_xyz, const int32_t *idx, const uint8_t *empty,
                           int64_t n_src, int64_t m, int32_t nsample, double *moments, void *ws, size_t ws_bytes,
                           spx_stream_t stream);

/* f [n_src, c], a [c, 3], b [c] -> out [m, c] fp32, arg [m, c] int32, every element written.  In fp32, with
 *     v(m, s, ch) = (e ? 0 : f[r, ch]) + (((a[ch,0] * dx + a[ch,1] * dy) + a[ch,2] * dz) + b[ch])
 *   (the compiler may contract a product and the add that follows it into one fused multiply-add):
 *     out[m, ch] = max(0, max_s v);  arg[m, ch] = the lowest s attaining the maximum when out > 0, else -1.
 *   An empty query has v = b[ch] in every slot: out = max(0, b[ch]), arg = 0 when b[ch] > 0.  A NaN v never wins. */
int spx_voxel_pool_max_fwd(const float *f, const float *xyz, const float *new_xyz, const int32_t *idx,
                           const uint8_t *empty, const float *a, const float *b, int32_t c, int64_t n_src, int64_t m,
                           int32_t nsample, float *out, int32_t *arg, spx_stream_t stream);

/* Backward of spx_voxel_pool_max_fwd.  dout [m, c], arg from the forward; g = dout[m, ch] where arg >= 0, else 0.  Any
 *   output may be NULL (not computed), not all:
 *   df [n_src, c], fully written (0 where nothing points): df[r, ch] = sum of g over the (m, ch) whose winning slot
 *     points at r (non-empty queries only), DETERMINISTIC: sorted runs of the (m, s) entries by r
 *     (csrc/sorted_runs.h), each run added in ascending m;
 *   da [c, 3] = sum_m g * d(m, arg), db [c] = sum_m g, DETERMINISTIC: per-block partials over chunks of 128 queries
 *     (four interleaved ascending sub-sums, added in order), then a fixed-order sum of the partials.
 *   No gradient flows to xyz or new_xyz.  ws: spx_voxel_pool_max_bwd_ws_bytes bytes. */
size_t spx_voxel_pool_max_bwd_ws_bytes(int32_t c, int64_t n_src, int64_t m, int32_t nsample);
int spx_voxel_pool_max_bwd(const float *dout, const int32_t *arg, const int32_t *idx, const uint8_t *empty,
                           const float *xyz, const float *new_xyz, int32_t c, int64_t n_src, int64_t m, int32_t nsample,
                           float *df, float *da, float *db, void *ws, size_t ws_bytes, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 28. Two-layer shared-MLP max pooling: the eval-mode tail of a StackSAModuleMSG scale after the ball query
 *     (csrc/sa_mlp.hip)
 *    replaces: the two groupings into (M, 3 + C, nsample), Conv2d + eval BatchNorm2d + ReLU twice over
 *      (1, C, M, nsample) tensors and the max over the slots (reference
 *      pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py, StackSAModuleMSG with two-layer mlps, max_pool).  The
 *      first conv's feature columns are the caller's GEMM p = features Wf^T over the SOURCE rows (as in §22); both
 *      BatchNorms are folded by the caller into (a1, b1), (a2, b2) from their running statistics.  Forward only.
 *    Queries m in [0, m); slots s in [0, nsample); r = idx[m, s] (GLOBAL rows); e = empty[m] != 0 (empty may be NULL).
 *    A column is ZERO when e, or when r is outside [0, n_src) (never dereferenced): it has p = 0 and d = 0, so
 *    h = relu(b1) — the reference zeroes the grouped tensor of an empty ball and still runs the MLP over it; an empty
 *    query is therefore NOT a zero output row.  idx of an empty query is never read.  Otherwise, in fp32,
 *      d = xyz[r] - new_xyz[m]
 *      h[s, c]   = max(0, a1[c] * (p[r, c] + ((wx[c,0] * dx + wx[c,1] * dy) + wx[c,2] * dz)) + b1[c])
 *      out[m, o] = max_s max(0, a2[o] * (sum_c w2[o, c] * h[s, c]) + b2[o])
 *    (the compiler may contract a product and the add that follows into one fused multiply-add; the sum over c is a
 *    chain of fused multiply-adds in the order c = k * c1 / 4 + j, j outer, k inner).
 *    p [n_src, c1] 16-byte aligned, or NULL (a grouper without features: p = 0); xyz [n_src, 3]; new_xyz [m, 3];
 *    idx [m, nsample] int32; wx [c1, 3]; a1, b1 [c1]; w2 [c2, c1]; a2, b2 [c2] -> out [m, c2], every element written.
 *    c1, c2 in {16, 32, 64}, nsample in {16, 32}: anything else SPX_ERR_UNSUPPORTED.  No workspace, no host read, no
 *    atomics, bitwise reproducible, capturable.  m * nsample, m * c2 >= 2^31 - 1: SPX_ERR_TOO_LARGE.
 * ---------------------------------------------------------------------------------------------- */
int spx_sa_mlp2_max(const float *p, const float *xyz, const float *new_xyz, const int32_t *idx, const uint8_t *empty,
                    const float *wx, const float *a1, const float *b1, const float *w2, const float *a2, const float *b2,
                    int32_t c1, int32_t c2, int64_t n_src, int64_t m, int32_t nsample, float *out, spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 29. Post-processing of dense (B, N, .) predictions without a host read (csrc/dense_post_process.hip)
 *    replaces: the per-frame mask / nonzero / topk / NMS / count read of Detector3DTemplate.post_processing over the
 *      anchors of AnchorHeadSingle and over the RoIs of a second stage (reference detector3d_template.py:207-349,
 *      model_nms_utils.py), and the topk + per-frame NMS of RoIHeadTemplate.proposal_layer (roi_head_template.py:45-95).
 *    §15 keeps a frame's candidates in one workgroup's LDS (n <= 4096); here n is any size with b * n < 2^31: an exact
 *    radix select over all rows, one LDS sort per (frame, class), the NMS pair tests spread over the whole grid.
 *    Every stage is a launch of its own; the launch count depends on the arguments only; integer atomics only; no host
 *    read; bitwise reproducible; capturable.  frame f owns the rows [f * n, (f + 1) * n).
 * ---------------------------------------------------------------------------------------------- */

size_t spx_dense_select_ws_bytes(int32_t b, int64_t n, int32_t n_thresh, int64_t pre_max);

/* The pre_max best members of every (frame, class).  scores [b * n] (already normalised), labels [b * n] int32 (1-based,
 *   read only when per_class != 0), thresholds: HOST float[n_thresh], or NULL for no threshold.
 *   Members of (frame f, class c): rows of f with score >= thresholds[c] (NULL: every row) and, per_class != 0,
 *   label == c + 1; per_class == 0 needs n_thresh == 1.  A NaN score is NEVER a member (torch.topk ranks it first).
 *   -> cand [b, n_thresh, pre_max] int64: the members by score descending, EQUAL SCORES LOWER ROW FIRST (-0 equals +0),
 *      the first pre_max, as rows in [0, b * n), -1 past the count; cand_count [b, n_thresh] int32.  Every element
 *      written on every call.  Exact for any score distribution.
 *   1 <= pre_max <= 16384, b <= 65535, b * n < 2^31, else SPX_ERR_TOO_LARGE; n_thresh <= 8 else SPX_ERR_UNSUPPORTED;
 *   b * n == 0: SPX_OK, nothing launched.  Launches: 1 + 2 * ceil((32 + bits(n - 1)) / 11) + 2. */
int spx_dense_select(const float *scores, const int32_t *labels, int32_t b, int64_t n, const float *thresholds,
                     int32_t n_thresh, int64_t pre_max, int per_class, int64_t *cand, int32_t *cand_count, void *ws,
                     size_t ws_bytes, spx_stream_t stream);

size_t spx_dense_post_process_ws_bytes(int32_t b, int64_t n, int32_t n_thresh, int64_t pre_max, int64_t post_max);

/* spx_dense_select, then per (frame, class) the greedy NMS of §15 over the sorted candidates (the pair test of
 *   csrc/box_iou.h, (earlier, later); rotated BEV, or axis aligned when axis_aligned != 0) cut at post_max, then with
 *   per_class != 0 the classes' survivors ordered again and reduced by one more NMS: the semantics and the OUTPUTS of
 *   spx_point_post_process (sel, count, out_boxes, out_scores, out_labels with K = spx_point_post_process_capacity(n,
 *   n_thresh, post_max, per_class) rows per frame, every element written), for any n, plus the NULL threshold.
 *   boxes [b * n, box_ld] fp32, box_ld >= 7, the first 7 columns are the box.
 *   The pair tests fill the upper triangle of a bit matrix [min(pre_max, n), ceil(min(pre_max, n) / 64)] of 64-bit words
 *   per (frame, class) in the workspace; the greedy walk stops at post_max kept boxes.
 *   Limits of spx_dense_select, and n_thresh * min(post_max, pre_max, n) <= 4096 (the final stage is one workgroup per
 *   frame) else SPX_ERR_TOO_LARGE.  Three launches after the selection's. */
int spx_dense_post_process(const float *scores, const int32_t *labels, const float *boxes, int32_t box_ld, int32_t b,
                           int64_t n, const float *thresholds, int32_t n_thresh, float nms_thresh, int64_t pre_max,
                           int64_t post_max, int axis_aligned, int per_class, int64_t *sel, int32_t *count,
                           float *out_boxes, float *out_scores, int64_t *out_labels, void *ws, size_t ws_bytes,
                           spx_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 30. Batched RoI-aware pooling that writes only the live cells, and ragged points in boxes (csrc/roiaware_sparse.hip)
 *    replaces: the per-frame loop of PartA2FCHead.roiaware_pool and the lines after it (reference
 *      pcdet/models/roi_heads/partA2_head.py:104-204): per frame two RoIAwarePool3d calls (avg over the 4 part
 *      channels, max over the backbone channels) into dense (N, o, o, o, C) grids, sum(-1).nonzero() (a host read), the
 *      gather of the non-empty cells and the fake_sparse_idx branch; and points_in_boxes_gpu over frames of unequal
 *      length.
 *    Semantics: §12's, verbatim (inside test, cell index, the first max_pts - 1 points per cell in ascending point
 *      index, max with strict > in list order and no winner -> 0 / arg -1, avg = list-order sum / count, the backward's
 *      grad * (1 / fmaxf(count, 1)) and its ascending-RoI order from 0.0f), extended to a batch:
 *      b frames, n_per RoIs each; RoI row r = f * n_per + i sees only the points of frame f, the rows
 *      [start_f, start_f + frame_cnt[f]) of points, start_f = frame_cnt[0] + ... + frame_cnt[f - 1].
 *      rois [b * n_per, 7]; points [np, 4] = (frame, x, y, z), rows grouped by ascending frame (the frame column is not
 *      read: frame_cnt decides); frame_cnt DEVICE int32[b]; part [np, 4]; rpn [np, c]; all fp32 contiguous.
 *      pf = the row stride of the per-RoI point records: a HOST bound on the longest frame (np always suffices).
 *    Emitted cells: a cell that keeps at least one point AND whose four averaged part values have a non-zero fp32 sum
 *      ((a0 + a1) + a2) + a3.  Defined for non-negative part values (sigmoid outputs): the order of the adds then cannot
 *      change whether the sum is zero.  Row order: ascending (r, x, y, z), the row-major order of nonzero().
 *    Fake branch: fewer than 3 emitted cells in the whole batch -> one row (r, 0, 0, 0) per RoI holding that cell's pooled
 *      values (zeros, cnt 0, arg -1 when it is empty); n_rows = b * n_per, faked = 1.  Decided on the device.
 *    Static capacity: rows at and past n_rows are dead: features 0, cnt 0, arg -1, coords -1; consumers take n_rows as
 *      their live count (no kernel of the library reads a dead row).  n_rows > rows: SPX_ERR_CAPACITY in d_status (nullable,
 *      see spx_read_status) and the rows past the capacity are dropped (row_of_cell -1: no gradient either).  Counts that
 *      are negative, exceed np in sum, or a frame longer than pf: SPX_ERR_CAPACITY in d_status, the spans clamped to the
 *      arrays (never an access outside them).
 *    Limits, else SPX_ERR_TOO_LARGE: b <= 256 (every workgroup sums the earlier counts); b * n_per <= 2^20 RoI rows (the
 *      scan is ONE workgroup walking them 1024 at a time); each out size < 256, b * n_per * ox * oy * oz < 2^31 (cell
 *      counters in LDS up to 8192 cells per RoI, in the workspace beyond); np, pf < 2^29 - 1, b * n_per * pf < 2^31,
 *      np * c < 2^31, rows < 2^29, rows * c < 2^31.
 *    Integer atomics only (the per-cell counters), no float atomics, no host read, bitwise reproducible, capturable.
 * ---------------------------------------------------------------------------------------------- */

/* The state of one collect call (point records, cell counts, lists, ranks): kept by the caller until the last pool /
 *   backward call that belongs to it.  0 for arguments the calls below refuse. */
size_t spx_roiaware_sparse_ws_bytes(int32_t b, int64_t n_per, int64_t pf, int32_t ox, int32_t oy, int32_t oz);

/* Two launches: collect (one workgroup per RoI: its frame's points, the lists, which cells are emitted) and the scan.
 *   -> n_rows DEVICE int64[1], faked DEVICE int32[1], both written on every call; ws: the state.
 *   b * n_per == 0: n_rows = 0, faked = 0. */
int spx_roiaware_sparse_collect(const float *rois, const float *points, const int32_t *frame_cnt, const float *part,
                                int32_t b, int64_t n_per, int64_t np, int64_t pf, int32_t ox, int32_t oy, int32_t oz,
                                int32_t max_pts, int64_t *n_rows, int32_t *faked, int32_t *d_status, void *ws,
                                size_t ws_bytes, spx_stream_t stream);

/* One launch (a wave per emitted row, its lanes over the 4 + c channels).  ws, n_rows, faked: of the collect call.
 *   -> coords [rows, 4] int32 (r, x, y, z); out_part [rows, 4]; out_rpn [rows, c]; arg [rows, c] int32 (GLOBAL point
 *      rows, -1: no winner); cnt [rows] int32; row_of_cell [b * n_per * ox * oy * oz] int32 (-1: no row).  Every element
 *      written on every call; may be called again with another capacity. */
int spx_roiaware_sparse_pool(const float *part, const float *rpn, int32_t b, int64_t n_per, int64_t np, int64_t pf,
                             int32_t c, int32_t ox, int32_t oy, int32_t oz, int64_t rows, const int64_t *n_rows,
                             const int32_t *faked, int32_t *row_of_cell, int32_t *coords, float *out_part,
                             float *out_rpn, int32_t *arg, int32_t *cnt, int32_t *d_status, const void *ws,
                             size_t ws_bytes, spx_stream_t stream);

/* grad [rows, c] -> grad_in [np, c], every element written.  mode 0 = max (arg [rows, c] of the pool call; cnt unused),
 *   1 = avg (cnt [rows]; arg unused; c = 4 for the part tensor).  One launch: a thread per (point, channel) walks the RoI
 *   rows of its own frame in ascending r from 0.0f and adds, through row_of_cell, grad[row] where arg == p (max) or
 *   grad[row] * (1 / fmaxf(cnt[row], 1)) (avg).  No sort, no atomics. */
int spx_roiaware_sparse_bwd(const float *grad, const int32_t *arg, const int32_t *cnt, const int32_t *row_of_cell,
                            const int32_t *frame_cnt, int32_t b, int64_t n_per, int64_t np, int64_t pf, int32_t c,
                            int32_t ox, int32_t oy, int32_t oz, int64_t rows, int32_t mode, float *grad_in,
                            const void *ws, size_t ws_bytes, spx_stream_t stream);

/* points [np, 4] = (frame, x, y, z) in any row order, boxes [b, t, 7] -> box_idx [np] int32: the first box of the
 *   point's own frame that holds it (spx_points_in_boxes' test, ascending box index), -1 when none or when the frame
 *   value is outside [0, b).  np < 2^29 - 1, t < 2^31 / 7, b <= 65535 else SPX_ERR_TOO_LARGE.  One launch. */
int spx_points_in_boxes_stack(const float *points, const float *boxes, int32_t b, int64_t np, int64_t t,
                              int32_t *box_idx, spx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPX_H_ */
