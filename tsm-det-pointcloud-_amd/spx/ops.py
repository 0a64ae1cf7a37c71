"""Tensor-level wrappers over the C ABI (include/spx.h).  torch is used for device memory and streams only.

Every function here launches HIP kernels from libspx.so on torch's current stream; nothing is computed by
torch ops and there is no CPU path (inputs must live on a GPU).
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import check, f_arr, i3

_WS = {}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the stream handle without building a Stream object


def _stream_handle(device):
    """torch's current stream on `device` as an integer handle (several microseconds cheaper per call than
    torch.cuda.current_stream(): the small layers at the end of the backward pass are host bound)."""
    if _raw_stream is not None:
        idx = device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream


def _stream(t):
    return ctypes.c_void_p(_stream_handle(t.device))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.SpxError("spx ops need GPU tensors (got a %s tensor): the sparse-conv hot path has no "
                                "CPU fallback" % t.device)


def workspace(device, nbytes):
    """Grow-only scratch buffer per (device, stream); stream order makes back-to-back reuse safe."""
    key = (device.index, _stream_handle(device))
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


_STATUS = {}


def status_word(device):
    """The sticky device status word of `device` (int32[1], include/spx.h: d_status): kernels of calls made without a host
    read (static-capacity / graph mode) report device-side errors here; check_status() reads it."""
    w = _STATUS.get(device.index)
    if w is None:
        w = _STATUS[device.index] = torch.zeros((1,), dtype=torch.int32, device=device)
    return w


def check_status(device):
    """Read (one host sync) and reset the sticky status word; raises SpxError on a device-side error."""
    w = status_word(device)
    rc = int(w.item())
    if rc != 0:
        w.zero_()
        check(rc, "device status")


def _count_and_status(buf, what):
    """buf: int64[2] = (row count, status word in the low 32 bits) -> count; raises on a device-side error (one sync)."""
    cnt, st = buf.tolist()
    st &= 0xFFFFFFFF
    if st:
        check(st - (1 << 32), what)
    return int(cnt)


def out_shape_of(in_shape, ksize, stride, pad, dil):
    return [(int(i) + 2 * int(p) - int(d) * (int(k) - 1) - 1) // int(s) + 1
            for i, k, s, p, d in zip(in_shape, ksize, stride, pad, dil)]


class Rulebook(object):
    """Indice pairs of one sparse conv (what spconv caches under `indice_key`).

    pair      int32 [K, ld]   forward table: pair[k, o] = input row feeding output o at offset k (or -1)
    pair_bwd  int32 [K, n_in] backward table (None for submanifold: the forward table is read at K-1-k)
    """

    def __init__(self, pair, ld, n_in, n_out, kvol, subm, out_indices, out_shape, in_shape, pair_bwd=None, cnt=None,
                 ksize=None, stride=None, padding=None, dilation=None):
        self.pair, self.ld, self.n_in, self.n_out, self.kvol, self.subm = pair, ld, n_in, n_out, kvol, subm
        self.out_indices, self.out_shape, self.in_shape = out_indices, list(out_shape), list(in_shape)
        self._plans = {}
        self.pair_bwd, self.cnt = pair_bwd, cnt
        self.ksize, self.stride, self.padding, self.dilation = ksize, stride, padding, dilation
        # static-capacity (graph) mode: live row counts stay on the device, n_in / n_out above are CAPACITIES
        self.d_n_in = self.d_n_out = None


# ------------------------------------------------------------------------------------------- voxelise

def voxelize(points, point_cloud_range, voxel_size, max_points, max_voxels, batch_size=1, batch_col=-1, xyz_col=0,
             feat_col=0, num_features=None, want_voxels=True, want_mean=True, sync=True, ws_precleared=False):
    """GPU hard voxelisation (+ fused MeanVFE).  Returns dict(voxels, coords[M,4], num_points, mean, M).

    sync=True: one host sync (reads M) and exact-size views.  sync=False (static-capacity / graph mode): no sync, every
    output keeps its capacity rows and the live count is the device tensor `d_num_voxels`.
    ws_precleared: SPX_WS_PRECLEARED — the caller filled ops.workspace() itself (see include/spx.h).
    Semantics: include/spx.h §1 / SURVEY.md §8a row a1.
    """
    _need_gpu(points)
    lib = _lib.load()
    points = points.contiguous().float()
    n, stride = points.shape
    c = (stride - feat_col) if num_features is None else int(num_features)
    rng = [float(x) for x in point_cloud_range]
    vs = [float(x) for x in voxel_size]
    grid = [int(round((rng[3 + j] - rng[j]) / vs[j])) for j in range(3)]
    cap = max(1, min(n, batch_size * max_voxels))
    dev = points.device
    voxels = torch.empty((cap, max_points, c), dtype=torch.float32, device=dev) if want_voxels else None
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    num = torch.empty((cap,), dtype=torch.int32, device=dev)
    mean = torch.empty((cap, c), dtype=torch.float32, device=dev) if want_mean else None
    # (count, status): with a host read the call gets its own status word next to the count, one copy fetches both;
    # without, device-side errors go to the sticky per-device word (check_status)
    buf = torch.zeros((2,), dtype=torch.int64, device=dev)
    d_m = buf[:1]
    d_st = ctypes.c_void_p(buf.data_ptr() + 8) if sync else _ptr(status_word(dev))
    wsb = lib.spx_voxelize_ws_bytes(n, batch_size, max_points)
    ws = workspace(dev, wsb)
    check(lib.spx_voxelize(_ptr(points), n, stride, xyz_col, feat_col, c, batch_col, batch_size, f_arr(rng), f_arr(vs),
                           i3(grid), max_points, max_voxels, _ptr(voxels), _ptr(coords), _ptr(num), _ptr(mean),
                           _ptr(d_m), cap, 1 if ws_precleared else 0, d_st, _ptr(ws), wsb, _stream(points)),
          "spx_voxelize")
    if not sync:
        return dict(voxels=voxels, coords=coords, num_points=num, mean=mean, num_voxels=None, d_num_voxels=d_m,
                    grid_size=grid)
    m = _count_and_status(buf, "spx_voxelize")
    return dict(voxels=None if voxels is None else voxels[:m], coords=coords[:m], num_points=num[:m],
                mean=None if mean is None else mean[:m], num_voxels=m, d_num_voxels=d_m, grid_size=grid)


def dynamic_voxelize(points, point_cloud_range, voxel_size, batch_size=1, batch_col=0, xyz_col=1, num_features=None,
                     max_voxels=None, sync=True):
    """Dynamic voxelisation + per-voxel mean (include/spx.h §1b; reference DynamicMeanVFE.forward).  Returns
    dict(features [M, C], coords [M, 4] (b, z, y, x), inverse [N] (voxel row of each point, -1 = out of range),
    num_voxels, d_num_voxels).  Voxels are sorted by the key ((b*X + cx)*Y + cy)*Z + cz."""
    _need_gpu(points)
    lib = _lib.load()
    points = points.contiguous().float()
    n, stride = points.shape
    c = (stride - xyz_col) if num_features is None else int(num_features)
    rng = [float(x) for x in point_cloud_range]
    vs = [float(x) for x in voxel_size]
    grid = [int(round((rng[3 + j] - rng[j]) / vs[j])) for j in range(3)]
    cap = max(1, n if max_voxels is None else min(n, int(max_voxels)))
    dev = points.device
    feats = torch.empty((cap, c), dtype=torch.float32, device=dev)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    inv = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    d_num = torch.zeros((1,), dtype=torch.int64, device=dev)
    g3 = i3(grid)
    wsb = lib.spx_dynamic_voxelize_ws_bytes(n, batch_size, g3, cap)
    ws = workspace(dev, wsb)
    check(lib.spx_dynamic_voxelize(_ptr(points), n, stride, batch_col, xyz_col, c, f_arr(rng), f_arr(vs), g3, batch_size,
                                   _ptr(feats), _ptr(coords), _ptr(inv), _ptr(d_num), cap, _ptr(ws), wsb, _stream(points)),
          "spx_dynamic_voxelize")
    out = {"d_num_voxels": d_num, "grid_size": grid}
    if sync:
        m = min(int(d_num.item()), cap)
        out.update(features=feats[:m], coords=coords[:m], inverse=inv[:n], num_voxels=m)
    else:
        out.update(features=feats, coords=coords, inverse=inv[:n], num_voxels=None)
    return out


def mean_vfe(voxels, num_points):
    _need_gpu(voxels, num_points)
    lib = _lib.load()
    voxels = voxels.contiguous().float()
    num = num_points.contiguous().to(torch.int32)
    n, t, c = voxels.shape
    out = torch.empty((n, c), dtype=torch.float32, device=voxels.device)
    check(lib.spx_mean_vfe(_ptr(voxels), _ptr(num), n, None, t, c, _ptr(out), _stream(voxels)), "spx_mean_vfe")
    return out


# ------------------------------------------------------------------------------------------- rulebooks

def subm_rulebook(indices, batch_size, spatial_shape, ksize, dilation=(1, 1, 1), want_cnt=False, d_n=None,
                  ws_precleared=False, unique=False):
    """d_n: optional device int64[1] live row count (<= indices.shape[0], which is then the capacity).  Device-side
    errors (only possible with ws_precleared on a dirty workspace) go to the sticky status word: check_status().
    unique: the caller guarantees one row per cell (SPX_ROWS_UNIQUE: half the table is probed, hits written twice)."""
    _need_gpu(indices)
    lib = _lib.load()
    indices = indices.contiguous()
    assert indices.dtype == torch.int32 and indices.shape[1] == 4
    n = indices.shape[0]
    K = int(ksize[0]) * int(ksize[1]) * int(ksize[2])
    dev = indices.device
    ld = max(n, 1)
    pair = torch.empty((K, ld), dtype=torch.int32, device=dev)
    cnt = torch.empty((K,), dtype=torch.int32, device=dev) if want_cnt else None   # zeroed by the library
    wsb = lib.spx_subm_rulebook_ws_bytes(n)
    ws = workspace(dev, wsb)
    check(lib.spx_subm_rulebook(_ptr(indices), n, _ptr(d_n), batch_size, i3(spatial_shape), i3(ksize), i3(dilation),
                                _ptr(pair), ld, _ptr(cnt), (1 if ws_precleared else 0) | (2 if unique else 0), _ptr(status_word(dev)),
                                _ptr(ws), wsb,
                                _stream(indices)), "spx_subm_rulebook")
    rb = Rulebook(pair, ld, n, n, K, True, indices, spatial_shape, spatial_shape, cnt=cnt, ksize=list(ksize),
                  stride=[1, 1, 1], padding=[k // 2 for k in ksize], dilation=list(dilation))
    rb.d_n_in = rb.d_n_out = d_n
    return rb


def conv_rulebook(indices, batch_size, spatial_shape, ksize, stride, padding, dilation=(1, 1, 1), want_cnt=False,
                  d_n_in=None, cap=None, sync=True, subm_ksize=None, subm_dilation=(1, 1, 1)):
    """Regular sparse conv rulebook.  subm_ksize: also build the SUBMANIFOLD table of the output level from the same rank
    bitmap (no hash for that level); it comes back as `rb.subm_next` (a Rulebook over rb.out_indices).  sync=True: one host sync (reads n_out), exact-size out_indices; sync="later": a
    PendingRulebook whose .finish() does that read.
    sync=False (static-capacity / graph mode): no sync; `cap` output rows (default: the no-overflow bound), live counts
    in rb.d_n_in / rb.d_n_out; rows beyond cap are dropped (overflow <=> rb.d_n_out > cap)."""
    _need_gpu(indices)
    lib = _lib.load()
    indices = indices.contiguous()
    assert indices.dtype == torch.int32 and indices.shape[1] == 4
    n_in = indices.shape[0]
    K = int(ksize[0]) * int(ksize[1]) * int(ksize[2])
    dev = indices.device
    out_shape = out_shape_of(spatial_shape, ksize, stride, padding, dilation)
    safe_cap = int(lib.spx_conv_out_cap(n_in, batch_size, i3(out_shape), i3(ksize), i3(stride)))
    cap = safe_cap if cap is None else max(1, min(int(cap), safe_cap))
    out_idx = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    pair_fwd = torch.empty((K, cap), dtype=torch.int32, device=dev)
    pair_bwd = torch.empty((K, max(n_in, 1)), dtype=torch.int32, device=dev)
    cnt = torch.empty((K,), dtype=torch.int32, device=dev) if want_cnt else None   # zeroed by the library
    d_n = torch.zeros((1,), dtype=torch.int64, device=dev)
    Ks = 0 if subm_ksize is None else int(subm_ksize[0]) * int(subm_ksize[1]) * int(subm_ksize[2])
    subm_pair = torch.empty((Ks, cap), dtype=torch.int32, device=dev) if Ks else None
    subm_cnt = torch.empty((Ks,), dtype=torch.int32, device=dev) if (Ks and want_cnt) else None
    wsb = lib.spx_conv_rulebook_ws_bytes(n_in, batch_size, i3(out_shape))
    ws = workspace(dev, wsb)
    # a capacity below the no-overflow bound can drop rows: the kernels say so in the sticky status word (check_status)
    d_st = _ptr(status_word(dev)) if cap < safe_cap else None
    check(lib.spx_conv_rulebook(_ptr(indices), n_in, _ptr(d_n_in), batch_size, i3(spatial_shape), i3(out_shape), i3(ksize),
                                i3(stride), i3(padding), i3(dilation), _ptr(out_idx), _ptr(pair_fwd), _ptr(pair_bwd),
                                _ptr(cnt), _ptr(d_n), cap, i3(subm_ksize) if Ks else None,
                                i3(subm_dilation) if Ks else None, _ptr(subm_pair), _ptr(subm_cnt), d_st, _ptr(ws), wsb,
                                _stream(indices)), "spx_conv_rulebook")

    def with_subm(rb):
        if Ks:
            n = rb.n_out
            nxt = Rulebook(subm_pair, cap, n, n, Ks, True, rb.out_indices, out_shape, out_shape, cnt=subm_cnt,
                           ksize=list(subm_ksize), stride=[1, 1, 1], padding=[k // 2 for k in subm_ksize],
                           dilation=list(subm_dilation))
            nxt.d_n_in = nxt.d_n_out = rb.d_n_out
            rb.subm_next = nxt
        return rb
    if not sync:
        rb = Rulebook(pair_fwd, cap, n_in, cap, K, False, out_idx, out_shape, spatial_shape, pair_bwd=pair_bwd, cnt=cnt,
                      ksize=list(ksize), stride=list(stride), padding=list(padding), dilation=list(dilation))
        rb.d_n_in, rb.d_n_out = d_n_in, d_n
        return with_subm(rb)
    if sync == "later":
        # The row count is read back asynchronously; .finish() waits for it.  A caller that launches this table one stage
        # early (before it queues the previous stage's kernels) finds the count already there: the host never waits on an
        # empty GPU (pcdet_amd/models/backbones_3d/spconv_backbone.py).
        return PendingRulebook(d_n, lambda n_out: with_subm(Rulebook(
            pair_fwd, cap, n_in, n_out, K, False, out_idx[:n_out], out_shape, spatial_shape, pair_bwd=pair_bwd, cnt=cnt,
            ksize=list(ksize), stride=list(stride), padding=list(padding), dilation=list(dilation))))
    n_out = int(d_n.item())
    rb = Rulebook(pair_fwd, cap, n_in, n_out, K, False, out_idx[:n_out], out_shape, spatial_shape, pair_bwd=pair_bwd,
                  cnt=cnt, ksize=list(ksize), stride=list(stride), padding=list(padding), dilation=list(dilation))
    return with_subm(rb)


class PendingRulebook(object):
    """A strided rule table whose kernels are queued and whose row count is on its way to the host."""

    _pool, _next = [], 0             # pinned host words, reused round-robin (pinning memory costs far more than the copy)

    def __init__(self, d_n, make):
        cls = PendingRulebook
        if len(cls._pool) < 16:
            cls._pool.append(torch.empty((1,), dtype=torch.int64).pin_memory())
            self._host = cls._pool[-1]
        else:
            self._host = cls._pool[cls._next % 16]
            cls._next += 1
        self._make = make
        self._host.copy_(d_n, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(d_n.device))
        self._d_n = d_n                          # keeps the source of the copy alive

    def finish(self):
        self._event.synchronize()
        return self._make(int(self._host[0]))


# ------------------------------------------------------------------------------------------- arithmetic

def pack_weight(weight, mode, out=None):
    """weight [Cout, kz, ky, kx, Cin] (or [Cout, K, Cin]) -> MFMA operand order.  mode 0 fwd, 1 dgrad, 2 both.  out: a buffer
    of a previous call with the same weight shape and mode, refilled in place."""
    _need_gpu(weight)
    lib = _lib.load()
    w = weight.detach().contiguous().float()
    cout, cin = w.shape[0], w.shape[-1]
    K = w.numel() // (cout * cin)
    n = (2 if mode == 2 else 1) * K * cin * cout
    packed = out if out is not None else torch.empty((n,), dtype=torch.float32, device=w.device)
    assert packed.numel() == n and packed.is_contiguous() and packed.device == w.device
    check(lib.spx_pack_weight(_ptr(w), cout, K, cin, mode, _ptr(packed), _stream(w)), "spx_pack_weight")
    return packed                # mode 2: forward operand in the first half, dgrad operand in the second


class PackedBank(object):
    """Both MFMA operand orders of a fixed list of contiguous weights, re-packed by ONE launch (spx_pack_weight_batched).
    halves(i) -> (forward operand, dgrad operand) views of weight i."""

    def __init__(self, weights):
        self.weights = list(weights)
        dev = self.weights[0].device
        sizes = [w.numel() for w in self.weights]
        self.flat = torch.empty((2 * sum(sizes),), dtype=torch.float32, device=dev)
        rows, off, blk = [], 0, 0
        self.views = []
        for w, n in zip(self.weights, sizes):
            cout, cin = w.shape[0], w.shape[-1]
            rows.append([w.data_ptr(), self.flat.data_ptr() + 4 * off, cout, n // (cout * cin), cin, blk])
            self.views.append((self.flat[off:off + n], self.flat[off + n:off + 2 * n]))
            off += 2 * n
            blk += (2 * n + 255) // 256
        self.blocks = blk
        self.desc = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.ptrs = tuple(w.data_ptr() for w in self.weights)

    def valid_for(self, weights):
        return len(weights) == len(self.weights) and tuple(w.data_ptr() for w in weights) == self.ptrs

    def repack(self):
        check(_lib.load().spx_pack_weight_batched(_ptr(self.desc), len(self.weights), self.blocks, _stream(self.flat)),
              "spx_pack_weight_batched")


def conv_gemm(src, w_packed, c_dst, kvol, pair, ld, n_dst, flip_k=False, scale=None, shift=None, relu=False,
              d_n_dst=None):
    """d_n_dst: optional device int64[1] live destination-row count (n_dst is then the launch capacity; rows beyond the
    live count are not written)."""
    _need_gpu(src, w_packed, pair)
    lib = _lib.load()
    src = src.contiguous()
    assert src.dtype == torch.float32
    dst = torch.empty((n_dst, c_dst), dtype=torch.float32, device=src.device)
    if n_dst == 0:
        return dst
    if src.shape[0] == 0:
        return dst.zero_()
    check(lib.spx_conv_gemm(_ptr(src), src.shape[1], _ptr(w_packed), c_dst, kvol, int(bool(flip_k)), _ptr(pair), ld,
                            n_dst, _ptr(d_n_dst), _ptr(scale), _ptr(shift), int(bool(relu)), _ptr(dst), _stream(src)),
          "spx_conv_gemm")
    return dst


_BALANCED_SHAPES = {(64, 64)}   # measured: 32x32 slower, 32x64 / 64x32 even (plan cost included)
if os.environ.get("SPX_CONV_BALANCED_SHAPES"):   # dev knob: "32x32,32x64,64x32,64x64"
    _BALANCED_SHAPES = {tuple(int(v) for v in t.split("x")) for t in os.environ["SPX_CONV_BALANCED_SHAPES"].split(",")}
# below this many destination rows the plan / fix-up launches cost more than the balanced schedule saves
_BALANCED_MIN_ROWS = int(os.environ.get("SPX_CONV_BALANCED_MIN_ROWS", "24000"))
_BALANCED = os.environ.get("SPX_CONV_BALANCED", "1") != "0"
_GROUPED = os.environ.get("SPX_CONV_GROUPED", "1") != "0"       # dev knob: rows grouped by offset mask (csrc/conv_group.hip)


def conv_plan(pair, ld, kvol, n_dst, d_n_dst=None):
    """Work plan of the balanced schedule for one rule table (include/spx.h: spx_conv_plan); int32 device tensor."""
    _need_gpu(pair)
    lib = _lib.load()
    plan = torch.empty((lib.spx_conv_plan_bytes(n_dst) // 4,), dtype=torch.int32, device=pair.device)
    check(lib.spx_conv_plan(_ptr(pair), ld, kvol, n_dst, _ptr(d_n_dst), _ptr(plan), _stream(pair)), "spx_conv_plan")
    return plan


def conv_group(pair, ld, kvol, n_dst, d_n_dst=None):
    """Rows of a rule table grouped by offset mask (include/spx.h: spx_conv_group) -> perm [n_dst] int32 and the table
    in that order [kvol, n_dst] int32."""
    _need_gpu(pair)
    lib = _lib.load()
    perm = torch.empty((n_dst,), dtype=torch.int32, device=pair.device)
    grouped = torch.empty((kvol, n_dst), dtype=torch.int32, device=pair.device)
    wsb = lib.spx_conv_group_ws_bytes(n_dst)
    ws = workspace(pair.device, wsb)
    check(lib.spx_conv_group(_ptr(pair), ld, kvol, n_dst, _ptr(d_n_dst), _ptr(perm), _ptr(grouped), _ptr(ws), wsb,
                             _stream(pair)), "spx_conv_group")
    return perm, grouped


def grouped_plan_for(rb, pair, ld, kvol, n_dst, d_n_dst=None):
    """(perm, grouped table, plan over it) of rule table `pair`, built once per Rulebook and table."""
    key = ("g", pair.data_ptr(), int(n_dst))
    hit = rb._plans.get(key)
    if hit is None:
        perm, grouped = conv_group(pair, ld, kvol, n_dst, d_n_dst)
        hit = rb._plans[key] = (perm, grouped, conv_plan(grouped, n_dst, kvol, n_dst, d_n_dst))
    return hit


def plan_for(rb, pair, ld, kvol, n_dst, d_n_dst=None):
    """Plan of rule table `pair`, built once per Rulebook and table (forward, dgrad and sibling layers share it)."""
    key = (pair.data_ptr(), int(n_dst))
    plan = rb._plans.get(key)
    if plan is None:
        plan = rb._plans[key] = conv_plan(pair, ld, kvol, n_dst, d_n_dst)
    return plan


def grouped_ok(rb, kvol):
    """Grouping the rows costs one sort per rule table: worth it for submanifold tables (forward and dgrad of two
    layers read the same one), not for the single-use tables of strided convolutions."""
    return _GROUPED and rb.subm and kvol <= 30


def balanced_ok(c_src, c_dst, n_dst, rb=None, pair=None):
    if not _BALANCED or n_dst < _BALANCED_MIN_ROWS:
        return False
    if (c_src, c_dst) in _BALANCED_SHAPES:
        return True
    # 128 -> 128: the two-half kernel (k_conv_mfma_pbl2) beats one tile per wave on tables whose 64-row super-tiles
    # really share their offsets — the forward table of the BEV entry conv (313 -> 209 us); on its backward table, where
    # every row has 9 of the 18 offsets, it loses (185 vs 165 us).  The caller marks the rulebook.
    return (c_src, c_dst) == (128, 128) and rb is not None and getattr(rb, "wide_balanced_fwd", False) and pair is rb.pair


def conv_gemm_balanced(src, w_packed, c_dst, kvol, pair, ld, n_dst, plan, flip_k=False, scale=None, shift=None,
                       relu=False, d_n_dst=None, perm=None):
    """conv_gemm under the MFMA-work-balanced persistent schedule (`plan` from conv_plan on the same table / n_dst)."""
    _need_gpu(src, w_packed, pair, plan)
    lib = _lib.load()
    src = src.contiguous()
    assert src.dtype == torch.float32 and n_dst > 0 and src.shape[0] > 0
    dst = torch.empty((n_dst, c_dst), dtype=torch.float32, device=src.device)
    wsb = lib.spx_conv_gemm_balanced_ws_bytes(c_dst, n_dst)
    ws = workspace(src.device, wsb)
    check(lib.spx_conv_gemm_balanced(_ptr(src), src.shape[1], _ptr(w_packed), c_dst, kvol, int(bool(flip_k)), _ptr(pair),
                                     ld, n_dst, _ptr(d_n_dst), _ptr(scale), _ptr(shift), int(bool(relu)), _ptr(plan),
                                     _ptr(perm), _ptr(dst), _ptr(ws), wsb, _stream(src)), "spx_conv_gemm_balanced")
    return dst


_RING = os.environ.get("SPX_CONV_RING", "1") != "0"              # dev knob: round-3 schedule (csrc/conv_ring.hip)
# 32x32 / 32x64 / 64x32 are built too and 15-25 % faster than the one-tile-per-wave kernels launch by launch (kbench --ring),
# but the training step gets SLOWER with them (299.9 vs 303.7 frames/s, same call): four more plans on the index stream and
# 1024-thread persistent workgroups that have to wait for whole CUs beside the side-stream weight-gradient kernels
_RING_SHAPES = {(64, 64)}
if os.environ.get("SPX_CONV_RING_SHAPES"):                       # dev knob: "32x32,32x64,64x32,64x64"
    _RING_SHAPES = {tuple(int(v) for v in t.split("x")) for t in os.environ["SPX_CONV_RING_SHAPES"].split(",")}
_RING_MIN_ROWS = int(os.environ.get("SPX_CONV_RING_MIN_ROWS", "24000"))


def ring_ok(c_src, c_dst, n_dst, kvol):
    return _RING and (c_src, c_dst) in _RING_SHAPES and n_dst >= _RING_MIN_ROWS and kvol <= 31


def conv_ring_plan(pair, ld, kvol, n_dst, d_n_dst=None):
    """Tile -> wave assignment of the ring schedule for one rule table (include/spx.h: spx_conv_ring_plan)."""
    _need_gpu(pair)
    lib = _lib.load()
    plan = torch.empty((lib.spx_conv_ring_plan_bytes(n_dst) // 4,), dtype=torch.int32, device=pair.device)
    check(lib.spx_conv_ring_plan(_ptr(pair), ld, kvol, n_dst, _ptr(d_n_dst), _ptr(plan), _stream(pair)),
          "spx_conv_ring_plan")
    return plan


def ring_plan_for(rb, pair, ld, kvol, n_dst, d_n_dst=None):
    """(perm, table, ring plan) of rule table `pair`, built once per Rulebook and table: over the grouped rows for submanifold
    tables (perm != None), over the plain table otherwise."""
    key = ("r", pair.data_ptr(), int(n_dst))
    hit = rb._plans.get(key)
    if hit is None:
        if grouped_ok(rb, kvol):
            gkey = ("g", pair.data_ptr(), int(n_dst))
            ghit = rb._plans.get(gkey)
            if ghit is not None:
                perm, grouped = ghit[0], ghit[1]
            else:
                perm, grouped = conv_group(pair, ld, kvol, n_dst, d_n_dst)
            hit = (perm, grouped, n_dst, conv_ring_plan(grouped, n_dst, kvol, n_dst, d_n_dst))
        else:
            hit = (None, pair, ld, conv_ring_plan(pair, ld, kvol, n_dst, d_n_dst))
        rb._plans[key] = hit
    return hit


def conv_gemm_ring(src, w_packed, c_dst, kvol, pair, ld, n_dst, plan, flip_k=False, scale=None, shift=None, relu=False,
                   d_n_dst=None, perm=None, want_stats=False):
    """conv_gemm under the ring schedule (`plan` from conv_ring_plan on the same table / n_dst).  want_stats: also return the
    per-workgroup column sums [rows, 2, c_dst] of the written values and their squares."""
    _need_gpu(src, w_packed, pair, plan)
    lib = _lib.load()
    src = src.contiguous()
    assert src.dtype == torch.float32 and n_dst > 0 and src.shape[0] > 0
    dst = torch.empty((n_dst, c_dst), dtype=torch.float32, device=src.device)
    stats = None
    if want_stats:
        stats = torch.empty((lib.spx_conv_ring_stat_rows(), 2, c_dst), dtype=torch.float32, device=src.device)
    check(lib.spx_conv_gemm_ring(_ptr(src), src.shape[0], src.shape[1], _ptr(w_packed), c_dst, kvol, int(bool(flip_k)),
                                 _ptr(pair), ld, n_dst, _ptr(d_n_dst), _ptr(scale), _ptr(shift), int(bool(relu)), _ptr(plan),
                                 _ptr(perm), _ptr(dst), _ptr(stats), _ptr(status_word(src.device)), _stream(src)),
          "spx_conv_gemm_ring")
    return (dst, stats) if want_stats else dst


def wgrad_counts(pair, ld, kvol, n_out, d_n_out=None):
    """Pair counts of a rule table for conv_wgrad's work split (include/spx.h: spx_conv_wgrad_counts); int32 device tensor."""
    _need_gpu(pair)
    lib = _lib.load()
    counts = torch.empty((lib.spx_conv_wgrad_counts_bytes(kvol, n_out) // 4,), dtype=torch.int32, device=pair.device)
    check(lib.spx_conv_wgrad_counts(_ptr(pair), ld, kvol, n_out, _ptr(d_n_out), _ptr(counts), _stream(pair)),
          "spx_conv_wgrad_counts")
    return counts


def wgrad_counts_for(rb, pair, ld, kvol, n_out, d_n_out=None):
    """Counts of rule table `pair`, computed once per Rulebook (shared by the layers that use the table)."""
    key = ("wc", pair.data_ptr(), int(n_out))
    hit = rb._plans.get(key)
    if hit is None:
        hit = rb._plans[key] = wgrad_counts(pair, ld, kvol, n_out, d_n_out)
    return hit


_WGRAD_MAX_C = 128      # spx_conv_wgrad's channel limit per side


def conv_wgrad(feat_in, dout, pair, ld, n_out, wshape, d_n_out=None, counts=None):
    """d_n_out: optional device int64[1] live output-row count (n_out is then the capacity); counts: wgrad_counts of the
    table (computed inside the call when None)."""
    _need_gpu(feat_in, dout, pair)
    lib = _lib.load()
    feat_in = feat_in.contiguous()
    dout = dout.contiguous()
    cout, cin = wshape[0], wshape[-1]
    K = 1
    for s in wshape[1:-1]:
        K *= int(s)
    dw = torch.empty(tuple(wshape), dtype=torch.float32, device=dout.device)
    if feat_in.shape[0] == 0 or n_out == 0:
        return dw.zero_()
    if cin > _WGRAD_MAX_C or cout > _WGRAD_MAX_C:
        # the kernel takes up to 128 channels a side; dw[o, k, i] reads only feat_in[:, i] and dout[:, o], so wider
        # layers (the voxel-point SA U-Net's 256) run as channel tiles with the same per-element arithmetic
        for o0 in range(0, cout, _WGRAD_MAX_C):
            o1 = min(o0 + _WGRAD_MAX_C, cout)
            for i0 in range(0, cin, _WGRAD_MAX_C):
                i1 = min(i0 + _WGRAD_MAX_C, cin)
                dw[o0:o1, ..., i0:i1] = conv_wgrad(feat_in[:, i0:i1], dout[:, o0:o1], pair, ld, n_out,
                                                   (o1 - o0,) + tuple(wshape[1:-1]) + (i1 - i0,), d_n_out=d_n_out,
                                                   counts=counts)
        return dw
    wsb = lib.spx_conv_wgrad_ws_bytes(cin, cout, K, n_out)
    ws = workspace(dout.device, wsb)
    check(lib.spx_conv_wgrad(_ptr(feat_in), cin, _ptr(dout), cout, K, _ptr(pair), ld, n_out, _ptr(d_n_out), _ptr(counts),
                             _ptr(dw), _ptr(ws),
                             wsb, _stream(dout)), "spx_conv_wgrad")
    return dw


# ------------------------------------------------------------------------------------------- densify

def densify(features, indices, batch_size, spatial_shape, channels_last=False, d_n=None):
    """[N,C] -> logical [B,C,D,H,W].  channels_last=True stores it as [B,H,W,C,D] (see include/spx.h §5).
    d_n: optional device int64[1] live row count."""
    _need_gpu(features, indices)
    lib = _lib.load()
    features = features.contiguous()
    n, c = features.shape
    d, h, w = [int(s) for s in spatial_shape]
    dev = features.device
    if channels_last:
        dense = torch.zeros((batch_size, h, w, c, d), dtype=torch.float32, device=dev)
    else:
        dense = torch.zeros((batch_size, c, d, h, w), dtype=torch.float32, device=dev)
    check(lib.spx_densify(_ptr(features), _ptr(indices), n, _ptr(d_n), c, batch_size, i3(spatial_shape),
                          1 if channels_last else 0, _ptr(dense), _stream(features)), "spx_densify")
    return dense.permute(0, 3, 4, 1, 2) if channels_last else dense


def densify_bwd(ddense, indices, batch_size, spatial_shape, channels_last=False, d_n=None):
    _need_gpu(ddense, indices)
    lib = _lib.load()
    n = indices.shape[0]
    c = ddense.shape[1]
    if channels_last:
        dd = ddense.permute(0, 3, 4, 1, 2).contiguous()  # -> [B,H,W,C,D] storage
    else:
        dd = ddense.contiguous()
    dfeat = torch.empty((n, c), dtype=torch.float32, device=ddense.device)
    check(lib.spx_densify_bwd(_ptr(dd), _ptr(indices), n, _ptr(d_n), c, batch_size, i3(spatial_shape),
                              1 if channels_last else 0, _ptr(dfeat), _stream(ddense)), "spx_densify_bwd")
    return dfeat


# ------------------------------------------------------------------------------------------- rotated BEV IoU / NMS

def boxes_iou_bev(boxes_a, boxes_b, overlap_only=False):
    """(N,7),(M,7) [x,y,z,dx,dy,dz,heading] -> (N,M) BEV IoU (or intersection area)."""
    _need_gpu(boxes_a, boxes_b)
    lib = _lib.load()
    a = boxes_a[:, :7].contiguous().float()
    b = boxes_b[:, :7].contiguous().float()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    check(lib.spx_boxes_iou_bev(_ptr(a), a.shape[0], _ptr(b), b.shape[0], int(bool(overlap_only)), _ptr(out), _stream(a)),
          "spx_boxes_iou_bev")
    return out


def nms_bev(boxes_sorted, thresh, axis_aligned=False):
    """boxes (N,7) already sorted by descending score -> (keep positions int64 [N] on device, count tensor int64[1]).
    No host sync here; the caller slices keep[:count]."""
    _need_gpu(boxes_sorted)
    lib = _lib.load()
    b = boxes_sorted[:, :7].contiguous().float()
    n = b.shape[0]
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=b.device)
    cnt = torch.zeros((1,), dtype=torch.int64, device=b.device)
    wsb = lib.spx_nms_ws_bytes(n)
    ws = workspace(b.device, wsb)
    check(lib.spx_nms_bev(_ptr(b), n, float(thresh), int(bool(axis_aligned)), _ptr(keep), _ptr(cnt), _ptr(ws), wsb,
                          _stream(b)), "spx_nms_bev")
    return keep, cnt


# ------------------------------------------------------------------------------------------- anchor target assignment

def assign_targets(anchors, per_location, gt_boxes, set_class, n_classes, matched, unmatched):
    """anchors [n_sets, A, 7] fp32, gt_boxes [B, M, 8] fp32, set_class int32[n_sets], matched/unmatched fp32[n_sets]
    (all on the GPU) -> labels int32 [B, n_sets*A], targets fp32 [B, n_sets*A, 7], weights fp32 [B, n_sets*A]
    in the head's (y, x, set, within-location) anchor order.  No host sync."""
    _need_gpu(anchors, gt_boxes, set_class, matched, unmatched)
    lib = _lib.load()
    n_sets, a, _ = anchors.shape
    gt = gt_boxes.contiguous().float()
    b, m = gt.shape[0], gt.shape[1]
    dev = gt.device
    labels = torch.empty((b, n_sets * a), dtype=torch.int32, device=dev)
    targets = torch.empty((b, n_sets * a, 7), dtype=torch.float32, device=dev)
    weights = torch.empty((b, n_sets * a), dtype=torch.float32, device=dev)
    wsb = lib.spx_assign_targets_ws_bytes(b, n_sets, m)
    ws = workspace(dev, wsb)
    check(lib.spx_assign_targets(_ptr(anchors), n_sets, a, int(per_location), _ptr(gt), b, m, _ptr(set_class),
                                 int(n_classes), _ptr(matched), _ptr(unmatched), _ptr(labels), _ptr(targets),
                                 _ptr(weights), _ptr(ws), wsb, _stream(gt)), "spx_assign_targets")
    return labels, targets, weights


# ------------------------------------------------------------------------------------------- anchor-head losses

def anchor_loss(cls_preds, box_preds, dir_preds, labels, reg_targets, anchors, dir_offset, cls_weight, loc_weight,
                dir_weight, beta=1.0 / 9.0, alpha=0.25):
    """cls_preds [B,A,NC], box_preds [B,A,7], dir_preds [B,A,NB] or None, labels int32 [B,A], reg_targets [B,A,7],
    anchors [A,7] -> (losses fp32[3] = weighted cls/loc/dir, dcls, dbox, ddir).  No host sync."""
    _need_gpu(cls_preds, box_preds, labels, reg_targets, anchors)
    lib = _lib.load()
    cls_preds, box_preds = cls_preds.contiguous().float(), box_preds.contiguous().float()
    dir_c = None if dir_preds is None else dir_preds.contiguous().float()
    labels = labels.contiguous()
    assert labels.dtype == torch.int32
    reg_targets, anchors = reg_targets.contiguous().float(), anchors.contiguous().float()
    b, a, nc = cls_preds.shape
    nb = 0 if dir_c is None else dir_c.shape[2]
    dev = cls_preds.device
    losses = torch.zeros((3,), dtype=torch.float32, device=dev)
    dcls, dbox = torch.empty_like(cls_preds), torch.empty_like(box_preds)
    ddir = None if dir_c is None else torch.empty_like(dir_c)
    wsb = lib.spx_anchor_loss_ws_bytes(b, a)
    ws = workspace(dev, wsb)
    check(lib.spx_anchor_loss(_ptr(cls_preds), _ptr(box_preds), _ptr(dir_c), _ptr(labels), _ptr(reg_targets),
                              _ptr(anchors), b, a, nc, nb, float(dir_offset), float(cls_weight), float(loc_weight),
                              float(dir_weight), float(beta), float(alpha), _ptr(losses), _ptr(dcls), _ptr(dbox),
                              _ptr(ddir), _ptr(ws), wsb, _stream(cls_preds)), "spx_anchor_loss")
    return losses, dcls, dbox, ddir


# ------------------------------------------------------------------------------------------- BatchNorm1d (+ReLU), training

def bn_relu_supported(c):
    return c % 4 == 0 and 1024 % c == 0


def _row_view_ok(t, n, c):
    """[n, c] float32 view whose rows are contiguous and 16-byte aligned at a row stride that is a multiple of 4."""
    return (t.dim() == 2 and tuple(t.shape) == (n, c) and t.dtype == torch.float32 and (n <= 1 or t.stride(0) % 4 == 0)
            and (c == 1 or t.stride(1) == 1) and t.stride(0) >= c and t.data_ptr() % 16 == 0)


def bn_relu_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None, out=None,
                num_batches_tracked=None, d_n=None):
    """Training-mode BatchNorm1d over the rows of x [N, C] (+ residual) (+ReLU).  Updates running_mean / running_var
    (and num_batches_tracked, when given) in place.  `out`: optional [N, C] view with its own row stride (a channel
    slice of a wider matrix) that receives y.  Returns y, save_mean, save_invstd."""
    _need_gpu(x, gamma, beta)
    lib = _lib.load()
    x = x.contiguous()
    n, c = x.shape
    if residual is not None:
        residual = residual.contiguous()
        if residual.shape != x.shape or residual.dtype != x.dtype or residual.device != x.device:
            raise ValueError("residual must match x: %s vs %s" % (tuple(residual.shape), tuple(x.shape)))
    if out is None:
        y = torch.empty_like(x)
    else:
        if not (_row_view_ok(out, n, c) and out.device == x.device):
            raise ValueError("out must be a float32 [N, C] row view (row stride a multiple of 4, 16-byte aligned)")
        y = out
    y_ld = y.stride(0) if n > 1 else c
    mean = torch.empty((c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty((c,), dtype=torch.float32, device=x.device)
    wsb = lib.spx_bn_relu_ws_bytes(c)
    ws = workspace(x.device, wsb)
    check(lib.spx_bn_add_relu_fwd(_ptr(x), _ptr(residual), n, _ptr(d_n), c, _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                  _ptr(running_var), _ptr(num_batches_tracked), float(momentum), float(eps),
                                  int(bool(relu)), _ptr(y), y_ld, _ptr(mean), _ptr(invstd), _ptr(ws), wsb, _stream(x)),
          "spx_bn_add_relu_fwd")
    return y, mean, invstd


def bn_relu_fwd_from_sums(x, partial, gamma, beta, running_mean, running_var, momentum, eps, relu, num_batches_tracked=None,
                          d_n=None):
    """bn_relu_fwd for rows x [N, C] whose per-block sums [rows, 2, C] the producing kernel already took (conv2d_wino with
    stats=True, conv_gemm_ring with want_stats=True): no statistics pass over x.  d_n: device-side live row count of a
    static-capacity x.  Returns y, save_mean, save_invstd."""
    _need_gpu(x, partial, gamma, beta)
    lib = _lib.load()
    x = x.contiguous()
    n, c = x.shape
    assert partial.dim() == 3 and partial.shape[1] == 2 and partial.shape[2] == c and partial.is_contiguous()
    y = torch.empty_like(x)
    mean = torch.empty((c,), dtype=torch.float32, device=x.device)
    invstd = torch.empty((c,), dtype=torch.float32, device=x.device)
    check(lib.spx_bn_relu_fwd_from_sums(_ptr(x), n, _ptr(d_n), c, _ptr(partial), int(partial.shape[0]), _ptr(gamma), _ptr(beta),
                                        _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), float(momentum),
                                        float(eps), int(bool(relu)), _ptr(y), c, _ptr(mean), _ptr(invstd), _stream(x)),
          "spx_bn_relu_fwd_from_sums")
    return y, mean, invstd


def bn_apply(x, mean, invstd, gamma, beta, relu, residual=None, out=None, d_n=None):
    """Inference-mode BatchNorm (+ residual) (+ReLU) over the rows of x [N, C] with given statistics, one pass.  `out`:
    optional [N, C] row view with its own stride (a channel slice of a wider matrix)."""
    _need_gpu(x, mean, invstd, gamma, beta)
    lib = _lib.load()
    x = x.contiguous()
    n, c = x.shape
    if out is None:
        y = torch.empty_like(x)
    else:
        if not (_row_view_ok(out, n, c) and out.device == x.device):
            raise ValueError("out must be a float32 [N, C] row view (row stride a multiple of 4, 16-byte aligned)")
        y = out
    y_ld = y.stride(0) if n > 1 else c
    if residual is not None:
        residual = residual.contiguous()
    check(lib.spx_bn_apply(_ptr(x), _ptr(residual), n, _ptr(d_n), c, _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta),
                           int(bool(relu)), _ptr(y), y_ld, _stream(x)), "spx_bn_apply")
    return y


def wino_ok(cin, cout):
    """Channel counts spx_conv2d_wino takes (else the caller keeps the vendor convolution)."""
    return cin % 32 == 0 and cout % 128 == 0


def wino_weight(weight, flip=False, out=None):
    """Transformed weight image of a [Cout, Cin, 3, 3] filter (any strides) for conv2d_wino.  flip: the image of the DATA
    GRADIENT's filter (taps rotated, channel roles swapped) — conv2d_wino(dy, wino_weight(w, flip=True)) = dx.
    out: a buffer of a previous call for the same shape to refill instead of allocating."""
    _need_gpu(weight)
    assert weight.dim() == 4 and weight.shape[2] == 3 and weight.shape[3] == 3 and weight.dtype == torch.float32
    lib = _lib.load()
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    k_in, k_out = (cout, cin) if flip else (cin, cout)
    nfl = lib.spx_wino_weight_floats(k_in, k_out)
    if out is not None and out.numel() == nfl and out.device == weight.device and out.dtype == torch.float32:
        u = out
    else:
        u = torch.empty((nfl,), dtype=torch.float32, device=weight.device)
    so, si, sa, sb = weight.stride()
    check(lib.spx_wino_weight(_ptr(weight), so, si, sa, sb, k_in, k_out, int(bool(flip)), _ptr(u), _stream(weight)),
          "spx_wino_weight")
    return u


def conv2d_wino(x, u, cout, scale=None, shift=None, relu=False, out=None, stats=False):
    """3x3 / stride 1 / pad 1 convolution of a channels-last map.  x: [N, Cin, H, W] tensor in channels_last memory format
    (or any [N, Cin, H, W] view whose pixels are dense rows: stride (H*W*ld, 1, W*ld, ld)); u: wino_weight image;
    returns [N, cout, H, W] channels_last (or writes `out`, same layout rule).  Optional epilogue relu?(y*scale + shift).
    stats=True: also returns the [rows, 2, cout] per-tile-block sums of y and y*y (bn_relu_fwd_from_sums takes them)."""
    _need_gpu(x, u)
    lib = _lib.load()
    n, cin, h, w = (int(v) for v in x.shape)
    x_ld = _cl_ld(x)
    if x_ld is None:
        x = x.contiguous(memory_format=torch.channels_last)
        x_ld = _cl_ld(x)
    if out is None:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    y_ld = _cl_ld(out)
    if y_ld is None or tuple(out.shape) != (n, cout, h, w):
        raise ValueError("out must be a float32 [N, Cout, H, W] channels-last map")
    if u.numel() != lib.spx_wino_weight_floats(cin, cout):
        raise ValueError("weight image does not match Cin=%d, Cout=%d" % (cin, cout))
    part = None
    if stats:
        part = torch.empty((lib.spx_wino_stat_rows(n, h, w), 2, cout), dtype=torch.float32, device=x.device)
    check(lib.spx_conv2d_wino(_ptr(x), x_ld, _ptr(u), n, h, w, cin, cout, _ptr(scale), _ptr(shift), int(bool(relu)),
                              _ptr(out), y_ld, _ptr(part), _stream(x)), "spx_conv2d_wino")
    return (out, part) if stats else out


def wino_wgrad_ok(cin, cout, w):
    """Shapes spx_conv2d_wino_wgrad takes (else the caller keeps the vendor weight-gradient kernel)."""
    return cin % 128 == 0 and cout % 128 == 0 and (w + 1) // 2 >= 8


def conv2d_wino_wgrad(x, dy, like):
    """Weight gradient of conv2d(x, w, padding=1) for a [Cout, Cin, 3, 3] weight, written with the strides of `like`.
    x [N, Cin, H, W], dy [N, Cout, H, W]: channels-last maps (see conv2d_wino)."""
    _need_gpu(x, dy)
    lib = _lib.load()
    n, cin, h, w = (int(v) for v in x.shape)
    cout = int(dy.shape[1])
    x_ld, dy_ld = _cl_ld(x), _cl_ld(dy)
    if x_ld is None:
        x = x.contiguous(memory_format=torch.channels_last)
        x_ld = _cl_ld(x)
    if dy_ld is None:
        dy = dy.contiguous(memory_format=torch.channels_last)
        dy_ld = _cl_ld(dy)
    assert tuple(like.shape) == (cout, cin, 3, 3) and tuple(dy.shape) == (n, cout, h, w)
    dw = torch.empty_like(like)
    so, si, sa, sb = dw.stride()
    wsb = lib.spx_wino_wgrad_ws_bytes(cin, cout)
    ws = workspace(x.device, wsb)
    check(lib.spx_conv2d_wino_wgrad(_ptr(x), x_ld, _ptr(dy), dy_ld, n, h, w, cin, cout, _ptr(dw), so, si, sa, sb, _ptr(ws), wsb,
                                    _stream(x)), "spx_conv2d_wino_wgrad")
    return dw


def _cl_ld(t):
    """Pixel pitch (floats) of a [N, C, H, W] float32 map whose memory is [N, H, W] rows of >= C channels, else None."""
    if t.dtype != torch.float32 or t.dim() != 4:
        return None
    n, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    ld = sw if w > 1 else (sh if h > 1 else c)
    if c > 1 and sc != 1:
        return None
    if ld < c or ld % 4 or t.data_ptr() % 16:
        return None
    if (w > 1 and sw != ld) or (h > 1 and sh != w * ld) or (n > 1 and sn != h * w * ld):
        return None
    return int(ld)


def bn_relu_bwd(x, dy, gamma, beta, mean, invstd, relu, residual=None, d_n=None):
    """Backward of bn_relu_fwd; the ReLU mask is recomputed from x (and the residual) inside the kernels (y is not
    read).  dy may be a row view with its own stride (a channel slice of a wider gradient).  Returns dx, dgamma, dbeta
    and, with a residual, dresidual."""
    _need_gpu(x, dy)
    lib = _lib.load()
    n, c = x.shape
    if not _row_view_ok(dy, n, c):
        dy = dy.contiguous()
    dy_ld = dy.stride(0) if n > 1 else c
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if residual is not None else None
    dgamma = torch.empty((c,), dtype=torch.float32, device=x.device)
    dbeta = torch.empty((c,), dtype=torch.float32, device=x.device)
    if n == 0:
        out = (dx, dgamma.zero_(), dbeta.zero_())
        return out if residual is None else out + (dres,)
    wsb = lib.spx_bn_relu_ws_bytes(c)
    ws = workspace(x.device, wsb)
    check(lib.spx_bn_add_relu_bwd(_ptr(x), _ptr(residual), _ptr(dy), dy_ld, n, _ptr(d_n), c, _ptr(gamma), _ptr(beta), _ptr(mean),
                                  _ptr(invstd), int(bool(relu)), _ptr(dx), _ptr(dres), _ptr(dgamma), _ptr(dbeta), _ptr(ws),
                                  wsb, _stream(x)), "spx_bn_add_relu_bwd")
    return (dx, dgamma, dbeta) if residual is None else (dx, dgamma, dbeta, dres)


# ------------------------------------------------------------------------------------------- voxel query (row f-4)

def voxel_query(new_xyz, xyz, new_coords, point_indices, nsample, radius, ranges):
    """Raw kernel result of include/spx.h §10: idx [M, nsample] int32 (slot 0 = -1 for empty balls) and cnt [M]."""
    _need_gpu(new_xyz, xyz, new_coords, point_indices)
    lib = _lib.load()
    new_xyz, xyz = new_xyz.contiguous().float(), xyz.contiguous().float()
    new_coords, point_indices = new_coords.contiguous().int(), point_indices.contiguous().int()
    m = new_coords.shape[0]
    b, z, y, x = point_indices.shape
    idx = torch.zeros((m, nsample), dtype=torch.int32, device=xyz.device)
    cnt = torch.zeros((m,), dtype=torch.int32, device=xyz.device)
    check(lib.spx_voxel_query(_ptr(new_xyz), _ptr(xyz), _ptr(new_coords), _ptr(point_indices), m, b, i3([z, y, x]),
                              int(nsample), float(radius), i3(ranges), _ptr(idx), _ptr(cnt), _stream(xyz)),
          "spx_voxel_query")
    return idx, cnt


def voxel_query_dilated(new_xyz, xyz, new_coords, point_indices, nsample, former_radius, radius, ranges, strides):
    """Raw kernel result of spx_voxel_query_dilated: idx [M, nsample] int32, cnt_unique [M] (occupied cells scanned) and
    idx_cnt [M] (slots filled before padding)."""
    _need_gpu(new_xyz, xyz, new_coords, point_indices)
    lib = _lib.load()
    new_xyz, xyz = new_xyz.contiguous().float(), xyz.contiguous().float()
    new_coords, point_indices = new_coords.contiguous().int(), point_indices.contiguous().int()
    m = new_coords.shape[0]
    b, z, y, x = point_indices.shape
    idx = torch.zeros((m, nsample), dtype=torch.int32, device=xyz.device)
    cnt = torch.zeros((m,), dtype=torch.int32, device=xyz.device)
    filled = torch.zeros((m,), dtype=torch.int32, device=xyz.device)
    check(lib.spx_voxel_query_dilated(_ptr(new_xyz), _ptr(xyz), _ptr(new_coords), _ptr(point_indices), m, b,
                                      i3([z, y, x]), int(nsample), float(former_radius), float(radius), i3(ranges),
                                      i3(strides), _ptr(idx), _ptr(cnt), _ptr(filled), _stream(xyz)),
          "spx_voxel_query_dilated")
    return idx, cnt, filled


# ------------------------------------------------------------------------------------------- point sampling (§11)

def _f32(t):
    return t.detach().contiguous().float()


def _i32(t):
    return t.detach().contiguous().int()


def furthest_point_sample(xyz, npoint, weights=None):
    """spx_furthest_point_sample: xyz (B, N, 3), weights (B, N) or None -> idx (B, npoint) int32."""
    _need_gpu(xyz, weights)
    lib = _lib.load()
    xyz = _f32(xyz)
    weights = None if weights is None else _f32(weights)
    b, n, _ = xyz.shape
    idx = torch.empty((b, int(npoint)), dtype=torch.int32, device=xyz.device)
    wsb = lib.spx_furthest_point_sample_ws_bytes(b, n)
    ws = workspace(xyz.device, wsb) if wsb else None
    check(lib.spx_furthest_point_sample(_ptr(xyz), _ptr(weights), b, n, int(npoint), _ptr(idx), _ptr(ws), wsb,
                                        _stream(xyz)), "spx_furthest_point_sample")
    return idx


def furthest_point_sample_matrix(matrix, npoint, weights=None):
    """spx_furthest_point_sample_matrix: matrix (B, N, N) pairwise distances, weights (B, N) or None -> idx (B, npoint)."""
    _need_gpu(matrix, weights)
    lib = _lib.load()
    matrix = _f32(matrix)
    weights = None if weights is None else _f32(weights)
    b, n, _ = matrix.shape
    idx = torch.empty((b, int(npoint)), dtype=torch.int32, device=matrix.device)
    wsb = lib.spx_furthest_point_sample_matrix_ws_bytes(b, n)
    ws = workspace(matrix.device, wsb)
    check(lib.spx_furthest_point_sample_matrix(_ptr(matrix), _ptr(weights), b, n, int(npoint), _ptr(idx), _ptr(ws), wsb,
                                               _stream(matrix)), "spx_furthest_point_sample_matrix")
    return idx


def ball_query(xyz, new_xyz, nsample, r_out, r_in=0.0):
    """spx_ball_query: -> idx_cnt (B, M), idx (B, M, nsample) int32 (hits r_in^2 <= d2 < r_out^2, padded cyclically)."""
    _need_gpu(xyz, new_xyz)
    lib = _lib.load()
    xyz, new_xyz = _f32(xyz), _f32(new_xyz)
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx_cnt = torch.empty((b, m), dtype=torch.int32, device=xyz.device)
    idx = torch.empty((b, m, int(nsample)), dtype=torch.int32, device=xyz.device)
    check(lib.spx_ball_query(_ptr(xyz), _ptr(new_xyz), b, n, m, float(r_in), float(r_out), int(nsample), _ptr(idx_cnt),
                             _ptr(idx), _stream(xyz)), "spx_ball_query")
    return idx_cnt, idx


def group_points(features, idx):
    """spx_group_points: features (B, C, N), idx (B, M, S) -> (B, C, M, S); idx (B, M) -> (B, C, M) (gather)."""
    _need_gpu(features, idx)
    lib = _lib.load()
    features, idx = _f32(features), _i32(idx)
    b, c, n = features.shape
    m, s = idx.shape[1], (idx.shape[2] if idx.dim() == 3 else 1)
    out = torch.empty((b, c) + tuple(idx.shape[1:]), dtype=torch.float32, device=features.device)
    check(lib.spx_group_points(_ptr(features), _ptr(idx), b, c, n, m, s, _ptr(out), _stream(features)), "spx_group_points")
    return out


def group_points_bwd(grad_out, idx, n):
    """spx_group_points_bwd: grad_out (B, C, M[, S]) -> grad_features (B, C, n), summed in a fixed order."""
    _need_gpu(grad_out, idx)
    lib = _lib.load()
    grad_out, idx = _f32(grad_out), _i32(idx)
    b, c = grad_out.shape[:2]
    m, s = idx.shape[1], (idx.shape[2] if idx.dim() == 3 else 1)
    grad = torch.empty((b, c, int(n)), dtype=torch.float32, device=grad_out.device)
    wsb = lib.spx_group_points_bwd_ws_bytes(b, n, m, s)
    ws = workspace(grad_out.device, wsb)
    check(lib.spx_group_points_bwd(_ptr(grad_out), _ptr(idx), b, c, int(n), m, s, _ptr(grad), _ptr(ws), wsb,
                                   _stream(grad_out)), "spx_group_points_bwd")
    return grad


def three_nn(unknown, known):
    """spx_three_nn: unknown (B, n, 3), known (B, m, 3) -> dist2 (B, n, 3) squared, idx (B, n, 3) int32."""
    _need_gpu(unknown, known)
    lib = _lib.load()
    unknown, known = _f32(unknown), _f32(known)
    b, n, _ = unknown.shape
    m = known.shape[1]
    dist2 = torch.empty((b, n, 3), dtype=torch.float32, device=unknown.device)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=unknown.device)
    check(lib.spx_three_nn(_ptr(unknown), _ptr(known), b, n, m, _ptr(dist2), _ptr(idx), _stream(unknown)), "spx_three_nn")
    return dist2, idx


def three_interpolate(features, idx, weight):
    """spx_three_interpolate: features (B, C, m), idx / weight (B, n, 3) -> (B, C, n)."""
    _need_gpu(features, idx, weight)
    lib = _lib.load()
    features, idx, weight = _f32(features), _i32(idx), _f32(weight)
    b, c, m = features.shape
    n = idx.shape[1]
    out = torch.empty((b, c, n), dtype=torch.float32, device=features.device)
    check(lib.spx_three_interpolate(_ptr(features), _ptr(idx), _ptr(weight), b, c, m, n, _ptr(out), _stream(features)),
          "spx_three_interpolate")
    return out


def three_interpolate_bwd(grad_out, idx, weight, m):
    """spx_three_interpolate_bwd: grad_out (B, C, n) -> grad_features (B, C, m), summed in a fixed order."""
    _need_gpu(grad_out, idx, weight)
    lib = _lib.load()
    grad_out, idx, weight = _f32(grad_out), _i32(idx), _f32(weight)
    b, c, n = grad_out.shape
    grad = torch.empty((b, c, int(m)), dtype=torch.float32, device=grad_out.device)
    wsb = lib.spx_three_interpolate_bwd_ws_bytes(b, m, n)
    ws = workspace(grad_out.device, wsb)
    check(lib.spx_three_interpolate_bwd(_ptr(grad_out), _ptr(idx), _ptr(weight), b, c, int(m), n, _ptr(grad), _ptr(ws), wsb,
                                        _stream(grad_out)), "spx_three_interpolate_bwd")
    return grad


# ------------------------------------------------------------------------- points in boxes, RoI-aware pooling (§12)

def points_in_boxes(points, boxes):
    """spx_points_in_boxes: points (B, M, 3), boxes (B, T, 7) -> (B, M) int32, the first box holding each point or -1."""
    _need_gpu(points, boxes)
    lib = _lib.load()
    points, boxes = _f32(points), _f32(boxes)
    b, m, _ = points.shape
    t = boxes.shape[1]
    out = torch.empty((b, m), dtype=torch.int32, device=points.device)
    check(lib.spx_points_in_boxes(_ptr(points), _ptr(boxes), b, m, t, _ptr(out), _stream(points)), "spx_points_in_boxes")
    return out


def roiaware_pool3d_fwd(rois, pts, feats, out_size, max_pts_each_voxel, pool_method):
    """spx_roiaware_pool3d_fwd: rois (N, 7), pts (P, 3), feats (P, C), out_size (ox, oy, oz), pool_method 0 = max / 1 = avg
    -> pooled (N, ox, oy, oz, C), argmax (same shape, int32; None for avg), pt_cell (N, P) and vox_cnt (N, ox, oy, oz)
    int32 (the record the backward reads)."""
    _need_gpu(rois, pts, feats)
    lib = _lib.load()
    rois, pts, feats = _f32(rois), _f32(pts), _f32(feats)
    n, npt, c = rois.shape[0], pts.shape[0], feats.shape[1]
    ox, oy, oz = (int(v) for v in out_size)
    dev = feats.device
    pooled = torch.empty((n, ox, oy, oz, c), dtype=torch.float32, device=dev)
    argmax = torch.empty((n, ox, oy, oz, c), dtype=torch.int32, device=dev) if pool_method == 0 else None
    pt_cell = torch.empty((n, npt), dtype=torch.int32, device=dev)
    vox_cnt = torch.empty((n, ox, oy, oz), dtype=torch.int32, device=dev)
    wsb = lib.spx_roiaware_pool3d_ws_bytes(n, npt, ox, oy, oz)
    ws = workspace(dev, wsb)
    check(lib.spx_roiaware_pool3d_fwd(_ptr(rois), _ptr(pts), _ptr(feats), n, npt, c, ox, oy, oz, int(max_pts_each_voxel),
                                      int(pool_method), _ptr(pooled), _ptr(argmax), _ptr(pt_cell), _ptr(vox_cnt), _ptr(ws),
                                      wsb, _stream(feats)), "spx_roiaware_pool3d_fwd")
    return pooled, argmax, pt_cell, vox_cnt


def roiaware_pool3d_bwd(grad_out, argmax, pt_cell, vox_cnt, pool_method):
    """spx_roiaware_pool3d_bwd: grad_out (N, ox, oy, oz, C) -> grad_in (P, C), summed over RoIs in ascending order."""
    _need_gpu(grad_out, argmax, pt_cell, vox_cnt)
    lib = _lib.load()
    grad_out = _f32(grad_out)
    n, ox, oy, oz, c = grad_out.shape
    npt = pt_cell.shape[1]
    grad_in = torch.empty((npt, c), dtype=torch.float32, device=grad_out.device)
    check(lib.spx_roiaware_pool3d_bwd(_ptr(grad_out), _ptr(None if argmax is None else _i32(argmax)), _ptr(_i32(pt_cell)),
                                      _ptr(_i32(vox_cnt)), n, npt, c, ox, oy, oz, int(pool_method), _ptr(grad_in),
                                      _stream(grad_out)), "spx_roiaware_pool3d_bwd")
    return grad_in


# ------------------------------------------------------------------------- gather-project (§13)

def group_project(p, wx, xyz, ctr, idx, empty, batch):
    """spx_group_project: p (N, Cout) = F · Wf^T or None, wx (Cout, 3) or None, xyz (N, 3), ctr (B * npoint, 3),
    idx (B * npoint, S) global source rows, empty (B * npoint) bool / uint8 or None -> y (B, Cout, npoint, S) with
    y = p[idx] + wx · (xyz[idx] - ctr), 0 in empty balls."""
    _need_gpu(p, wx, xyz, ctr, idx, empty)
    lib = _lib.load()
    ref = p if p is not None else wx
    p = None if p is None else _f32(p)
    wx = None if wx is None else _f32(wx)
    xyz = None if xyz is None else _f32(xyz)
    ctr = None if ctr is None else _f32(ctr)
    idx = _i32(idx)
    empty = None if empty is None else empty.detach().contiguous().to(torch.uint8)
    c_out = p.shape[1] if p is not None else wx.shape[0]
    n_src = p.shape[0] if p is not None else xyz.shape[0]
    m, s = idx.shape
    npoint = m // int(batch)
    assert npoint * int(batch) == m
    y = torch.empty((int(batch), c_out, npoint, s), dtype=torch.float32, device=ref.device)
    check(lib.spx_group_project(_ptr(p), _ptr(wx), _ptr(xyz), _ptr(ctr), _ptr(idx), _ptr(empty), c_out, n_src, int(batch),
                                npoint, s, _ptr(y), _stream(ref)), "spx_group_project")
    return y


def group_project_bwd(dy, xyz, ctr, idx, empty, n_src, need_dp=True, need_dwx=True):
    """spx_group_project_bwd: dy (B, Cout, npoint, S) -> dP^T (Cout, n_src) or None, dWx (Cout, 3) or None, both summed
    in a fixed order."""
    _need_gpu(dy, xyz, ctr, idx, empty)
    lib = _lib.load()
    dy = _f32(dy)
    b, c_out, npoint, s = dy.shape
    xyz = None if xyz is None else _f32(xyz)
    ctr = None if ctr is None else _f32(ctr)
    idx = _i32(idx)
    empty = None if empty is None else empty.detach().contiguous().to(torch.uint8)
    dpt = torch.empty((c_out, int(n_src)), dtype=torch.float32, device=dy.device) if need_dp else None
    dwx = torch.empty((c_out, 3), dtype=torch.float32, device=dy.device) if need_dwx else None
    wsb = lib.spx_group_project_bwd_ws_bytes(c_out, int(n_src), b, npoint, s)
    ws = workspace(dy.device, wsb)
    check(lib.spx_group_project_bwd(_ptr(dy), _ptr(xyz), _ptr(ctr), _ptr(idx), _ptr(empty), c_out, int(n_src), b, npoint,
                                    s, _ptr(dpt), _ptr(dwx), _ptr(ws), wsb, _stream(dy)), "spx_group_project_bwd")
    return dpt, dwx


# ------------------------------------------------------------------------------------------------ point head (§14)

def _point_mlp(params, c_in, c_out, device):
    """(w1 (H, c_in[, 1]), bn_mean, bn_var, bn_weight, bn_bias (H), eps, w2 (c_out, H[, 1]), b2 (c_out)) ->
    (spx_point_mlp, H, tensors to keep alive through the launch).  The pointers are the tensors' own storage when they
    are already contiguous float32 (a module's parameters are), so the kernel reads the current weights."""
    w1, mean, var, gamma, beta, eps, w2, b2 = params
    w1 = _f32(w1).reshape(w1.shape[0], -1)
    w2 = _f32(w2).reshape(w2.shape[0], -1)
    h = w1.shape[0]
    vecs = [_f32(t).reshape(-1) for t in (mean, var, gamma, beta)]
    b2 = _f32(b2).reshape(-1)
    if w1.shape[1] != c_in or tuple(w2.shape) != (c_out, h) or b2.numel() != c_out or any(v.numel() != h for v in vecs):
        raise _lib.SpxError("point-head MLP shapes do not chain: w1 %s, w2 %s, b2 %s, c_in %d, c_out %d"
                            % (tuple(w1.shape), tuple(w2.shape), tuple(b2.shape), c_in, c_out))
    keep = [w1] + vecs + [w2, b2]
    _need_gpu(*keep)
    if any(t.device != device for t in keep):
        raise _lib.SpxError("point-head MLP parameters are on another device than the features")
    desc = _lib.PointMlp(w1.data_ptr(), vecs[0].data_ptr(), vecs[1].data_ptr(), vecs[2].data_ptr(), vecs[3].data_ptr(),
                         float(eps), w2.data_ptr(), b2.data_ptr())
    return desc, h, keep


def point_vote(feat, xyz, lo, hi, mlp, max_range):
    """spx_point_vote: feat (B, C, N), xyz (B, N, 3), candidates are the columns [lo, hi) (clamped like a Python slice),
    mlp = (w1, bn_mean, bn_var, bn_weight, bn_bias, eps, w2, b2) of the C -> H -> 3 vote layers, max_range 3 floats ->
    vote (B, hi - lo, 3) = xyz[:, lo:hi] + clamp(offset, -max_range, max_range).  No autograd."""
    _need_gpu(feat, xyz)
    lib = _lib.load()
    feat, xyz = _f32(feat), _f32(xyz)
    b, c, n = feat.shape
    if tuple(xyz.shape) != (b, n, 3):
        raise _lib.SpxError("point_vote: xyz %s does not match features %s" % (tuple(xyz.shape), tuple(feat.shape)))
    lo, hi, _ = slice(int(lo), int(hi)).indices(n)
    hi = max(hi, lo)
    desc, h, keep = _point_mlp(mlp, c, 3, feat.device)
    vote = torch.empty((b, hi - lo, 3), dtype=torch.float32, device=feat.device)
    check(lib.spx_point_vote(_ptr(feat), _ptr(xyz), b, c, n, lo, hi, ctypes.byref(desc), h, f_arr(max_range),
                             _ptr(vote), _stream(feat)), "spx_point_vote")
    return vote


def point_head_predict(feat, stat, vote_xyz, cls_mlps, reg_mlp, bins):
    """spx_point_head_predict: feat (B, C, N), stat (num_class, C), vote_xyz (B * N, 3), cls_mlps a list of num_class
    (w1, bn_mean, bn_var, bn_weight, bn_bias, eps, w2, b2) tuples (C -> H -> 1, applied to feat * stat[k]), reg_mlp one
    (C -> H -> 6 + 2 * bins) -> cls (B * N, num_class) logits, reg (B * N, 6 + 2 * bins), box (B * N, 7) decoded at the
    vote xyz (PointBinResidualCoder, use_mean_size False).  No autograd."""
    _need_gpu(feat, stat, vote_xyz)
    lib = _lib.load()
    feat, stat, vote_xyz = _f32(feat), _f32(stat), _f32(vote_xyz)
    b, c, n = feat.shape
    nc = len(cls_mlps)
    if tuple(stat.shape) != (nc, c) or tuple(vote_xyz.shape) != (b * n, 3):
        raise _lib.SpxError("point_head_predict: stat %s / vote_xyz %s do not match features %s and %d classes"
                            % (tuple(stat.shape), tuple(vote_xyz.shape), tuple(feat.shape), nc))
    descs, keep, hc = [], [], None
    for p in cls_mlps:
        d, h, k = _point_mlp(p, c, 1, feat.device)
        if hc is not None and h != hc:
            raise _lib.SpxError("point_head_predict: class blocks of different widths")
        hc = h
        descs.append(d)
        keep += k
    r_out = 6 + 2 * int(bins)
    rdesc, hr, rkeep = _point_mlp(reg_mlp, c, r_out, feat.device)
    cls_arr = (_lib.PointMlp * max(nc, 1))(*descs)
    dev = feat.device
    cls = torch.empty((b * n, nc), dtype=torch.float32, device=dev)
    reg = torch.empty((b * n, r_out), dtype=torch.float32, device=dev)
    box = torch.empty((b * n, 7), dtype=torch.float32, device=dev)
    check(lib.spx_point_head_predict(_ptr(feat), _ptr(stat), _ptr(vote_xyz), b, c, n, nc, cls_arr, hc or 0,
                                     ctypes.byref(rdesc), hr, int(bins), _ptr(cls), _ptr(reg), _ptr(box), _stream(feat)),
          "spx_point_head_predict")
    return cls, reg, box


# --------------------------------------------------------------------------------- point-head post-processing (§15)

POST_PROCESS_MAX_N = 4096   # candidates per frame spx_point_post_process takes


def point_post_process(scores, labels, boxes, batch_size, thresholds, nms_thresh, pre_max, post_max, axis_aligned=False,
                       per_class=True):
    """spx_point_post_process: scores (B * n) normalised, labels (B * n) 1-based, boxes (B * n, >= 7), frames contiguous
    with n rows each; thresholds one float per class (per_class, the fork's multi_thresh) or a single one
    (class-agnostic NMS) -> dict of static-capacity tensors, K rows per frame: sel (B, K) int64 rows of the input or
    -1, count (B) int32, boxes (B, K, 7), scores (B, K), labels (B, K) int64, zeros past count.  No host read."""
    _need_gpu(scores, labels, boxes)
    lib = _lib.load()
    b = int(batch_size)
    thresholds = [float(t) for t in (thresholds if isinstance(thresholds, (list, tuple)) else [thresholds])]
    if scores.dim() != 1 or labels.shape != scores.shape or boxes.dim() != 2 or boxes.shape[0] != scores.shape[0] \
            or boxes.shape[1] < 7 or b < 0 or (b == 0 and scores.shape[0] != 0) or (b > 0 and scores.shape[0] % b != 0):
        raise _lib.SpxError("point_post_process: scores %s, labels %s, boxes %s do not make %d equal frames of (n, 7) boxes"
                            % (tuple(scores.shape), tuple(labels.shape), tuple(boxes.shape), b))
    if not per_class and len(thresholds) != 1:
        raise _lib.SpxError("point_post_process: class-agnostic mode takes one threshold, got %d" % len(thresholds))
    n = scores.shape[0] // b if b > 0 else 0
    dev = scores.device
    scores, labels, boxes = _f32(scores), _i32(labels), _f32(boxes[:, :7])
    nt = len(thresholds)
    k = int(lib.spx_point_post_process_capacity(n, nt, int(post_max), int(bool(per_class)))) if nt > 0 else 0
    out = {"sel": torch.empty((b, k), dtype=torch.int64, device=dev),
           "count": torch.empty((b,), dtype=torch.int32, device=dev),
           "boxes": torch.empty((b, k, 7), dtype=torch.float32, device=dev),
           "scores": torch.empty((b, k), dtype=torch.float32, device=dev),
           "labels": torch.empty((b, k), dtype=torch.int64, device=dev)}
    if b * k == 0 and nt > 0 and int(post_max) >= 1:
        out["count"].zero_()      # frames without candidates: nothing to launch (and no storage to point at)
        return out
    wsb = lib.spx_point_post_process_ws_bytes(b, n, nt, int(post_max))
    ws = workspace(dev, wsb)
    check(lib.spx_point_post_process(_ptr(scores), _ptr(labels), _ptr(boxes), b, n, f_arr(thresholds), nt, float(nms_thresh),
                                     int(pre_max), int(post_max), int(bool(axis_aligned)), int(bool(per_class)),
                                     _ptr(out["sel"]), _ptr(out["count"]), _ptr(out["boxes"]), _ptr(out["scores"]),
                                     _ptr(out["labels"]), _ptr(ws), wsb, _stream(scores)), "spx_point_post_process")
    return out


def recall_count(out_boxes, count, gt_boxes, thresholds):
    """spx_recall_count: out_boxes (B, K, 7) and count (B) int32 of point_post_process, gt_boxes (B, G, >= 7) padded with
    trailing zero rows, thresholds a list of floats -> recalled (B, T) int32, num_gt (B) int32 (the reference's
    generate_recall_record, rcnn_* and gt, per frame).  No host read."""
    _need_gpu(out_boxes, count, gt_boxes)
    lib = _lib.load()
    thresholds = [float(t) for t in thresholds]
    if out_boxes.dim() != 3 or out_boxes.shape[2] != 7 or count.dim() != 1 or count.shape[0] != out_boxes.shape[0] \
            or gt_boxes.dim() != 3 or gt_boxes.shape[0] != out_boxes.shape[0] or gt_boxes.shape[2] < 7 \
            or count.dtype != torch.int32:
        raise _lib.SpxError("recall_count: out_boxes %s, count %s (%s), gt_boxes %s do not match"
                            % (tuple(out_boxes.shape), tuple(count.shape), count.dtype, tuple(gt_boxes.shape)))
    out_boxes, gt_boxes, count = _f32(out_boxes), _f32(gt_boxes), count.contiguous()
    b, k, _ = out_boxes.shape
    nt = len(thresholds)
    dev = out_boxes.device
    recalled = torch.empty((b, nt), dtype=torch.int32, device=dev)
    num_gt = torch.empty((b,), dtype=torch.int32, device=dev)
    check(lib.spx_recall_count(_ptr(out_boxes), _ptr(count), b, k, _ptr(gt_boxes), gt_boxes.shape[1], gt_boxes.shape[2],
                               f_arr(thresholds), nt, _ptr(recalled), _ptr(num_gt), _stream(out_boxes)),
          "spx_recall_count")
    return recalled, num_gt


# ------------------------------------------------------------------------------ point-head target assignment (§16)

TARGET_PLAIN, TARGET_IGNORE_RING, TARGET_BALL = 0, 1, 2
_TARGET_FLOAT_OUTPUTS = ("box_labels", "center_labels", "reg_labels", "centerness")


def point_assign_targets(points, gt_boxes, mode, extra_width=None, central_radius=0.0, num_class=1, angle_bin_num=0,
                         want=_TARGET_FLOAT_OUTPUTS):
    """spx_point_assign_targets: points (B, N, 3), gt_boxes (B, M, >= 8) [x, y, z, dx, dy, dz, rz, class, ...], mode
    TARGET_PLAIN (foreground = inside the box grown by extra_width), TARGET_IGNORE_RING (foreground = inside the gt box,
    -1 in the grown-only ring) or TARGET_BALL (foreground = inside the gt box and within central_radius of its centre,
    -1 for the rest of the box) -> dict of static-shape tensors over the B * N points, frame-major: cls_labels int64,
    box_idx int32 (first box holding the point, -1 none) and those of `want`: box_labels (., 7), center_labels (., 3),
    reg_labels (., 6 + 2 * angle_bin_num; needs angle_bin_num > 0), centerness (.), zero for points whose label is not
    > 0.  num_class 1 labels every foreground point 1; any other value, None included, takes (int64) of the class
    column.  One launch, no host read, no data-dependent shape."""
    _need_gpu(points, gt_boxes)
    lib = _lib.load()
    if points.dim() != 3 or points.shape[2] != 3 or gt_boxes.dim() != 3 or gt_boxes.shape[0] != points.shape[0] \
            or gt_boxes.shape[2] < 8:
        raise _lib.SpxError("point_assign_targets: points %s and gt_boxes %s are not (B, N, 3) and (B, M, >= 8)"
                            % (tuple(points.shape), tuple(gt_boxes.shape)))
    want = tuple(want)
    unknown = [k for k in want if k not in _TARGET_FLOAT_OUTPUTS]
    if unknown or ("reg_labels" in want and int(angle_bin_num) <= 0):
        raise _lib.SpxError("point_assign_targets: want %s (reg_labels needs angle_bin_num > 0, got %d)"
                            % (want, int(angle_bin_num)))
    points, gt_boxes = _f32(points), _f32(gt_boxes)
    b, n, _ = points.shape
    m, ld = gt_boxes.shape[1], gt_boxes.shape[2]
    dev = points.device
    rows = b * n
    widths = {"box_labels": (rows, 7), "center_labels": (rows, 3), "reg_labels": (rows, 6 + 2 * int(angle_bin_num)),
              "centerness": (rows,)}
    out = {"cls_labels": torch.empty((rows,), dtype=torch.int64, device=dev),
           "box_idx": torch.empty((rows,), dtype=torch.int32, device=dev)}
    for k in want:
        out[k] = torch.empty(widths[k], dtype=torch.float32, device=dev)
    num_class = 0 if num_class is None else int(num_class)      # the library tests num_class == 1 only
    ew = f_arr([0.0, 0.0, 0.0] if extra_width is None else [float(v) for v in extra_width])
    if len(ew) != 3:
        raise _lib.SpxError("point_assign_targets: extra_width takes 3 values, got %d" % len(ew))
    if rows == 0:
        return out
    check(lib.spx_point_assign_targets(_ptr(points), _ptr(gt_boxes) if m > 0 else None, b, n, m, ld, ew, int(mode),
                                       float(central_radius), num_class, int(angle_bin_num),
                                       _ptr(out["cls_labels"]), _ptr(out["box_idx"]), _ptr(out.get("box_labels")),
                                       _ptr(out.get("center_labels")), _ptr(out.get("reg_labels")),
                                       _ptr(out.get("centerness")), _stream(points)), "spx_point_assign_targets")
    return out


# --------------------------------------------------------------------------------------- point-head losses (§17)

SEG_BCE, SEG_FOCAL = 0, 1


def _rows_f32(name, t, rows, cols):
    """t as a contiguous fp32 (rows, cols) device tensor, without a copy when it already is one."""
    if t.dim() != 2 or t.shape[0] != rows or (cols is not None and t.shape[1] != cols) or not t.is_floating_point():
        raise _lib.SpxError("%s: shape %s %s, expected float (%d, %s)" % (name, tuple(t.shape), t.dtype, rows, cols))
    return _f32(t)


def _labels_i64(name, t, rows):
    if t.dim() != 1 or t.shape[0] != rows or t.dtype != torch.int64:
        raise _lib.SpxError("%s: shape %s %s, expected int64 (%d,)" % (name, tuple(t.shape), t.dtype, rows))
    return t.detach().contiguous()


def point_head_loss(vote_coords, cls_preds, reg_preds, box_preds, t_cls_preds, t_reg_preds, t_box_preds, vote_cls_labels,
                    vote_reg_labels, cls_labels, reg_labels, box_labels, loss_weights, beta=1.0 / 9.0, centerness_min=0.0,
                    centerness_max=1.0, with_centerness=True, rdiou=True, corner=True):
    """spx_point_head_loss: the student's vote_coords (N, 3), cls_preds (N, C), reg_preds (N, 6 + 2K), box_preds (N, 7),
    the teacher's t_cls_preds, t_reg_preds, t_box_preds, and the targets vote_cls_labels (N) int64, vote_reg_labels
    (N, 3), cls_labels (N) int64, reg_labels (N, 6 + 2K), box_labels (N, 7); loss_weights: the eight LOSS_WEIGHTS in the
    order of include/spx.h §17 -> (losses fp32[3] = (vote, cls, box) weighted and normalised as get_loss does, d_vote,
    d_cls, d_reg, d_box = d(vote + cls + box)/d(the student's four inputs), every element written).  No host read."""
    tensors = (vote_coords, cls_preds, reg_preds, box_preds, t_cls_preds, t_reg_preds, t_box_preds, vote_cls_labels,
               vote_reg_labels, cls_labels, reg_labels, box_labels)
    _need_gpu(*tensors)
    lib = _lib.load()
    if vote_coords.dim() != 2 or cls_preds.dim() != 2 or reg_preds.dim() != 2:
        raise _lib.SpxError("point_head_loss: vote_coords %s, cls_preds %s, reg_preds %s are not (N, 3), (N, C), "
                            "(N, 6 + 2K)" % (tuple(vote_coords.shape), tuple(cls_preds.shape), tuple(reg_preds.shape)))
    n, c, width = vote_coords.shape[0], cls_preds.shape[1], reg_preds.shape[1]
    bins = (width - 6) // 2
    if width != 6 + 2 * bins or bins < 1 or c < 1:
        raise _lib.SpxError("point_head_loss: reg_preds has %d columns, expected 6 + 2 * angle_bin_num; %d classes"
                            % (width, c))
    loss_weights = [float(v) for v in loss_weights]
    if len(loss_weights) != 8:
        raise _lib.SpxError("point_head_loss: loss_weights takes 8 values, got %d" % len(loss_weights))
    vote_coords = _rows_f32("vote_coords", vote_coords, n, 3)
    cls_preds, t_cls_preds = _rows_f32("cls_preds", cls_preds, n, c), _rows_f32("t_cls_preds", t_cls_preds, n, c)
    reg_preds, t_reg_preds = _rows_f32("reg_preds", reg_preds, n, width), _rows_f32("t_reg_preds", t_reg_preds, n, width)
    box_preds, t_box_preds = _rows_f32("box_preds", box_preds, n, 7), _rows_f32("t_box_preds", t_box_preds, n, 7)
    vote_reg_labels = _rows_f32("vote_reg_labels", vote_reg_labels, n, 3)
    reg_labels, box_labels = _rows_f32("reg_labels", reg_labels, n, width), _rows_f32("box_labels", box_labels, n, 7)
    vote_cls_labels = _labels_i64("vote_cls_labels", vote_cls_labels, n)
    cls_labels = _labels_i64("cls_labels", cls_labels, n)
    dev = vote_coords.device
    losses = torch.empty((3,), dtype=torch.float32, device=dev)
    d_vote, d_cls = torch.empty_like(vote_coords), torch.empty_like(cls_preds)
    d_reg, d_box = torch.empty_like(reg_preds), torch.empty_like(box_preds)
    if n == 0:
        losses.zero_()
        return losses, d_vote, d_cls, d_reg, d_box
    params = f_arr(loss_weights + [float(beta), float(centerness_min), float(centerness_max)])
    wsb = lib.spx_point_head_loss_ws_bytes(n)
    ws = workspace(dev, wsb)
    check(lib.spx_point_head_loss(_ptr(vote_coords), _ptr(cls_preds), _ptr(reg_preds), _ptr(box_preds), _ptr(t_cls_preds),
                                  _ptr(t_reg_preds), _ptr(t_box_preds), _ptr(vote_cls_labels), _ptr(vote_reg_labels),
                                  _ptr(cls_labels), _ptr(reg_labels), _ptr(box_labels), n, c, bins, params,
                                  int(bool(with_centerness)), int(bool(rdiou)), int(bool(corner)), _ptr(losses),
                                  _ptr(d_vote), _ptr(d_cls), _ptr(d_reg), _ptr(d_box), _ptr(ws), wsb, _stream(vote_coords)),
          "spx_point_head_loss")
    return losses, d_vote, d_cls, d_reg, d_box


def point_seg_loss(scores, labels, num_class, func, layer_weight):
    """spx_point_seg_loss (one layer of PointSASALoss.loss_forward): scores (N, 1) or (N, num_class) logits, labels (N)
    int64 (> 0 the class, 0 background, -1 ignored), func SEG_BCE or SEG_FOCAL -> (loss fp32[1] = layer_weight * sum /
    max(#labels >= 0, 1), d_scores like scores).  No host read."""
    _need_gpu(scores, labels)
    lib = _lib.load()
    if scores.dim() != 2:
        raise _lib.SpxError("point_seg_loss: scores %s are not (N, 1) or (N, num_class)" % (tuple(scores.shape),))
    n, s = scores.shape
    num_class = int(num_class)
    if s not in (1, num_class) or int(func) not in (SEG_BCE, SEG_FOCAL):
        raise _lib.SpxError("point_seg_loss: %d score columns for %d classes, func %s" % (s, num_class, func))
    scores, labels = _rows_f32("scores", scores, n, s), _labels_i64("labels", labels, n)
    dev = scores.device
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    d_scores = torch.empty_like(scores)
    if n == 0:
        loss.zero_()
        return loss, d_scores
    wsb = lib.spx_point_seg_loss_ws_bytes(n)
    ws = workspace(dev, wsb)
    check(lib.spx_point_seg_loss(_ptr(scores), _ptr(labels), n, s, num_class, int(func), float(layer_weight), _ptr(loss),
                                 _ptr(d_scores), _ptr(ws), wsb, _stream(scores)), "spx_point_seg_loss")
    return loss, d_scores


# ------------------------------------------------------------------------- stacked (ragged-batch) point ops (§18)

def _cnt(name, cnt, dev):
    """A *_batch_cnt as the kernels read it: int32, contiguous, on the device.  Never read here."""
    if cnt.dim() != 1 or cnt.shape[0] < 1:
        raise _lib.SpxError("%s: expected (batch_size,) counts, got %s" % (name, tuple(cnt.shape)))
    if cnt.device != dev:
        raise _lib.SpxError("%s lives on %s, the points on %s" % (name, cnt.device, dev))
    return _i32(cnt)


def stack_ball_query(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, radius, nsample):
    """spx_stack_ball_query: xyz (N, 3), new_xyz (M, 3), counts (B,) int32 on the device -> idx (M, nsample) int32 of
    frame-local rows (unfilled slots = the first hit) and empty (M,) bool.  Rows past the counts' sums are dead: idx 0,
    empty True.  No host read."""
    _need_gpu(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
    lib = _lib.load()
    xyz, new_xyz = _f32(xyz), _f32(new_xyz)
    dev = xyz.device
    nc, mc = _cnt("xyz_batch_cnt", xyz_batch_cnt, dev), _cnt("new_xyz_batch_cnt", new_xyz_batch_cnt, dev)
    n, m = xyz.shape[0], new_xyz.shape[0]
    idx = torch.empty((m, int(nsample)), dtype=torch.int32, device=dev)
    empty = torch.empty((m,), dtype=torch.bool, device=dev)
    if m:
        check(lib.spx_stack_ball_query(_ptr(xyz), _ptr(nc), _ptr(new_xyz), _ptr(mc), nc.shape[0], n, m, float(radius),
                                       int(nsample), _ptr(idx), _ptr(empty), _stream(xyz)), "spx_stack_ball_query")
    return idx, empty


def stack_group_points(features, features_batch_cnt, idx, idx_batch_cnt):
    """spx_stack_group_points: features (N, C), idx (M, S) frame-local -> (M, C, S); dead rows and bad indices read 0."""
    _need_gpu(features, features_batch_cnt, idx, idx_batch_cnt)
    lib = _lib.load()
    features, idx = _f32(features), _i32(idx)
    dev = features.device
    nc, mc = _cnt("features_batch_cnt", features_batch_cnt, dev), _cnt("idx_batch_cnt", idx_batch_cnt, dev)
    (n, c), (m, s) = features.shape, idx.shape
    out = torch.empty((m, c, s), dtype=torch.float32, device=dev)
    if out.numel():
        check(lib.spx_stack_group_points(_ptr(features), _ptr(nc), _ptr(idx), _ptr(mc), nc.shape[0], n, m, c, s, _ptr(out),
                                         _stream(features)), "spx_stack_group_points")
    return out


def stack_group_points_bwd(grad_out, features_batch_cnt, idx, idx_batch_cnt, n):
    """spx_stack_group_points_bwd: grad_out (M, C, S) -> grad_features (n, C), summed in a fixed order."""
    _need_gpu(grad_out, features_batch_cnt, idx, idx_batch_cnt)
    lib = _lib.load()
    grad_out, idx = _f32(grad_out), _i32(idx)
    dev = grad_out.device
    nc, mc = _cnt("features_batch_cnt", features_batch_cnt, dev), _cnt("idx_batch_cnt", idx_batch_cnt, dev)
    m, c, s = grad_out.shape
    grad = torch.empty((int(n), c), dtype=torch.float32, device=dev)
    if grad.numel():
        wsb = lib.spx_stack_group_points_bwd_ws_bytes(int(n), m, c, s)
        ws = workspace(dev, wsb)
        check(lib.spx_stack_group_points_bwd(_ptr(grad_out), _ptr(nc), _ptr(idx), _ptr(mc), nc.shape[0], int(n), m, c, s,
                                             _ptr(grad), _ptr(ws), wsb, _stream(grad_out)), "spx_stack_group_points_bwd")
    return grad


def stack_three_nn(unknown, unknown_batch_cnt, known, known_batch_cnt):
    """spx_stack_three_nn: unknown (N, 3), known (M, 3) -> dist2 (N, 3) squared, idx (N, 3) int32 global known rows."""
    _need_gpu(unknown, unknown_batch_cnt, known, known_batch_cnt)
    lib = _lib.load()
    unknown, known = _f32(unknown), _f32(known)
    dev = unknown.device
    nc, mc = _cnt("unknown_batch_cnt", unknown_batch_cnt, dev), _cnt("known_batch_cnt", known_batch_cnt, dev)
    if nc.shape[0] != mc.shape[0]:
        raise _lib.SpxError("stack_three_nn: %d and %d frames" % (nc.shape[0], mc.shape[0]))
    n, m = unknown.shape[0], known.shape[0]
    dist2 = torch.empty((n, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((n, 3), dtype=torch.int32, device=dev)
    if n:
        check(lib.spx_stack_three_nn(_ptr(unknown), _ptr(nc), _ptr(known), _ptr(mc), nc.shape[0], n, m, _ptr(dist2),
                                     _ptr(idx), _stream(unknown)), "spx_stack_three_nn")
    return dist2, idx


def stack_three_interpolate(features, idx, weight, batch_cnt=None):
    """spx_stack_three_interpolate: features (M, C), idx / weight (N, 3) -> (N, C).  batch_cnt: the counts of the N side;
    rows past their sum are written as 0 (None: every row is live)."""
    _need_gpu(features, idx, weight, batch_cnt)
    lib = _lib.load()
    features, idx, weight = _f32(features), _i32(idx), _f32(weight)
    dev = features.device
    cnt = None if batch_cnt is None else _cnt("batch_cnt", batch_cnt, dev)
    (m, c), n = features.shape, idx.shape[0]
    out = torch.empty((n, c), dtype=torch.float32, device=dev)
    if out.numel():
        check(lib.spx_stack_three_interpolate(_ptr(features), _ptr(idx), _ptr(weight), _ptr(cnt),
                                              0 if cnt is None else cnt.shape[0], m, n, c, _ptr(out), _stream(features)),
              "spx_stack_three_interpolate")
    return out


def stack_three_interpolate_bwd(grad_out, idx, weight, m, batch_cnt=None):
    """spx_stack_three_interpolate_bwd: grad_out (N, C) -> grad_features (m, C), summed in a fixed order."""
    _need_gpu(grad_out, idx, weight, batch_cnt)
    lib = _lib.load()
    grad_out, idx, weight = _f32(grad_out), _i32(idx), _f32(weight)
    dev = grad_out.device
    cnt = None if batch_cnt is None else _cnt("batch_cnt", batch_cnt, dev)
    n, c = grad_out.shape
    grad = torch.empty((int(m), c), dtype=torch.float32, device=dev)
    if grad.numel():
        wsb = lib.spx_stack_three_interpolate_bwd_ws_bytes(int(m), n, c)
        ws = workspace(dev, wsb)
        check(lib.spx_stack_three_interpolate_bwd(_ptr(grad_out), _ptr(idx), _ptr(weight), _ptr(cnt),
                                                  0 if cnt is None else cnt.shape[0], int(m), n, c, _ptr(grad), _ptr(ws),
                                                  wsb, _stream(grad_out)), "spx_stack_three_interpolate_bwd")
    return grad


def stack_furthest_point_sample(xyz, xyz_batch_cnt, npoint, total):
    """spx_stack_furthest_point_sample: xyz (N, 3), counts (B,), npoint (B,) int32 on the device, total = the sum of
    npoint as the caller knows it on the host -> idx (total,) int32 global rows.  No host read."""
    _need_gpu(xyz, xyz_batch_cnt, npoint)
    lib = _lib.load()
    xyz = _f32(xyz)
    dev = xyz.device
    nc, npt = _cnt("xyz_batch_cnt", xyz_batch_cnt, dev), _cnt("npoint", npoint, dev)
    if nc.shape[0] != npt.shape[0]:
        raise _lib.SpxError("stack_furthest_point_sample: %d counts, %d npoint" % (nc.shape[0], npt.shape[0]))
    n = xyz.shape[0]
    idx = torch.empty((int(total),), dtype=torch.int32, device=dev)
    if idx.numel():
        wsb = lib.spx_stack_furthest_point_sample_ws_bytes(n)
        ws = workspace(dev, wsb) if wsb else None
        check(lib.spx_stack_furthest_point_sample(_ptr(xyz), _ptr(nc), _ptr(npt), nc.shape[0], n, int(total), _ptr(idx),
                                                  _ptr(ws), wsb, _stream(xyz)), "spx_stack_furthest_point_sample")
    return idx


# ------------------------------------------------------------------------- voxel rows at static capacity (§19)

VOXEL_ROWS_MAX_M = 4096   # points per frame spx_voxel_rows_mean takes


def _d_n(name, d_n, dev):
    """An optional live row count: int64[1] on `dev`."""
    if d_n is None:
        return None
    if not isinstance(d_n, torch.Tensor) or d_n.dtype != torch.int64 or d_n.numel() != 1 or d_n.device != dev:
        raise _lib.SpxError("%s must be one int64 on %s" % (name, dev))
    return d_n.contiguous()


def voxel_table_build(indices, batch_size, spatial_shape, d_n=None):
    """spx_voxel_table_build: indices (cap, 4) int32 (b, z, y, x), d_n the device live row count (None: every row is
    live) -> table (B, Z, Y, X) int32, the row of the live voxel at each cell, -1 elsewhere.  Rows at or beyond d_n are
    never read; a live row outside the grid is skipped and raises SPX_ERR_OUT_OF_GRID in the sticky status word
    (check_status).  No host read."""
    _need_gpu(indices, d_n)
    lib = _lib.load()
    if indices.dim() != 2 or indices.shape[1] != 4 or indices.dtype != torch.int32:
        raise _lib.SpxError("voxel_table_build: indices must be (cap, 4) int32, got %s %s"
                            % (tuple(indices.shape), indices.dtype))
    indices = indices.contiguous()
    dev = indices.device
    d_n = _d_n("voxel_table_build: d_n", d_n, dev)
    shape = [int(s) for s in spatial_shape]
    table = torch.empty([int(batch_size)] + shape, dtype=torch.int32, device=dev)
    if indices.shape[0] == 0:
        return table.fill_(-1)
    check(lib.spx_voxel_table_build(_ptr(indices), indices.shape[0], _ptr(d_n), int(batch_size), i3(shape), _ptr(table),
                                    _ptr(status_word(dev)), _stream(indices)), "spx_voxel_table_build")
    return table


def voxel_rows_mean(new_xyz, feats, table, range_lo, voxel_size, cap, d_n_rows=None, out=None):
    """spx_voxel_rows_mean: new_xyz (B, m, 3), feats (B, C, m) channels first, table (B, Z, Y, X) of voxel_table_build,
    range_lo / voxel_size 3 host floats (x, y, z) -> out (cap, C): the per-cell mean of the feature columns over each
    frame's points, at the table's row of the cell; the other rows below the live count d_n_rows (None: cap) are 0,
    rows at or beyond it are not written (they keep what a caller's `out` (cap, C) held).  Deterministic, no host read."""
    _need_gpu(new_xyz, feats, table, d_n_rows)
    lib = _lib.load()
    if new_xyz.dim() != 3 or new_xyz.shape[2] != 3 or feats.dim() != 3 or feats.shape[0] != new_xyz.shape[0] \
            or feats.shape[2] != new_xyz.shape[1] or table.dim() != 4 or table.shape[0] != new_xyz.shape[0] \
            or table.dtype != torch.int32:
        raise _lib.SpxError("voxel_rows_mean: new_xyz %s, feats %s, table %s %s do not match (B, m, 3), (B, C, m), "
                            "(B, Z, Y, X) int32" % (tuple(new_xyz.shape), tuple(feats.shape), tuple(table.shape),
                                                    table.dtype))
    new_xyz, feats, table = _f32(new_xyz), _f32(feats), table.contiguous()
    dev = feats.device
    d_n_rows = _d_n("voxel_rows_mean: d_n_rows", d_n_rows, dev)
    b, c, m = feats.shape
    if out is None:
        out = torch.empty((int(cap), c), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (int(cap), c) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise _lib.SpxError("voxel_rows_mean: out must be a contiguous float32 (%d, %d) on %s" % (int(cap), c, dev))
    wsb = lib.spx_voxel_rows_mean_ws_bytes(b, m)
    ws = workspace(dev, wsb)
    check(lib.spx_voxel_rows_mean(_ptr(new_xyz), _ptr(feats), b, c, m, _ptr(table), i3(table.shape[1:]), f_arr(range_lo),
                                  f_arr(voxel_size), _ptr(d_n_rows), int(cap), _ptr(out), _ptr(ws), wsb, _stream(feats)),
          "spx_voxel_rows_mean")
    return out


# --------------------------------------------------------------------------------- centre-head target assignment (§20)

def center_assign_targets(gt_boxes, class_to_head_slot, head_channels, point_cloud_range, voxel_size, feature_map_stride,
                          feature_map_size, num_max_objs=500, gaussian_overlap=0.1, min_radius=2):
    """spx_center_assign_targets: the targets of every head of a centre head for the whole batch, two launches, no host
    read.  gt_boxes (B, M, C >= 8) fp32 device [x, y, z, dx, dy, dz, rz, (extra ...), class], the class in the LAST column,
    1-based over the detector's classes, 0 on padding rows; class_to_head_slot: device int32 (num_class + 1, 2) = (head,
    1-based class within the head) per global class id, -1 where no head owns it; head_channels: the classes of each head
    (host ints); feature_map_size (W, H).  Returns a dict of per-head lists, dtypes and shapes as the reference's
    assign_target_of_single_head stacked over the batch: heatmaps (B, C_h, H, W) fp32, target_boxes (B, num_max_objs, C)
    fp32, inds and masks (B, num_max_objs) int64.  Slot k of a frame and head is the k-th of the frame's boxes owned by
    the head, in input order.  gt_boxes is NOT written: the reference rewrites its class column in place while it filters
    the boxes per head, so with several heads its later heads (and later modules) see corrupted labels; here every head
    sees the original ones.  Deterministic (max of Gaussians, no atomics); the outputs are fully written by the call."""
    _need_gpu(gt_boxes, class_to_head_slot)
    lib = _lib.load()
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] < 8:
        raise _lib.SpxError("center_assign_targets: gt_boxes %s is not (B, M, >= 8)" % (tuple(gt_boxes.shape),))
    heads = [int(c) for c in head_channels]
    if class_to_head_slot.dtype != torch.int32 or class_to_head_slot.dim() != 2 or class_to_head_slot.shape[1] != 2 \
            or class_to_head_slot.shape[0] < 1 or class_to_head_slot.device != gt_boxes.device:
        raise _lib.SpxError("center_assign_targets: class_to_head_slot %s %s is not int32 (num_class + 1, 2) on %s"
                            % (tuple(class_to_head_slot.shape), class_to_head_slot.dtype, gt_boxes.device))
    gt_boxes = _f32(gt_boxes)
    table = class_to_head_slot.contiguous()
    b, m, ld = gt_boxes.shape
    w, h = int(feature_map_size[0]), int(feature_map_size[1])
    k, n_heads, total = int(num_max_objs), len(heads), sum(heads)
    dev = gt_boxes.device
    heat = torch.empty((b * total * h * w,), dtype=torch.float32, device=dev)
    boxes = torch.empty((n_heads, b, k, ld), dtype=torch.float32, device=dev)
    inds = torch.empty((n_heads, b, k), dtype=torch.int64, device=dev)
    masks = torch.empty((n_heads, b, k), dtype=torch.int64, device=dev)
    if b > 0:
        nbytes = lib.spx_center_assign_targets_ws_bytes(b, n_heads, k)
        ws = workspace(dev, nbytes)
        check(lib.spx_center_assign_targets(_ptr(gt_boxes) if m > 0 else None, b, m, ld, _ptr(table), table.shape[0] - 1,
                                            n_heads, (ctypes.c_int32 * n_heads)(*heads),
                                            f_arr([point_cloud_range[0], point_cloud_range[1]]),
                                            f_arr([voxel_size[0], voxel_size[1]]), float(feature_map_stride), w, h, k,
                                            float(gaussian_overlap), int(min_radius), _ptr(heat), _ptr(boxes), _ptr(inds),
                                            _ptr(masks), _ptr(ws), nbytes, _stream(gt_boxes)),
              "spx_center_assign_targets")
    heatmaps, off = [], 0
    for c in heads:
        heatmaps.append(heat[b * h * w * off:b * h * w * (off + c)].view(b, c, h, w))
        off += c
    return {"heatmaps": heatmaps, "target_boxes": list(boxes.unbind(0)), "inds": list(inds.unbind(0)),
            "masks": list(masks.unbind(0))}


# ------------------------------------------------------------------------------------ centre-head box decoding (§21)

CENTER_DECODE_MAX_K = 1024   # rows per frame spx_center_decode selects


def center_decode(hm, center, center_z, dim, rot, vel, K, feature_map_stride, voxel_size, point_cloud_range,
                  post_center_limit_range, score_thresh=None, raw=True):
    """spx_center_decode: the K best cells of one head's heatmap for every frame, decoded to boxes, at static capacity
    and with no host read.  hm (B, C, H, W), center (B, 2, H, W), center_z (B, 1, H, W), dim (B, 3, H, W), rot
    (B, 2, H, W) (cos, sin), vel (B, 2, H, W) or None, fp32 on the GPU; raw: hm holds logits and dim logs (the head's
    outputs), otherwise both are used as given (decode_bbox_from_heatmap's arguments).  Selection is by the value of hm
    as given, descending, equal values lower flat index first.  Returns a dict: boxes (B, K, 7 | 9), scores (B, K),
    labels (B, K) int32 (0-based channel), cells (B, K) int64, keep (B, K) uint8 (inside post_center_limit_range and,
    with score_thresh, score > score_thresh), count (B) int32.  Rows that are not kept hold their decoded values."""
    _need_gpu(hm, center, center_z, dim, rot, vel)
    lib = _lib.load()
    if hm.dim() != 4:
        raise _lib.SpxError("center_decode: hm %s is not (B, C, H, W)" % (tuple(hm.shape),))
    b, c, h, w = hm.shape
    for name, t, ch in (("center", center, 2), ("center_z", center_z, 1), ("dim", dim, 3), ("rot", rot, 2),
                        ("vel", vel, 2)):
        if t is not None and (tuple(t.shape) != (b, ch, h, w) or t.device != hm.device):
            raise _lib.SpxError("center_decode: %s %s on %s is not %s on %s"
                                % (name, tuple(t.shape), t.device, (b, ch, h, w), hm.device))
    k = int(K)
    if not 1 <= k <= h * w:
        raise _lib.SpxError("center_decode: K = %d is outside 1 .. H * W = %d" % (k, h * w))
    hm, center, center_z, dim, rot = _f32(hm), _f32(center), _f32(center_z), _f32(dim), _f32(rot)
    vel = None if vel is None else _f32(vel)
    dev = hm.device
    out = {"boxes": torch.empty((b, k, 7 if vel is None else 9), dtype=torch.float32, device=dev),
           "scores": torch.empty((b, k), dtype=torch.float32, device=dev),
           "labels": torch.empty((b, k), dtype=torch.int32, device=dev),
           "cells": torch.empty((b, k), dtype=torch.int64, device=dev),
           "keep": torch.empty((b, k), dtype=torch.uint8, device=dev),
           "count": torch.empty((b,), dtype=torch.int32, device=dev)}
    if b == 0:
        return out
    wsb = lib.spx_center_decode_ws_bytes(b, c, h, w, k)
    ws = workspace(dev, wsb)
    check(lib.spx_center_decode(_ptr(hm), _ptr(center), _ptr(center_z), _ptr(dim), _ptr(rot), _ptr(vel), b, c, h, w, k,
                                float(feature_map_stride), f_arr([voxel_size[0], voxel_size[1]]),
                                f_arr([point_cloud_range[0], point_cloud_range[1]]),
                                f_arr([float(v) for v in post_center_limit_range]),
                                0.0 if score_thresh is None else float(score_thresh), int(score_thresh is not None),
                                int(bool(raw)), _ptr(out["boxes"]), _ptr(out["scores"]), _ptr(out["labels"]),
                                _ptr(out["cells"]), _ptr(out["keep"]), _ptr(out["count"]), _ptr(ws), wsb, _stream(hm)),
          "spx_center_decode")
    return out


# -------------------------------------------------------------------------------------------- centre-head losses (§22)

def center_head_loss(hm, heatmap, regs, target_boxes, inds, masks, code_weights, cls_weight, loc_weight):
    """spx_center_head_loss: one centre head's focal and L1 losses with their gradients for the whole batch, three
    launches, no host read, no float atomics (bitwise reproducible).  hm (B, C, H, W) heatmap logits and heatmap
    (B, C, H, W) the target of center_assign_targets (1 exactly at the live centres), fp32 on the GPU; regs: the four or
    five regression maps (B, d_i, H, W) in HEAD_ORDER (not concatenated), D = sum d_i <= 10; target_boxes (B, K, D),
    inds and masks (B, K) int64; code_weights: D HOST floats (a sequence or a CPU tensor, so that nothing is read back).
    Returns (losses fp32[2] = (hm_loss * cls_weight, (reg_loss * code_weights).sum() * loc_weight), reg_loss fp32[D]
    unweighted, d_hm like hm, d_regs: one tensor like each of regs), the gradients being those of the two weighted
    losses, every element written by the op (zeros off the live cells).

    Semantics are CenterHead.get_loss's (clamped sigmoid, neg_loss_cornernet with mask=None and its device-side
    num_pos == 0 branch, _reg_loss), except that a slot with masks == 0 is never dereferenced: its inds and target_boxes
    influence nothing.  center_assign_targets zero-fills dead slots, so this differs from the composition only for a NaN
    in a dead slot's target (there NaN * 0 poisons the composition's column), which the target op never produces.  A
    NaN target in a LIVE slot makes its column of reg_loss NaN, as in the composition.  Where sigmoid(hm) lies outside
    [1e-4, 1 - 1e-4] d_hm is exactly 0.  B == 0 launches nothing and returns zeros; with K == 0 the regression part
    launches nothing of its own and its outputs are zeros."""
    regs = list(regs)
    _need_gpu(hm, heatmap, target_boxes, inds, masks, *regs)
    lib = _lib.load()
    if hm.dim() != 4 or not hm.is_floating_point():
        raise _lib.SpxError("center_head_loss: hm %s %s is not float (B, C, H, W)" % (tuple(hm.shape), hm.dtype))
    b, c, h, w = hm.shape
    dev = hm.device
    if tuple(heatmap.shape) != (b, c, h, w) or not heatmap.is_floating_point() or heatmap.device != dev:
        raise _lib.SpxError("center_head_loss: heatmap %s %s on %s is not float %s on %s"
                            % (tuple(heatmap.shape), heatmap.dtype, heatmap.device, (b, c, h, w), dev))
    if not 1 <= len(regs) <= 5:
        raise _lib.SpxError("center_head_loss: %d regression maps, expected 1 .. 5" % len(regs))
    for i, t in enumerate(regs):
        if t.dim() != 4 or t.shape[0] != b or t.shape[1] < 1 or tuple(t.shape[2:]) != (h, w) \
                or not t.is_floating_point() or t.device != dev:
            raise _lib.SpxError("center_head_loss: regs[%d] %s %s on %s is not float (%d, d, %d, %d) on %s"
                                % (i, tuple(t.shape), t.dtype, t.device, b, h, w, dev))
    chans = [int(t.shape[1]) for t in regs]
    d = sum(chans)
    if target_boxes.dim() != 3 or target_boxes.shape[0] != b or target_boxes.shape[2] != d \
            or not target_boxes.is_floating_point() or target_boxes.device != dev:
        raise _lib.SpxError("center_head_loss: target_boxes %s %s is not float (%d, K, %d): the regression maps have %s "
                            "channels" % (tuple(target_boxes.shape), target_boxes.dtype, b, d, chans))
    k = target_boxes.shape[1]
    for name, t in (("inds", inds), ("masks", masks)):
        if tuple(t.shape) != (b, k) or t.dtype != torch.int64 or t.device != dev:
            raise _lib.SpxError("center_head_loss: %s %s %s on %s is not int64 (%d, %d) on %s"
                                % (name, tuple(t.shape), t.dtype, t.device, b, k, dev))
    if isinstance(code_weights, torch.Tensor):
        if code_weights.is_cuda:
            raise _lib.SpxError("center_head_loss: code_weights is a GPU tensor; pass host floats (reading it back would "
                                "be a host sync)")
        code_weights = code_weights.tolist()
    code_weights = [float(v) for v in code_weights]
    if len(code_weights) != d:
        raise _lib.SpxError("center_head_loss: %d code_weights for %d regression columns" % (len(code_weights), d))
    hm, heatmap, target_boxes = _f32(hm), _f32(heatmap), _f32(target_boxes)
    regs = [_f32(t) for t in regs]
    inds, masks = inds.detach().contiguous(), masks.detach().contiguous()
    losses = torch.empty((2,), dtype=torch.float32, device=dev)
    reg_loss = torch.empty((d,), dtype=torch.float32, device=dev)
    d_hm = torch.empty_like(hm)
    d_regs = [torch.empty_like(t) for t in regs]
    if b == 0:
        losses.zero_()
        reg_loss.zero_()
        return losses, reg_loss, d_hm, d_regs
    n = len(regs)
    wsb = lib.spx_center_head_loss_ws_bytes(b, c, h, w, k)
    ws = workspace(dev, wsb)
    check(lib.spx_center_head_loss(_ptr(hm), _ptr(heatmap), (ctypes.c_void_p * n)(*[t.data_ptr() for t in regs]),
                                   (ctypes.c_int32 * n)(*chans), n, _ptr(target_boxes) if k > 0 else None,
                                   _ptr(inds) if k > 0 else None, _ptr(masks) if k > 0 else None, b, c, h, w, k,
                                   f_arr(code_weights), float(cls_weight), float(loc_weight), _ptr(losses),
                                   _ptr(reg_loss), _ptr(d_hm), (ctypes.c_void_p * n)(*[t.data_ptr() for t in d_regs]),
                                   _ptr(ws), wsb, _stream(hm)), "spx_center_head_loss")
    return losses, reg_loss, d_hm, d_regs


# --------------------------------------------------------------------------------- PillarVFE, one last-layer PFN (§23)

PILLAR_VFE_MAX_T = 32     # points per pillar spx_pillar_vfe_* takes
PILLAR_VFE_C_OUT = 64     # the one output width it is instantiated for


def pillar_vfe_c_in(c, use_absolute_xyz, with_distance):
    """Width of PillarVFE's per-point feature vector for c raw columns."""
    return (c + 6 if use_absolute_xyz else c + 3) + (1 if with_distance else 0)


def _pfn_geom(voxel_size, offsets):
    return f_arr([float(v) for v in voxel_size] + [float(v) for v in offsets])


def _pfn_weight(what, weight, c, use_absolute_xyz, with_distance, dev):
    """The weight checks of both PFN ops (§23, §24) -> C_in."""
    c_in = pillar_vfe_c_in(c, use_absolute_xyz, with_distance)
    if weight.dim() != 2 or weight.shape[1] != c_in or weight.dtype != torch.float32 or weight.device != dev:
        raise _lib.SpxError("%s: weight %s %s is not float32 (C_out, %d) on %s: C = %d, use_absolute_xyz = %s, "
                            "with_distance = %s" % (what, tuple(weight.shape), weight.dtype, c_in, dev, c,
                                                    bool(use_absolute_xyz), bool(with_distance)))
    if weight.shape[0] != PILLAR_VFE_C_OUT:
        raise _lib.SpxError("%s: C_out = %d is not supported, the kernels are built for C_out = %d"
                            % (what, weight.shape[0], PILLAR_VFE_C_OUT))
    return c_in


def _pillar_inputs(what, voxels, num_points, coords, weight, use_absolute_xyz, with_distance, d_n):
    """Shape, dtype and device checks shared by the two entry points -> contiguous inputs."""
    if voxels.dim() != 3 or voxels.dtype != torch.float32:
        raise _lib.SpxError("%s: voxels %s %s is not float32 (M, T, C)" % (what, tuple(voxels.shape), voxels.dtype))
    m, t, c = voxels.shape
    dev = voxels.device
    if not 1 <= t <= PILLAR_VFE_MAX_T or not 3 <= c <= 6:
        raise _lib.SpxError("%s: T = %d, C = %d outside 1 <= T <= %d, 3 <= C <= 6" % (what, t, c, PILLAR_VFE_MAX_T))
    if tuple(num_points.shape) != (m,) or num_points.device != dev or num_points.dtype not in (torch.int32, torch.int64):
        raise _lib.SpxError("%s: num_points %s %s on %s is not an integer (%d,) on %s"
                            % (what, tuple(num_points.shape), num_points.dtype, num_points.device, m, dev))
    if tuple(coords.shape) != (m, 4) or coords.device != dev or coords.dtype not in (torch.int32, torch.int64):
        raise _lib.SpxError("%s: coords %s %s on %s is not an integer (%d, 4) on %s"
                            % (what, tuple(coords.shape), coords.dtype, coords.device, m, dev))
    c_in = _pfn_weight(what, weight, c, use_absolute_xyz, with_distance, dev)
    if d_n is not None and isinstance(d_n, torch.Tensor) and d_n.dtype == torch.int32 and d_n.numel() == 1:
        d_n = d_n.to(torch.int64).view(1)              # a device cast, no host read
    d_n = _d_n("%s: d_n" % what, d_n, dev)
    return (voxels.contiguous(), num_points.to(torch.int32).contiguous(), coords.to(torch.int32).contiguous(),
            weight.detach().contiguous(), d_n, m, t, c, c_in)


def _vec64(what, name, v, dev, dtype=torch.float32, n=PILLAR_VFE_C_OUT):
    if v is None:
        return None
    if tuple(v.shape) != (n,) or v.dtype != dtype or v.device != dev or not v.is_contiguous():
        raise _lib.SpxError("%s: %s %s %s on %s is not a contiguous %s (%d,) on %s"
                            % (what, name, tuple(v.shape), v.dtype, v.device, dtype, n, dev))
    return v


def _pfn_bn(what, gamma, beta, running_mean, running_var, num_batches_tracked, training, dev):
    """The forward's BatchNorm tensors, checked -> (gamma, beta, running_mean, running_var, nbt)."""
    gamma = _vec64(what, "gamma", gamma.detach(), dev)
    beta = _vec64(what, "beta", beta.detach(), dev)
    running_mean = _vec64(what, "running_mean", running_mean, dev)
    running_var = _vec64(what, "running_var", running_var, dev)
    nbt = None
    if num_batches_tracked is not None:
        nbt = _vec64(what, "num_batches_tracked", num_batches_tracked.view(-1), dev, torch.int64, 1)
    if not training and (running_mean is None or running_var is None):
        raise _lib.SpxError("%s: eval mode needs running_mean and running_var" % what)
    return gamma, beta, running_mean, running_var, nbt


def _pfn_train_buffers(training, stats_len, dev):
    """(mean, invstd (64,) float32, stats float64[stats_len()]) in training, else three None."""
    if not training:
        return None, None, None
    return (torch.empty((PILLAR_VFE_C_OUT,), dtype=torch.float32, device=dev),
            torch.empty((PILLAR_VFE_C_OUT,), dtype=torch.float32, device=dev),
            torch.empty((int(stats_len()),), dtype=torch.float64, device=dev))


def _pfn_bwd_state(what, weight, gamma, stats, stats_len, running_mean, running_var, training, dev):
    """The backward's gamma and stats (training) or running statistics (eval), checked, and the three gradients ->
    (gamma, stats, running_mean, running_var, d_weight, d_gamma, d_beta)."""
    gamma = _vec64(what, "gamma", gamma.detach(), dev)
    if training:
        stats = _vec64(what, "stats", stats, dev, torch.float64, int(stats_len()))
        if stats is None:
            raise _lib.SpxError("%s: training mode needs the forward's stats" % what)
    else:
        running_mean = _vec64(what, "running_mean", running_mean, dev)
        running_var = _vec64(what, "running_var", running_var, dev)
        if running_mean is None or running_var is None:
            raise _lib.SpxError("%s: eval mode needs running_mean and running_var" % what)
    d_weight = torch.empty_like(weight)
    d_gamma = torch.empty((PILLAR_VFE_C_OUT,), dtype=torch.float32, device=dev)
    d_beta = torch.empty((PILLAR_VFE_C_OUT,), dtype=torch.float32, device=dev)
    return gamma, stats, running_mean, running_var, d_weight, d_gamma, d_beta


def pillar_vfe_fwd(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, num_batches_tracked,
                   momentum, eps, voxel_size, offsets, use_absolute_xyz=True, with_distance=False, training=False,
                   d_n=None):
    """spx_pillar_vfe_fwd (include/spx.h §23): PillarVFE with one last-layer PFNLayer, Linear + BatchNorm1d + ReLU + max
    over the points of every pillar without the (M, T, C_out) tensor.  voxels (M, T, C) float32, num_points (M,),
    coords (M, 4) (b, z, y, x), weight (64, C_in); voxel_size / offsets: 3 host floats each (x, y, z), offsets = voxel / 2
    + range_lo; d_n: device int64[1] live row count (static capacity), rows at or beyond it are never read and come back
    as zeros.  training: batch statistics, and running_mean / running_var / num_batches_tracked are updated IN PLACE.
    Returns dict(out (M, 64), arg (M, 64) uint8: the winning point of each (pillar, channel), T = a padding row;
    mean, invstd (64,) and stats (double, for pillar_vfe_bwd) in training, else None).  No host read."""
    what = "pillar_vfe_fwd"
    _need_gpu(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, num_batches_tracked, d_n)
    lib = _lib.load()
    voxels, num, coords, weight, d_n, m, t, c, c_in = _pillar_inputs(what, voxels, num_points, coords, weight,
                                                                      use_absolute_xyz, with_distance, d_n)
    dev = voxels.device
    gamma, beta, running_mean, running_var, nbt = _pfn_bn(what, gamma, beta, running_mean, running_var,
                                                          num_batches_tracked, training, dev)
    out = torch.empty((m, PILLAR_VFE_C_OUT), dtype=torch.float32, device=dev)
    arg = torch.empty((m, PILLAR_VFE_C_OUT), dtype=torch.uint8, device=dev)
    mean, invstd, stats = _pfn_train_buffers(training, lib.spx_pillar_vfe_stats_len, dev)
    res = dict(out=out, arg=arg, mean=mean, invstd=invstd, stats=stats)
    if m == 0:
        if training:
            raise _lib.SpxError("%s: training-mode batch statistics of 0 pillars" % what)
        return res
    wsb = lib.spx_pillar_vfe_ws_bytes(m)
    ws = workspace(dev, wsb)
    check(lib.spx_pillar_vfe_fwd(_ptr(voxels), _ptr(num), _ptr(coords), m, _ptr(d_n), t, c, _ptr(weight), c_in,
                                 weight.shape[0], _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(nbt),
                                 float(momentum), float(eps), _pfn_geom(voxel_size, offsets),
                                 1 if use_absolute_xyz else 0, 1 if with_distance else 0, 1 if training else 0, _ptr(out),
                                 _ptr(arg), _ptr(mean), _ptr(invstd), _ptr(stats), _ptr(ws), wsb, _stream(voxels)),
          "spx_pillar_vfe_fwd")
    return res


def pillar_vfe_bwd(d_out, out, arg, stats, voxels, num_points, coords, weight, gamma, running_mean, running_var, eps,
                   voxel_size, offsets, use_absolute_xyz=True, with_distance=False, training=True, d_n=None):
    """spx_pillar_vfe_bwd: (d_weight (64, C_in), d_gamma (64,), d_beta (64,)) from d_out (M, 64) and what pillar_vfe_fwd
    returned (out, arg, and stats in training): the exact train-mode BatchNorm gradient (eval: on the running statistics)
    from the selected rows alone.  Deterministic, no host read."""
    what = "pillar_vfe_bwd"
    _need_gpu(d_out, out, arg, stats, voxels, num_points, coords, weight, gamma, running_mean, running_var, d_n)
    lib = _lib.load()
    voxels, num, coords, weight, d_n, m, t, c, c_in = _pillar_inputs(what, voxels, num_points, coords, weight,
                                                                      use_absolute_xyz, with_distance, d_n)
    dev = voxels.device
    shape = (m, PILLAR_VFE_C_OUT)
    if tuple(d_out.shape) != shape or d_out.device != dev or tuple(out.shape) != shape or out.dtype != torch.float32 \
            or tuple(arg.shape) != shape or arg.dtype != torch.uint8:
        raise _lib.SpxError("%s: d_out %s, out %s %s, arg %s %s do not match float32 / float32 / uint8 %s"
                            % (what, tuple(d_out.shape), tuple(out.shape), out.dtype, tuple(arg.shape), arg.dtype, shape))
    d_out, out, arg = _f32(d_out), out.contiguous(), arg.contiguous()
    gamma, stats, running_mean, running_var, d_weight, d_gamma, d_beta = _pfn_bwd_state(
        what, weight, gamma, stats, lib.spx_pillar_vfe_stats_len, running_mean, running_var, training, dev)
    if m == 0:
        return d_weight.zero_(), d_gamma.zero_(), d_beta.zero_()
    wsb = lib.spx_pillar_vfe_ws_bytes(m)
    ws = workspace(dev, wsb)
    check(lib.spx_pillar_vfe_bwd(_ptr(voxels), _ptr(num), _ptr(coords), m, _ptr(d_n), t, c, _ptr(weight), c_in,
                                 weight.shape[0], _ptr(gamma), _ptr(running_mean), _ptr(running_var), float(eps),
                                 _pfn_geom(voxel_size, offsets), 1 if use_absolute_xyz else 0,
                                 1 if with_distance else 0, 1 if training else 0, _ptr(out), _ptr(arg), _ptr(d_out),
                                 _ptr(stats) if training else None, _ptr(d_weight), _ptr(d_gamma), _ptr(d_beta), _ptr(ws),
                                 wsb, _stream(voxels)), "spx_pillar_vfe_bwd")
    return d_weight, d_gamma, d_beta


class _PillarVFEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, gamma, beta, voxels, num_points, coords, running_mean, running_var, nbt, cfg):
        res = pillar_vfe_fwd(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, nbt,
                             cfg["momentum"], cfg["eps"], cfg["voxel_size"], cfg["offsets"], cfg["use_absolute_xyz"],
                             cfg["with_distance"], cfg["training"], cfg["d_n"])
        ctx.cfg = cfg
        ctx.inputs = (voxels, num_points, coords, running_mean, running_var)
        ctx.save_for_backward(weight, gamma, res["out"], res["arg"], *([res["stats"]] if cfg["training"] else []))
        ctx.mark_non_differentiable(res["arg"])
        mean, invstd = res["mean"], res["invstd"]
        if mean is None:
            mean = invstd = weight.new_empty((0,))
        ctx.mark_non_differentiable(mean, invstd)
        return res["out"], res["arg"], mean, invstd

    @staticmethod
    def backward(ctx, d_out, _d_arg, _d_mean, _d_invstd):
        cfg = ctx.cfg
        weight, gamma, out, arg = ctx.saved_tensors[:4]
        stats = ctx.saved_tensors[4] if cfg["training"] else None
        voxels, num_points, coords, running_mean, running_var = ctx.inputs
        dw, dg, db = pillar_vfe_bwd(d_out, out, arg, stats, voxels, num_points, coords, weight, gamma, running_mean,
                                    running_var, cfg["eps"], cfg["voxel_size"], cfg["offsets"], cfg["use_absolute_xyz"],
                                    cfg["with_distance"], cfg["training"], cfg["d_n"])
        return dw, dg, db, None, None, None, None, None, None, None


def pillar_vfe(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, num_batches_tracked, momentum,
               eps, voxel_size, offsets, use_absolute_xyz=True, with_distance=False, training=False, d_n=None):
    """The differentiable form of pillar_vfe_fwd / pillar_vfe_bwd: (pillar_features (M, 64), arg (M, 64) uint8, mean,
    invstd) with gradients for weight, gamma and beta.  In eval mode the running statistics are read a second time by the
    backward, so they must not change in between.  There is no gradient with respect to voxels."""
    if voxels.requires_grad:
        raise _lib.SpxError("pillar_vfe: voxels.requires_grad is set, but the op has no gradient with respect to voxels")
    cfg = dict(momentum=float(momentum), eps=float(eps), voxel_size=[float(v) for v in voxel_size],
               offsets=[float(v) for v in offsets], use_absolute_xyz=bool(use_absolute_xyz),
               with_distance=bool(with_distance), training=bool(training), d_n=d_n)
    return _PillarVFEFn.apply(weight, gamma, beta, voxels, num_points, coords, running_mean, running_var,
                              num_batches_tracked, cfg)


# ------------------------------------------------------- DynamicPillarVFE: pillarisation + one last-layer PFN (§24)

def _grid2(point_cloud_range, voxel_size):
    rng = [float(x) for x in point_cloud_range]
    vs = [float(x) for x in voxel_size]
    return rng, vs, [int(round((rng[3 + j] - rng[j]) / vs[j])) for j in range(2)]


def dynamic_pillarize(points, point_cloud_range, voxel_size, batch_size=1, batch_col=0, xyz_col=1, max_pillars=None,
                      sync=True):
    """spx_dynamic_pillarize (include/spx.h §24; reference DynamicPillarVFE.forward's torch.unique): every point with
    0 <= cx < X and 0 <= cy < Y is kept, z is not tested; NaN x / y and a batch column outside [0, batch_size) drop the
    point.  Pillars are the unique cells in ascending key (b X + cx) Y + cy.  Returns dict(coords [M, 4] (b, 0, cy, cx),
    inverse [N] (pillar row of each point, -1 = dropped), count [M], offset [M + 1], order [N] (point rows grouped by
    pillar, ascending inside a pillar), d_num_pillars, d_num_points (device int64[1]), num_pillars, num_points, grid_size).
    sync=True reads the two counts (one host read) and trims the rows to M; sync=False reads nothing: rows stay at the
    capacity min(N, max_pillars), num_pillars / num_points are None, and a pillar count above the capacity raises
    SPX_ERR_CAPACITY in the device status word (check_status)."""
    _need_gpu(points)
    if points.dim() != 2 or points.dtype != torch.float32:
        raise _lib.SpxError("dynamic_pillarize: points %s %s is not float32 (N, stride)" % (tuple(points.shape), points.dtype))
    lib = _lib.load()
    points = points.contiguous()
    n, stride = points.shape
    rng, vs, grid = _grid2(point_cloud_range, voxel_size)
    if min(grid) <= 0 or batch_size <= 0 or xyz_col < 0 or xyz_col + 2 > stride or batch_col >= stride:
        raise _lib.SpxError("dynamic_pillarize: grid %s, batch_size %d, xyz_col %d, batch_col %d do not fit points of stride "
                            "%d" % (grid, batch_size, xyz_col, batch_col, stride))
    cap = max(1, n if max_pillars is None else min(n, int(max_pillars)))
    dev = points.device
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    inv = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    count = torch.empty((cap,), dtype=torch.int32, device=dev)
    offset = torch.empty((cap + 1,), dtype=torch.int32, device=dev)
    order = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    d_num = torch.zeros((2,), dtype=torch.int64, device=dev)
    g2 = (ctypes.c_int32 * 2)(*grid)
    wsb = lib.spx_dynamic_pillarize_ws_bytes(n, batch_size, g2, cap)
    ws = workspace(dev, wsb)
    status = None if sync else status_word(dev)
    check(lib.spx_dynamic_pillarize(_ptr(points), n, stride, batch_col, xyz_col, f_arr(rng[:2]), f_arr(vs[:2]), g2,
                                    batch_size, _ptr(coords), _ptr(inv), _ptr(count), _ptr(offset), _ptr(order),
                                    _ptr(d_num[0:1]), _ptr(d_num[1:2]), cap, _ptr(status), _ptr(ws), wsb, _stream(points)),
          "spx_dynamic_pillarize")
    out = {"d_num_pillars": d_num[0:1], "d_num_points": d_num[1:2], "grid_size": grid, "inverse": inv[:n], "order": order[:n]}
    if sync:
        m, kept = d_num.tolist()
        m = min(int(m), cap)
        out.update(coords=coords[:m], count=count[:m], offset=offset[:m + 1], num_pillars=m, num_points=int(kept))
    else:
        out.update(coords=coords, count=count, offset=offset, num_pillars=None, num_points=None)
    return out


def _dyn_pillar_inputs(what, points, pillars, weight, use_absolute_xyz, with_distance, xyz_col, num_features):
    """Shape, dtype and device checks shared by the two entry points."""
    if points.dim() != 2 or points.dtype != torch.float32:
        raise _lib.SpxError("%s: points %s %s is not float32 (N, stride)" % (what, tuple(points.shape), points.dtype))
    n, stride = points.shape
    dev = points.device
    c = (stride - xyz_col) if num_features is None else int(num_features)
    if not 3 <= c <= 6 or xyz_col < 0 or xyz_col + c > stride:
        raise _lib.SpxError("%s: %d raw columns from column %d of %d: outside 3 <= C <= 6" % (what, c, xyz_col, stride))
    coords = pillars["coords"]
    cap = coords.shape[0]
    for name, shape in (("coords", (cap, 4)), ("offset", (cap + 1,)), ("inverse", (n,)), ("order", (n,))):
        t = pillars[name]
        if tuple(t.shape) != shape or t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            raise _lib.SpxError("%s: pillars[%r] %s %s on %s is not a contiguous int32 %s on %s"
                                % (what, name, tuple(t.shape), t.dtype, t.device, shape, dev))
    if cap < 1:
        raise _lib.SpxError("%s: no pillar rows (a cloud with no kept point has no batch statistics and no output)" % what)
    d_np = _d_n("%s: d_num_pillars" % what, pillars["d_num_pillars"], dev)
    d_npts = _d_n("%s: d_num_points" % what, pillars["d_num_points"], dev)
    c_in = _pfn_weight(what, weight, c, use_absolute_xyz, with_distance, dev)
    return points.contiguous(), weight.detach().contiguous(), d_np, d_npts, n, stride, c, c_in, cap


def dynamic_pillar_vfe_fwd(points, pillars, weight, gamma, beta, running_mean, running_var, num_batches_tracked, momentum,
                           eps, voxel_size, offsets, use_absolute_xyz=True, with_distance=False, training=False, xyz_col=1,
                           num_features=None):
    """spx_dynamic_pillar_vfe_fwd (include/spx.h §24): DynamicPillarVFE with one last-layer PFNLayerV2 over the ragged
    pillars of dynamic_pillarize (`pillars`: its dict, synced or at capacity), without the (N, 64) activations.  points
    (N, stride) float32 with the raw columns (x, y, z first) from xyz_col; offsets = voxel / 2 + range_lo (x, y, z).
    training: batch statistics over the kept points, and running_mean / running_var / num_batches_tracked are updated IN
    PLACE; fewer than two kept points leave them untouched and raise SPX_ERR_BATCH_STATS in the device status word.
    Returns dict(out (M, 64), arg (M, 64) int32: the winning point row of each (pillar, channel), pillar_mean (M, 3)
    float64; mean, invstd (64,) and stats (double, for dynamic_pillar_vfe_bwd) in training, else None).  No host read."""
    what = "dynamic_pillar_vfe_fwd"
    _need_gpu(points, weight, gamma, beta, running_mean, running_var, num_batches_tracked, pillars["coords"])
    lib = _lib.load()
    points, weight, d_np, d_npts, n, stride, c, c_in, cap = _dyn_pillar_inputs(
        what, points, pillars, weight, use_absolute_xyz, with_distance, xyz_col, num_features)
    dev = points.device
    gamma, beta, running_mean, running_var, nbt = _pfn_bn(what, gamma, beta, running_mean, running_var,
                                                          num_batches_tracked, training, dev)
    out = torch.empty((cap, PILLAR_VFE_C_OUT), dtype=torch.float32, device=dev)
    arg = torch.empty((cap, PILLAR_VFE_C_OUT), dtype=torch.int32, device=dev)
    pmean = torch.empty((cap, 3), dtype=torch.float64, device=dev)
    mean, invstd, stats = _pfn_train_buffers(training, lib.spx_dynamic_pillar_vfe_stats_len, dev)
    wsb = lib.spx_dynamic_pillar_vfe_ws_bytes(n)
    ws = workspace(dev, wsb)
    check(lib.spx_dynamic_pillar_vfe_fwd(
        _ptr(points), n, stride, xyz_col, c, _ptr(pillars["coords"]), _ptr(pillars["inverse"]), _ptr(pillars["offset"]),
        _ptr(pillars["order"]), cap, _ptr(d_np), _ptr(d_npts), _ptr(weight), c_in, weight.shape[0], _ptr(gamma), _ptr(beta),
        _ptr(running_mean), _ptr(running_var), _ptr(nbt), float(momentum), float(eps), _pfn_geom(voxel_size[:2], offsets),
        1 if use_absolute_xyz else 0, 1 if with_distance else 0, 1 if training else 0, _ptr(out), _ptr(arg), _ptr(pmean),
        _ptr(mean), _ptr(invstd), _ptr(stats), _ptr(status_word(dev)), _ptr(ws), wsb, _stream(points)),
        "spx_dynamic_pillar_vfe_fwd")
    return dict(out=out, arg=arg, pillar_mean=pmean, mean=mean, invstd=invstd, stats=stats)


def dynamic_pillar_vfe_bwd(d_out, out, arg, pillar_mean, stats, points, pillars, weight, gamma, running_mean, running_var,
                           eps, voxel_size, offsets, use_absolute_xyz=True, with_distance=False, training=True, xyz_col=1,
                           num_features=None):
    """spx_dynamic_pillar_vfe_bwd: (d_weight (64, C_in), d_gamma (64,), d_beta (64,)) from d_out (M, 64) and what
    dynamic_pillar_vfe_fwd returned (out, arg, pillar_mean, and stats in training): the exact train-mode BatchNorm
    gradient (eval: on the running statistics) from the selected points alone.  Deterministic, no host read."""
    what = "dynamic_pillar_vfe_bwd"
    _need_gpu(d_out, out, arg, pillar_mean, stats, points, weight, gamma, running_mean, running_var)
    lib = _lib.load()
    points, weight, d_np, _d_npts, n, stride, c, c_in, cap = _dyn_pillar_inputs(
        what, points, pillars, weight, use_absolute_xyz, with_distance, xyz_col, num_features)
    dev = points.device
    shape = (cap, PILLAR_VFE_C_OUT)
    if tuple(d_out.shape) != shape or d_out.device != dev or tuple(out.shape) != shape or out.dtype != torch.float32 \
            or tuple(arg.shape) != shape or arg.dtype != torch.int32 or tuple(pillar_mean.shape) != (cap, 3) \
            or pillar_mean.dtype != torch.float64:
        raise _lib.SpxError("%s: d_out %s, out %s %s, arg %s %s, pillar_mean %s %s do not match float32 / float32 / int32 %s "
                            "and float64 (%d, 3)" % (what, tuple(d_out.shape), tuple(out.shape), out.dtype, tuple(arg.shape),
                                                     arg.dtype, tuple(pillar_mean.shape), pillar_mean.dtype, shape, cap))
    d_out, out, arg, pillar_mean = _f32(d_out), out.contiguous(), arg.contiguous(), pillar_mean.contiguous()
    gamma, stats, running_mean, running_var, d_weight, d_gamma, d_beta = _pfn_bwd_state(
        what, weight, gamma, stats, lib.spx_dynamic_pillar_vfe_stats_len, running_mean, running_var, training, dev)
    wsb = lib.spx_dynamic_pillar_vfe_ws_bytes(n)
    ws = workspace(dev, wsb)
    check(lib.spx_dynamic_pillar_vfe_bwd(
        _ptr(points), n, stride, xyz_col, c, _ptr(pillars["coords"]), cap, _ptr(d_np), _ptr(weight), c_in, weight.shape[0],
        _ptr(gamma), _ptr(running_mean), _ptr(running_var), float(eps), _pfn_geom(voxel_size[:2], offsets),
        1 if use_absolute_xyz else 0, 1 if with_distance else 0, 1 if training else 0, _ptr(out), _ptr(arg), _ptr(d_out),
        _ptr(pillar_mean), _ptr(stats) if training else None, _ptr(d_weight), _ptr(d_gamma), _ptr(d_beta), _ptr(ws), wsb,
        _stream(points)), "spx_dynamic_pillar_vfe_bwd")
    return d_weight, d_gamma, d_beta


class _DynPillarVFEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, gamma, beta, points, running_mean, running_var, nbt, pillars, cfg):
        res = dynamic_pillar_vfe_fwd(points, pillars, weight, gamma, beta, running_mean, running_var, nbt, cfg["momentum"],
                                     cfg["eps"], cfg["voxel_size"], cfg["offsets"], cfg["use_absolute_xyz"],
                                     cfg["with_distance"], cfg["training"], cfg["xyz_col"], cfg["num_features"])
        ctx.cfg = cfg
        ctx.inputs = (points, pillars, running_mean, running_var)
        ctx.save_for_backward(weight, gamma, res["out"], res["arg"], res["pillar_mean"],
                              *([res["stats"]] if cfg["training"] else []))
        ctx.mark_non_differentiable(res["arg"])
        return res["out"], res["arg"]

    @staticmethod
    def backward(ctx, d_out, _d_arg):
        cfg = ctx.cfg
        weight, gamma, out, arg, pmean = ctx.saved_tensors[:5]
        stats = ctx.saved_tensors[5] if cfg["training"] else None
        points, pillars, running_mean, running_var = ctx.inputs
        dw, dg, db = dynamic_pillar_vfe_bwd(d_out, out, arg, pmean, stats, points, pillars, weight, gamma, running_mean,
                                            running_var, cfg["eps"], cfg["voxel_size"], cfg["offsets"],
                                            cfg["use_absolute_xyz"], cfg["with_distance"], cfg["training"], cfg["xyz_col"],
                                            cfg["num_features"])
        return dw, dg, db, None, None, None, None, None, None


def dynamic_pillar_vfe(points, pillars, weight, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                       voxel_size, offsets, use_absolute_xyz=True, with_distance=False, training=False, xyz_col=1,
                       num_features=None):
    """The differentiable form of dynamic_pillar_vfe_fwd / _bwd: (pillar_features (M, 64), arg (M, 64) int32) with
    gradients for weight, gamma and beta.  In eval mode the running statistics are read a second time by the backward, so
    they must not change in between.  Points are data: there is no gradient with respect to them."""
    if points.requires_grad:
        raise _lib.SpxError("dynamic_pillar_vfe: points.requires_grad is set, but the op has no gradient with respect to "
                            "points")
    cfg = dict(momentum=float(momentum), eps=float(eps), voxel_size=[float(v) for v in voxel_size],
               offsets=[float(v) for v in offsets], use_absolute_xyz=bool(use_absolute_xyz),
               with_distance=bool(with_distance), training=bool(training), xyz_col=int(xyz_col),
               num_features=None if num_features is None else int(num_features))
    return _DynPillarVFEFn.apply(weight, gamma, beta, points, running_mean, running_var, num_batches_tracked, pillars, cfg)


# ------------------------------------------------------------------------------ second stage: RoI pooling, sampling (§25, §26)

ROI_GRID_POOL_MAX_G = 12
PROPOSAL_SAMPLE_MAX_R = 2048


def roi_grid_pool_bev(rois, features, grid_size, min_x, min_y, step_x, step_y, d_n=None):
    """spx_roi_grid_pool_bev: rois (B, N, >= 7) fp32, features (B, C, H, W) fp32 in any strided layout (dense NCHW and
    channels_last are read without a copy), step = voxel size * downsample ratio -> (B * N, C, G, G) fp32, the reference's
    SECONDHead.roi_grid_pool.  d_n: optional int64[1] live row count over the B * N rows; rows past it are zeros.  Forward
    only: neither input receives a gradient (the reference detaches both).  No host read."""
    _need_gpu(rois, features)
    lib = _lib.load()
    if rois.dim() != 3 or rois.shape[2] < 7 or features.dim() != 4 or features.shape[0] != rois.shape[0] \
            or rois.dtype != torch.float32 or features.dtype != torch.float32:
        raise _lib.SpxError("roi_grid_pool_bev: rois %s (%s), features %s (%s) do not match"
                            % (tuple(rois.shape), rois.dtype, tuple(features.shape), features.dtype))
    rois = rois.detach().contiguous()
    features = features.detach()
    b, n, rs = rois.shape
    _, c, h, w = features.shape
    g = int(grid_size)
    sb, sc, sh, sw = features.stride()
    if min(sc, sh, sw) < 1 or sb < 0:                 # an expanded (stride 0) view has no single element per index
        features = features.contiguous()
        sb, sc, sh, sw = features.stride()
    d_n = _d_n("roi_grid_pool_bev: d_n", d_n, rois.device)
    out = torch.empty((b * n, c, g, g), dtype=torch.float32, device=rois.device)
    check(lib.spx_roi_grid_pool_bev(_ptr(rois), b, n, rs, _ptr(d_n), _ptr(features), c, h, w, sb, sc, sh, sw, g,
                                    float(min_x), float(min_y), float(step_x), float(step_y), _ptr(out), _stream(rois)),
          "spx_roi_grid_pool_bev")
    return out


def proposal_sample(rois, roi_labels, gt_boxes, roi_per_image, fg_per_image, reg_fg_thresh, cls_fg_thresh,
                    cls_bg_thresh_lo, hard_bg_ratio, by_class, fg_keys, slot_u):
    """spx_proposal_sample: rois (B, R, >= 7) fp32, roi_labels (B, R) int64, gt_boxes (B, G, >= 8) fp32 with the class
    last, fg_keys (B, R) and slot_u (B, M) fp32 uniform draws -> sampled_inds (B, M) int64, roi_ious (B, M) fp32, gt_inds
    (B, M) int64: the reference's ProposalTargetLayer.sample_rois_for_rcnn with its random numbers as inputs
    (include/spx.h §26).  fg_per_image = int(round(FG_RATIO * M)).  No host read."""
    _need_gpu(rois, roi_labels, gt_boxes, fg_keys, slot_u)
    lib = _lib.load()
    m = int(roi_per_image)
    if rois.dim() != 3 or rois.shape[2] < 7 or gt_boxes.dim() != 3 or gt_boxes.shape[2] < 8 or rois.shape[1] < 1 \
            or gt_boxes.shape[0] != rois.shape[0] or tuple(roi_labels.shape) != tuple(rois.shape[:2]) \
            or tuple(fg_keys.shape) != tuple(rois.shape[:2]) or tuple(slot_u.shape) != (rois.shape[0], m):
        raise _lib.SpxError("proposal_sample: rois %s, roi_labels %s, gt_boxes %s, fg_keys %s, slot_u %s do not match"
                            % (tuple(rois.shape), tuple(roi_labels.shape), tuple(gt_boxes.shape), tuple(fg_keys.shape),
                               tuple(slot_u.shape)))
    rois, gt_boxes, fg_keys, slot_u = _f32(rois), _f32(gt_boxes), _f32(fg_keys), _f32(slot_u)
    roi_labels = roi_labels.to(torch.int64).contiguous()
    b, r, rs = rois.shape
    if gt_boxes.shape[1] == 0:                        # the reference samples against one all-zero row
        gt_boxes = gt_boxes.new_zeros((b, 1, gt_boxes.shape[2]))
    gmax, gs = gt_boxes.shape[1], gt_boxes.shape[2]
    dev = rois.device
    sampled = torch.empty((b, m), dtype=torch.int64, device=dev)
    ious = torch.empty((b, m), dtype=torch.float32, device=dev)
    gt_inds = torch.empty((b, m), dtype=torch.int64, device=dev)
    wsb = lib.spx_proposal_sample_ws_bytes(b, r, gmax)
    ws = workspace(dev, wsb)
    check(lib.spx_proposal_sample(_ptr(rois), _ptr(roi_labels), _ptr(gt_boxes), b, r, rs, gmax, gs, m, int(fg_per_image),
                                  float(reg_fg_thresh), float(cls_fg_thresh), float(cls_bg_thresh_lo), float(hard_bg_ratio),
                                  int(bool(by_class)), _ptr(fg_keys), _ptr(slot_u), _ptr(sampled), _ptr(ious),
                                  _ptr(gt_inds), _ptr(ws), wsb, _stream(rois)), "spx_proposal_sample")
    return sampled, ious, gt_inds


# ------------------------------------------------------------------------------ voxel-grid max pooling (§27)

def _voxel_pool_args(xyz, new_xyz, idx, empty, what):
    if xyz.dim() != 2 or xyz.shape[1] != 3 or new_xyz.dim() != 2 or new_xyz.shape[1] != 3 or idx.dim() != 2 \
            or idx.shape[0] != new_xyz.shape[0] or idx.shape[1] < 1 \
            or (empty is not None and tuple(empty.shape) != (new_xyz.shape[0],)):
        raise _lib.SpxError("%s: xyz %s, new_xyz %s, idx %s, empty %s do not match" % (
            what, tuple(xyz.shape), tuple(new_xyz.shape), tuple(idx.shape), None if empty is None else tuple(empty.shape)))
    empty = None if empty is None else empty.detach().contiguous().to(torch.uint8)
    return _f32(xyz), _f32(new_xyz), _i32(idx), empty


def voxel_pool_moments(xyz, new_xyz, idx, empty):
    """spx_voxel_pool_moments: xyz (N, 3), new_xyz (M, 3), idx (M, S) global rows, empty (M) bool / uint8 or None ->
    float64[9] = (sum d, upper triangle of sum d d^T) of the offsets d = xyz[idx] - new_xyz over all M * S columns, empty
    queries counting as zero columns (include/spx.h §27).  Fixed summation order; no host read."""
    _need_gpu(xyz, new_xyz, idx, empty)
    lib = _lib.load()
    xyz, new_xyz, idx, empty = _voxel_pool_args(xyz, new_xyz, idx, empty, "voxel_pool_moments")
    m, s = idx.shape
    out = torch.empty((9,), dtype=torch.float64, device=xyz.device)
    wsb = lib.spx_voxel_pool_moments_ws_bytes(m, s)
    ws = workspace(xyz.device, wsb)
    check(lib.spx_voxel_pool_moments(_ptr(xyz), _ptr(new_xyz), _ptr(idx), _ptr(empty), xyz.shape[0], m, s, _ptr(out),
                                     _ptr(ws), wsb, _stream(xyz)), "spx_voxel_pool_moments")
    return out


def voxel_pool_max_fwd(f, xyz, new_xyz, idx, empty, a, b):
    """spx_voxel_pool_max_fwd -> out (M, C) fp32, arg (M, C) int32 (the winning slot, -1 where out is 0)."""
    _need_gpu(f, xyz, new_xyz, idx, empty, a, b)
    lib = _lib.load()
    xyz, new_xyz, idx, empty = _voxel_pool_args(xyz, new_xyz, idx, empty, "voxel_pool_max")
    f, a, b = _f32(f), _f32(a), _f32(b)
    if f.dim() != 2 or f.shape[0] != xyz.shape[0] or f.shape[1] < 1 or tuple(a.shape) != (f.shape[1], 3) \
            or tuple(b.shape) != (f.shape[1],):
        raise _lib.SpxError("voxel_pool_max: f %s, xyz %s, a %s, b %s do not match"
                            % (tuple(f.shape), tuple(xyz.shape), tuple(a.shape), tuple(b.shape)))
    m, s = idx.shape
    n_src, c = f.shape
    out = torch.empty((m, c), dtype=torch.float32, device=f.device)
    arg = torch.empty((m, c), dtype=torch.int32, device=f.device)
    check(lib.spx_voxel_pool_max_fwd(_ptr(f), _ptr(xyz), _ptr(new_xyz), _ptr(idx), _ptr(empty), _ptr(a), _ptr(b), c, n_src,
                                     m, s, _ptr(out), _ptr(arg), _stream(f)), "spx_voxel_pool_max_fwd")
    return out, arg


def voxel_pool_max_bwd(dout, arg, xyz, new_xyz, idx, empty, n_src):
    """spx_voxel_pool_max_bwd: dout (M, C), arg from the forward -> df (n_src, C), dA (C, 3), db (C), all summed in a
    fixed order."""
    _need_gpu(dout, arg, xyz, new_xyz, idx, empty)
    lib = _lib.load()
    xyz, new_xyz, idx, empty = _voxel_pool_args(xyz, new_xyz, idx, empty, "voxel_pool_max_bwd")
    dout, arg = _f32(dout), _i32(arg)
    m, s = idx.shape
    if dout.dim() != 2 or dout.shape[0] != m or tuple(arg.shape) != tuple(dout.shape) or int(n_src) != xyz.shape[0]:
        raise _lib.SpxError("voxel_pool_max_bwd: dout %s, arg %s, idx %s, n_src %d do not match"
                            % (tuple(dout.shape), tuple(arg.shape), tuple(idx.shape), int(n_src)))
    c = dout.shape[1]
    dev = dout.device
    df = torch.empty((int(n_src), c), dtype=torch.float32, device=dev)
    da = torch.empty((c, 3), dtype=torch.float32, device=dev)
    db = torch.empty((c,), dtype=torch.float32, device=dev)
    wsb = lib.spx_voxel_pool_max_bwd_ws_bytes(c, int(n_src), m, s)
    ws = workspace(dev, wsb)
    check(lib.spx_voxel_pool_max_bwd(_ptr(dout), _ptr(arg), _ptr(idx), _ptr(empty), _ptr(xyz), _ptr(new_xyz), c, int(n_src),
                                     m, s, _ptr(df), _ptr(da), _ptr(db), _ptr(ws), wsb, _stream(dout)),
          "spx_voxel_pool_max_bwd")
    return df, da, db


class _VoxelPoolMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, xyz, new_xyz, idx, empty, a, b):
        out, arg = voxel_pool_max_fwd(f, xyz, new_xyz, idx, empty, a, b)
        ctx.save_for_backward(arg, xyz, new_xyz, idx, empty)
        ctx.n_src = f.shape[0]
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        arg, xyz, new_xyz, idx, empty = ctx.saved_tensors
        df, da, db = voxel_pool_max_bwd(dout, arg, xyz, new_xyz, idx, empty, ctx.n_src)
        return df, None, None, None, None, da, db


def voxel_pool_max(f, xyz, new_xyz, idx, empty, a, b, return_arg=False):
    """out (M, C) = max(0, max_s f[idx[m, s]] + a . (xyz[idx[m, s]] - new_xyz[m]) + b), the pooling tail of
    NeighborVoxelSAModuleMSG with its BatchNorm folded into (a, b) (include/spx.h §27).  f (N, C), xyz (N, 3), new_xyz
    (M, 3), idx (M, S) global rows, empty (M) bool, a (C, 3), b (C).  Differentiable in f, a, b; nothing flows to the
    coordinates.  return_arg: also the winning slots (M, C) int32."""
    _need_gpu(f, xyz, new_xyz, idx, empty, a, b)
    if empty is None:
        empty = torch.zeros((new_xyz.shape[0],), dtype=torch.bool, device=new_xyz.device)
    out, arg = _VoxelPoolMax.apply(f, xyz.detach(), new_xyz.detach(), idx, empty, a, b)
    return (out, arg) if return_arg else out


# ------------------------------------------------------------------------------ two-layer SA-MLP max pooling (§28)

SA_MLP2_CHANNELS = (16, 32, 64)
SA_MLP2_NSAMPLE = (16, 32)


def sa_mlp2_supported(c1, c2, nsample):
    """Whether spx_sa_mlp2_max has a kernel for this shape (PV-RCNN's pointnets)."""
    return c1 in SA_MLP2_CHANNELS and c2 in SA_MLP2_CHANNELS and nsample in SA_MLP2_NSAMPLE


def sa_mlp2_max(P, xyz, new_xyz, idx, empty, Wx, a1, b1, W2, a2, b2):
    """out (M, C2) = max_s relu(a2 * (W2 h[m, s]) + b2), h[m, s] = relu(a1 * (P[r] + Wx (xyz[r] - new_xyz[m])) + b1),
    r = idx[m, s]: the eval-mode tail of a two-layer stacked SA pointnet with both BatchNorms folded (include/spx.h §28).
    P (N, C1) = features @ Wf^T or None, xyz (N, 3), new_xyz (M, 3), idx (M, S) int32 GLOBAL rows, empty (M) bool or
    None, Wx (C1, 3), a1 / b1 (C1), W2 (C2, C1), a2 / b2 (C2), fp32.  An empty ball, and a row of idx outside [0, N), is a
    zero column (h = relu(b1)), not a zero output.  Forward only: tensors that require grad are refused.  C1, C2 in
    {16, 32, 64} and S in {16, 32}; anything else raises SpxError.  No host read; capturable; bitwise reproducible."""
    named = (("P", P), ("xyz", xyz), ("new_xyz", new_xyz), ("idx", idx), ("empty", empty), ("Wx", Wx), ("a1", a1),
             ("b1", b1), ("W2", W2), ("a2", a2), ("b2", b2))
    _need_gpu(*[t for _, t in named])
    for name, t in named:
        if t is not None and t.requires_grad:
            raise _lib.SpxError("sa_mlp2_max: %s requires grad; the op is forward only (detach it, or use the "
                                "composition to train)" % name)
    for name, t in named:
        if t is not None and name not in ("idx", "empty") and t.dtype != torch.float32:
            raise _lib.SpxError("sa_mlp2_max: %s is %s; the op is fp32 in and out" % (name, t.dtype))
    lib = _lib.load()
    xyz, new_xyz, idx, empty = _voxel_pool_args(xyz, new_xyz, idx, empty, "sa_mlp2_max")
    Wx, a1, b1, W2, a2, b2 = _f32(Wx), _f32(a1), _f32(b1), _f32(W2), _f32(a2), _f32(b2)
    m, s = idx.shape
    n_src = xyz.shape[0]
    c2, c1 = (W2.shape if W2.dim() == 2 else (0, 0))
    if not sa_mlp2_supported(c1, c2, s):
        raise _lib.SpxError("sa_mlp2_max: unsupported shape C1 = %d, C2 = %d, S = %d; C1 and C2 must be in %s and S in %s"
                            % (c1, c2, s, SA_MLP2_CHANNELS, SA_MLP2_NSAMPLE))
    if tuple(Wx.shape) != (c1, 3) or tuple(a1.shape) != (c1,) or tuple(b1.shape) != (c1,) or tuple(a2.shape) != (c2,) \
            or tuple(b2.shape) != (c2,) or (P is not None and tuple(P.shape) != (n_src, c1)):
        raise _lib.SpxError("sa_mlp2_max: P %s, xyz %s, Wx %s, a1 %s, b1 %s, W2 %s, a2 %s, b2 %s do not match" % (
            None if P is None else tuple(P.shape), tuple(xyz.shape), tuple(Wx.shape), tuple(a1.shape), tuple(b1.shape),
            tuple(W2.shape), tuple(a2.shape), tuple(b2.shape)))
    if P is not None:
        P = _f32(P)
        if P.data_ptr() % 16:
            P = P.clone()
    out = torch.empty((m, c2), dtype=torch.float32, device=xyz.device)
    check(lib.spx_sa_mlp2_max(_ptr(P), _ptr(xyz), _ptr(new_xyz), _ptr(idx), _ptr(empty), _ptr(Wx), _ptr(a1), _ptr(b1),
                              _ptr(W2), _ptr(a2), _ptr(b2), c1, c2, n_src, m, s, _ptr(out), _stream(xyz)),
          "spx_sa_mlp2_max")
    return out


# ------------------------------------------------------------------- dense-prediction post-processing (§29)

DENSE_POST_PROCESS_MAX_PRE = 16384   # candidates per (frame, class) that go into an NMS: their keys sit in one CU's LDS


def _dense_args(what, scores, labels, boxes, batch_size, thresholds, pre_max, post_max, per_class):
    """The shape and limit checks the two dense ops share -> (b, n, thresholds or None, n_thresh).  Host values only."""
    b = int(batch_size)
    if thresholds is not None:
        thresholds = [float(t) for t in (thresholds if isinstance(thresholds, (list, tuple)) else [thresholds])]
    bad = scores.dim() != 1 or labels.shape != scores.shape or b < 0 or (b == 0 and scores.shape[0] != 0) \
        or (b > 0 and scores.shape[0] % b != 0)
    if boxes is not None:
        bad = bad or boxes.dim() != 2 or boxes.shape[0] != scores.shape[0] or boxes.shape[1] < 7
    if bad:
        raise _lib.SpxError("%s: scores %s, labels %s%s do not make %d equal frames"
                            % (what, tuple(scores.shape), tuple(labels.shape),
                               "" if boxes is None else ", boxes %s" % (tuple(boxes.shape),), b))
    nt = 1 if thresholds is None else len(thresholds)
    if not per_class and nt != 1:
        raise _lib.SpxError("%s: class-agnostic mode takes one threshold, got %d" % (what, nt))
    if thresholds is None and per_class:
        raise _lib.SpxError("%s: thresholds=None (no threshold) goes with per_class=False" % what)
    if not 1 <= nt <= 8:
        raise _lib.SpxError("%s: 1 .. 8 thresholds, got %d" % (what, nt))
    if not 1 <= int(pre_max) <= DENSE_POST_PROCESS_MAX_PRE:
        raise _lib.SpxError("%s: pre_max %d outside 1 .. %d" % (what, int(pre_max), DENSE_POST_PROCESS_MAX_PRE))
    if post_max is not None and int(post_max) < 1:
        raise _lib.SpxError("%s: post_max %d < 1" % (what, int(post_max)))
    if scores.shape[0] >= 2 ** 31 or b > 65535:
        raise _lib.SpxError("%s: %d rows in %d frames are too many" % (what, scores.shape[0], b))
    n = scores.shape[0] // b if b > 0 else 0
    if post_max is not None and nt * min(int(post_max), int(pre_max), max(n, 1)) > POST_PROCESS_MAX_N:
        raise _lib.SpxError("%s: %d classes x %d kept boxes exceed the %d survivors the final stage takes"
                            % (what, nt, min(int(post_max), int(pre_max), n), POST_PROCESS_MAX_N))
    return b, n, thresholds, nt


def dense_select(scores, labels, batch_size, thresholds, pre_max, per_class=True):
    """spx_dense_select: scores (B * n) normalised, labels (B * n) 1-based, frames contiguous with n rows each (any n);
    thresholds one float per class (per_class), a single one, or None for no threshold (per_class=False) ->
    cand (B, T, pre_max) int64: per (frame, class) the members by score descending, equal scores lower row first, as rows
    of the input, -1 past the count; count (B, T) int32.  A NaN score is never a member.  No host read."""
    b, n, thresholds, nt = _dense_args("dense_select", scores, labels, None, batch_size, thresholds, pre_max, None,
                                       per_class)
    _need_gpu(scores, labels)
    lib = _lib.load()
    dev = scores.device
    pre_max = int(pre_max)
    if b * n == 0:
        return (torch.full((b, nt, pre_max), -1, dtype=torch.int64, device=dev),
                torch.zeros((b, nt), dtype=torch.int32, device=dev))
    scores, labels = _f32(scores), _i32(labels)
    cand = torch.empty((b, nt, pre_max), dtype=torch.int64, device=dev)
    count = torch.empty((b, nt), dtype=torch.int32, device=dev)
    wsb = lib.spx_dense_select_ws_bytes(b, n, nt, pre_max)
    ws = workspace(dev, wsb)
    check(lib.spx_dense_select(_ptr(scores), _ptr(labels), b, n, None if thresholds is None else f_arr(thresholds), nt,
                               pre_max, int(bool(per_class)), _ptr(cand), _ptr(count), _ptr(ws), wsb, _stream(scores)),
          "spx_dense_select")
    return cand, count


def dense_post_process(scores, labels, boxes, batch_size, thresholds, nms_thresh, pre_max, post_max, axis_aligned=False,
                       per_class=True):
    """spx_dense_post_process: point_post_process for any n -- scores (B * n) normalised, labels (B * n) 1-based, boxes
    (B * n, >= 7) read by their row stride; thresholds one float per class (per_class, the fork's multi_thresh), a single
    one (class-agnostic NMS) or None (no threshold, per_class=False: proposals) -> the dict of point_post_process: sel
    (B, K) int64 rows of the input or -1, count (B) int32, boxes (B, K, 7), scores (B, K), labels (B, K) int64, zeros
    past count.  pre_max <= DENSE_POST_PROCESS_MAX_PRE.  No host read."""
    b, n, thresholds, nt = _dense_args("dense_post_process", scores, labels, boxes, batch_size, thresholds, pre_max,
                                       post_max, per_class)
    _need_gpu(scores, labels, boxes)
    lib = _lib.load()
    dev = scores.device
    scores, labels, boxes = _f32(scores), _i32(labels), boxes.detach()
    if boxes.dtype != torch.float32 or boxes.stride(1) != 1 or boxes.stride(0) < boxes.shape[1] or b * n == 0:
        boxes = boxes.contiguous().float()
    k = int(lib.spx_point_post_process_capacity(n, nt, int(post_max), int(bool(per_class))))
    out = {"sel": torch.empty((b, k), dtype=torch.int64, device=dev),
           "count": torch.empty((b,), dtype=torch.int32, device=dev),
           "boxes": torch.empty((b, k, 7), dtype=torch.float32, device=dev),
           "scores": torch.empty((b, k), dtype=torch.float32, device=dev),
           "labels": torch.empty((b, k), dtype=torch.int64, device=dev)}
    if b * k == 0:
        out["count"].zero_()      # frames without candidates: nothing to launch (and no storage to point at)
        return out
    wsb = lib.spx_dense_post_process_ws_bytes(b, n, nt, int(pre_max), int(post_max))
    ws = workspace(dev, wsb)
    check(lib.spx_dense_post_process(_ptr(scores), _ptr(labels), _ptr(boxes), boxes.stride(0), b, n,
                                     None if thresholds is None else f_arr(thresholds), nt, float(nms_thresh),
                                     int(pre_max), int(post_max), int(bool(axis_aligned)), int(bool(per_class)),
                                     _ptr(out["sel"]), _ptr(out["count"]), _ptr(out["boxes"]), _ptr(out["scores"]),
                                     _ptr(out["labels"]), _ptr(ws), wsb, _stream(scores)), "spx_dense_post_process")
    return out


# ------------------------------------------------- sparse batched RoI-aware pooling, ragged points in boxes (§30)

def points_in_boxes_stack(points_bxyz, boxes):
    """spx_points_in_boxes_stack: points (P, 4) [frame, x, y, z] (frames of any length, any row order), boxes (B, M, 7)
    -> (P) int32: the first box of the point's own frame holding it, or -1 (also for a frame outside [0, B))."""
    _need_gpu(points_bxyz, boxes)
    lib = _lib.load()
    if points_bxyz.dim() != 2 or points_bxyz.shape[1] != 4 or boxes.dim() != 3 or boxes.shape[2] != 7:
        raise _lib.SpxError("points_in_boxes_stack: points %s, boxes %s do not match (P, 4), (B, M, 7)"
                            % (tuple(points_bxyz.shape), tuple(boxes.shape)))
    points_bxyz, boxes = _f32(points_bxyz), _f32(boxes)
    p = points_bxyz.shape[0]
    out = torch.empty((p,), dtype=torch.int32, device=points_bxyz.device)
    check(lib.spx_points_in_boxes_stack(_ptr(points_bxyz), _ptr(boxes), boxes.shape[0], p, boxes.shape[1], _ptr(out),
                                        _stream(points_bxyz)), "spx_points_in_boxes_stack")
    return out


def frame_layout(bs_idx, batch_size):
    """Rows per frame as a device int32 (B) (counted by comparison, as VoxelSetAbstraction.frame_counts: no bincount, no
    host read) and the 0-dim device bool `layout_ok`: the rows are grouped by ascending frame."""
    frames = torch.arange(batch_size, device=bs_idx.device, dtype=bs_idx.dtype)
    cnt = (bs_idx.reshape(-1, 1) == frames.view(1, -1)).sum(dim=0).int()
    ok = (bs_idx[1:] >= bs_idx[:-1]).all() & (cnt.sum() == bs_idx.numel())
    return cnt, ok


class RoiawareSparseState(object):
    """What roiaware_sparse_collect hands to roiaware_sparse_pool: the inputs, the device record of the collection
    (`ws`), and the device scalars n_rows (int64[1]), faked (int32[1]) and layout_ok (0-dim bool)."""
    __slots__ = ("rois", "points", "part", "rpn", "part_in", "rpn_in", "frame_cnt", "layout_ok", "b", "n_per", "np",
                 "pf", "out_size", "max_pts", "ws", "n_rows", "faked")


def roiaware_sparse_collect(rois, points, part, rpn, out_size, max_pts_each_voxel, frame_cnt=None,
                            max_frame_points=None):
    """spx_roiaware_sparse_collect: rois (B, N, 7), points (P, 4) [frame, x, y, z] grouped by ascending frame, part
    (P, 4) non-negative, rpn (P, C); frame_cnt the device int32 (B) rows per frame (None: frame_layout of the frame
    column); max_frame_points a host bound on the longest frame (None: P) -> RoiawareSparseState.  Per RoI the point
    lists, the cell counts and which cells are emitted; the scan over the B * N RoIs; n_rows and faked on the device.
    No host read: the caller decides who reads n_rows."""
    _need_gpu(rois, points, part, rpn, frame_cnt)
    lib = _lib.load()
    if rois.dim() != 3 or rois.shape[2] != 7 or points.dim() != 2 or points.shape[1] != 4 or part.dim() != 2 \
            or tuple(part.shape) != (points.shape[0], 4) or rpn.dim() != 2 or rpn.shape[0] != points.shape[0]:
        raise _lib.SpxError("roiaware_sparse_collect: rois %s, points %s, part %s, rpn %s do not match (B, N, 7), (P, 4), "
                            "(P, 4), (P, C)" % (tuple(rois.shape), tuple(points.shape), tuple(part.shape),
                                                tuple(rpn.shape)))
    st = RoiawareSparseState()
    st.part_in, st.rpn_in = part, rpn
    st.rois, st.points, st.part, st.rpn = _f32(rois), _f32(points), _f32(part), _f32(rpn)
    dev = st.points.device
    st.b, st.n_per, st.np = int(rois.shape[0]), int(rois.shape[1]), int(points.shape[0])
    if frame_cnt is None:
        st.frame_cnt, st.layout_ok = frame_layout(st.points[:, 0], st.b)
    else:
        if frame_cnt.dtype != torch.int32 or frame_cnt.numel() != st.b:
            raise _lib.SpxError("roiaware_sparse_collect: frame_cnt must be int32 (%d)" % st.b)
        st.frame_cnt, st.layout_ok = frame_cnt.contiguous(), torch.ones((), dtype=torch.bool, device=dev)
    st.pf = st.np if max_frame_points is None else min(int(max_frame_points), st.np)
    st.out_size = tuple(int(v) for v in out_size)
    st.max_pts = int(max_pts_each_voxel)
    ox, oy, oz = st.out_size
    wsb = lib.spx_roiaware_sparse_ws_bytes(st.b, st.n_per, st.pf, ox, oy, oz)
    st.ws = torch.empty((max(int(wsb), 4),), dtype=torch.uint8, device=dev)
    st.n_rows = torch.empty((1,), dtype=torch.int64, device=dev)
    st.faked = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib.spx_roiaware_sparse_collect(_ptr(st.rois), _ptr(st.points), _ptr(st.frame_cnt), _ptr(st.part), st.b,
                                          st.n_per, st.np, st.pf, ox, oy, oz, st.max_pts, _ptr(st.n_rows),
                                          _ptr(st.faked), _ptr(status_word(dev)), _ptr(st.ws), wsb, _stream(st.points)),
          "spx_roiaware_sparse_collect")
    return st


def roiaware_sparse_pool_fwd(st, rows):
    """spx_roiaware_sparse_pool on the state of roiaware_sparse_collect -> coords (rows, 4) int32 [r, x, y, z], part
    (rows, 4), rpn (rows, C), arg (rows, C) int32 (point rows), cnt (rows) int32, row_of_cell (B * N * V) int32.  Rows at
    and past n_rows are dead (features 0, coords -1); n_rows > rows sets the status word (check_status)."""
    lib = _lib.load()
    rows = int(rows)
    dev = st.points.device
    c = st.rpn.shape[1]
    ox, oy, oz = st.out_size
    coords = torch.empty((rows, 4), dtype=torch.int32, device=dev)
    out_part = torch.empty((rows, 4), dtype=torch.float32, device=dev)
    out_rpn = torch.empty((rows, c), dtype=torch.float32, device=dev)
    arg = torch.empty((rows, c), dtype=torch.int32, device=dev)
    cnt = torch.empty((rows,), dtype=torch.int32, device=dev)
    row_of_cell = torch.empty((st.b * st.n_per * ox * oy * oz,), dtype=torch.int32, device=dev)
    check(lib.spx_roiaware_sparse_pool(_ptr(st.part), _ptr(st.rpn), st.b, st.n_per, st.np, st.pf, c, ox, oy, oz, rows,
                                       _ptr(st.n_rows), _ptr(st.faked), _ptr(row_of_cell), _ptr(coords), _ptr(out_part),
                                       _ptr(out_rpn), _ptr(arg), _ptr(cnt), _ptr(status_word(dev)), _ptr(st.ws),
                                       st.ws.numel(), _stream(st.points)), "spx_roiaware_sparse_pool")
    return coords, out_part, out_rpn, arg, cnt, row_of_cell


def roiaware_sparse_pool_bwd(st, grad, arg, cnt, row_of_cell, pool_method):
    """spx_roiaware_sparse_bwd: grad (rows, C) -> (P, C); pool_method 0 = max (arg), 1 = avg (cnt).  Fixed order."""
    lib = _lib.load()
    grad = _f32(grad)
    rows, c = grad.shape
    ox, oy, oz = st.out_size
    grad_in = torch.empty((st.np, c), dtype=torch.float32, device=grad.device)
    check(lib.spx_roiaware_sparse_bwd(_ptr(grad), _ptr(arg), _ptr(cnt), _ptr(row_of_cell), _ptr(st.frame_cnt), st.b,
                                      st.n_per, st.np, st.pf, c, ox, oy, oz, rows, int(pool_method), _ptr(grad_in),
                                      _ptr(st.ws), st.ws.numel(), _stream(grad)), "spx_roiaware_sparse_bwd")
    return grad_in


class _RoiawareSparsePool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, part, rpn, st, rows):
        coords, out_part, out_rpn, arg, cnt, row_of_cell = roiaware_sparse_pool_fwd(st, rows)
        # The state (frame counts, the collection record) rides on ctx, not in save_for_backward, so autograd does not
        # notice an in-place change of part / rpn between forward and backward.  That is harmless: the backward reads
        # neither input, only grad, arg, cnt, row_of_cell (saved below) and the record of which point lies in which cell.
        ctx.st = st
        ctx.save_for_backward(arg, cnt, row_of_cell)
        ctx.mark_non_differentiable(coords, arg, cnt, row_of_cell)
        return out_part, out_rpn, coords, arg, cnt, row_of_cell

    @staticmethod
    def backward(ctx, d_part, d_rpn, *_unused):
        arg, cnt, row_of_cell = ctx.saved_tensors
        g_part = roiaware_sparse_pool_bwd(ctx.st, d_part, None, cnt, row_of_cell, 1) if ctx.needs_input_grad[0] else None
        g_rpn = roiaware_sparse_pool_bwd(ctx.st, d_rpn, arg, None, row_of_cell, 0) if ctx.needs_input_grad[1] else None
        return g_part, g_rpn, None, None


def roiaware_sparse_pool(st, rows):
    """The second call of the fused RoI-aware pooling (include/spx.h §30): writes `rows` rows (a capacity: the caller's
    host copy of st.n_rows, or a static cap) -> dict(coords, part, rpn, arg, cnt, row_of_cell, n_rows, faked, layout_ok).
    Differentiable in the part and rpn tensors given to roiaware_sparse_collect."""
    out_part, out_rpn, coords, arg, cnt, row_of_cell = _RoiawareSparsePool.apply(st.part_in, st.rpn_in, st, int(rows))
    return {"coords": coords, "part": out_part, "rpn": out_rpn, "arg": arg, "cnt": cnt, "row_of_cell": row_of_cell,
            "n_rows": st.n_rows, "faked": st.faked, "layout_ok": st.layout_ok}
