"""Times the roiaware_pool3d ops (include/spx.h §12) at the fork's shapes with HIP events; prints one table.

  python tools/roiaware_bench.py [--iters N]

points_in_boxes is reported beside its HBM floor of 16 bytes per point (12 read, 4 written; the boxes are noise), and
in microseconds per call: at the KITTI size it is launch-bound.  The head's pattern is two calls per frame (gt boxes,
then the enlarged boxes), 2 * B calls per batch; the batched row is one call over the whole batch.  The pooling forward
is reported beside the write of pooled (+ argmax for max), the backward beside the write of grad_in plus the read of
the per-(RoI, point) record."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BPS = 8.0e12


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters      # microseconds


def kitti(batch, m, seed=0):
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    pts, gts = [], []
    for i in range(batch):
        f = syn.make_frame(1, i)
        p = f["points"][:, :3]
        pts.append(p[rng.choice(p.shape[0], m, replace=p.shape[0] < m)])
        gts.append(f["gt_boxes"][:, :7])
    t = max(g.shape[0] for g in gts)
    gt = np.zeros((batch, t, 7), np.float32)
    for i, g in enumerate(gts):
        gt[i, :g.shape[0]] = g
    return np.stack(pts).astype(np.float32), gt


def rois_around(gt, n, seed):
    rng = np.random.default_rng(seed)
    base = gt[rng.integers(0, gt.shape[0], n)].astype(np.float64)
    base[:, 0:3] += rng.normal(scale=0.3, size=(n, 3))
    base[:, 3:6] *= rng.uniform(0.9, 1.3, size=(n, 3))
    return base.astype(np.float32)


def floor_us(nbytes):
    return nbytes / HBM_BPS * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from pcdet_amd.ops.roiaware_pool3d import roiaware_pool3d_utils as ru
    from pcdet_amd.utils import box_utils
    from spx import ops
    dev = torch.device("cuda:0")
    rows = []

    pts_np, gt_np = kitti(16, 16384)
    pts, gt = torch.from_numpy(pts_np).to(dev), torch.from_numpy(gt_np).to(dev)
    gt40 = torch.zeros((16, 40, 7), device=dev)
    gt40[:, :gt.shape[1]] = gt
    ext = box_utils.enlarge_box3d(gt40.view(-1, 7), extra_width=(0.2, 0.2, 0.2)).view(16, 40, 7).contiguous()

    def per_frame():
        for k in range(16):
            ru.points_in_boxes_gpu(pts[k:k + 1], gt40[k:k + 1])
            ru.points_in_boxes_gpu(pts[k:k + 1], ext[k:k + 1])
    t = timed(per_frame, args.iters)
    rows.append(("KITTI pib per frame 16x(gt+ext) m=16384 t=40", t, "%.1f us/call; HBM floor %.2f us/call"
                 % (t / 32, floor_us(16384 * 16))))
    t = timed(lambda: ru.points_in_boxes_gpu(pts, gt40), args.iters)
    rows.append(("KITTI pib batched b=16 m=16384 t=40", t, "HBM floor %.2f us (%.1f%%)"
                 % (floor_us(16 * 16384 * 16), 100 * floor_us(16 * 16384 * 16) / t)))

    from pcdet_amd.datasets import synthetic as syn
    f = syn.make_frame(3, 0)
    wp = torch.from_numpy(np.stack([f["points"][:163840, :3], f["points"][-163840:, :3]]).astype(np.float32)).to(dev)
    wb = torch.from_numpy(np.stack([rois_around(f["gt_boxes"][:, :7], 200, s) for s in (1, 2)])).to(dev)
    t = timed(lambda: ru.points_in_boxes_gpu(wp, wb), args.iters)
    rows.append(("Waymo pib b=2 m=163840 t=200", t, "HBM floor %.2f us (%.1f%%)"
                 % (floor_us(2 * 163840 * 16), 100 * floor_us(2 * 163840 * 16) / t)))
    del wp, wb

    n, npt = 128, 16384
    rois = torch.from_numpy(rois_around(gt_np[0][gt_np[0, :, 3] > 0], n, 3)).to(dev)
    ppts = pts[0].contiguous()
    V = 14 ** 3
    for c in (128, 4):
        feats = torch.randn(npt, c, device=dev)
        for mode, name in ((0, "max"), (1, "avg")):
            t = timed(lambda: ops.roiaware_pool3d_fwd(rois, ppts, feats, (14, 14, 14), 128, mode), args.iters)
            wbytes = n * V * c * 4 * (2 if mode == 0 else 1)
            rows.append(("PartA2 pool fwd %s n=128 np=16384 14^3 c=%d" % (name, c), t, "write floor %.1f us (%.1f%%)"
                         % (floor_us(wbytes), 100 * floor_us(wbytes) / t)))
            pooled, argmax, pt_cell, vox_cnt = ops.roiaware_pool3d_fwd(rois, ppts, feats, (14, 14, 14), 128, mode)
            go = torch.randn_like(pooled)
            t = timed(lambda: ops.roiaware_pool3d_bwd(go, argmax, pt_cell, vox_cnt, mode), args.iters)
            bbytes = npt * c * 4 + n * npt * 4
            rows.append(("PartA2 pool bwd %s c=%d (deterministic)" % (name, c), t, "floor %.1f us (%.1f%%)"
                         % (floor_us(bbytes), 100 * floor_us(bbytes) / t)))
            del pooled, argmax, pt_cell, vox_cnt, go
        del feats

    print("%-50s %14s  %s" % ("op", "time (us)", "rate"))
    for name, t, rate in rows:
        print("%-50s %14.1f  %s" % (name, t, rate))


if __name__ == "__main__":
    main()
