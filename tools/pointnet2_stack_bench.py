"""Times the stacked point ops (include/spx.h §18, csrc/pointnet2_stack.hip) at PV-RCNN's shapes against an eager torch
composition of the same results; prints one table and writes it to profiles/pointnet2_stack_bench.log.

  python tools/pointnet2_stack_bench.py [--iters N] [--out FILE]

Batch 4, KITTI-shaped synthetic frames of 16384 points.  The shapes are upstream PV-RCNN's (the fork ships no such yaml)
and are constants of this file: 2048 keypoints per frame by the stack FPS; QueryAndGroup of the keypoints against the
raw points (r 0.4 / 0.8, nsample 16) and against the x_conv3 voxel centres (r 1.2 / 2.4, nsample 16 / 32); RoI-grid
pooling of 128 x 216 grid points per frame against the keypoints (r 0.8 / 1.6, nsample 16, C = 128), forward and
backward; one StackPointnetFPModule from the keypoints back to the raw points.

The baseline is written here, per frame: chunked torch.cdist, a stable argsort of the miss mask for "the first nsample
hits", an index gather, and index_add_ for the backward.  (No CUDA build of the reference exists for this hardware.)  Its
distances come from cdist (a square root, in its difference form), so a hit exactly at the radius may differ; the share
of equal index rows is printed, and the backward is compared on the fused path's own index lists.  There is
no FPS baseline: an eager FPS is one tiny launch chain per pick.  Times are HIP-event times around windows of
back-to-back calls, the median of five alternating windows of baseline and fused after a warm-up, in one process; spread =
the largest |window / median - 1| of either path."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH, POINTS, KEYPOINTS = 4, 16384, 2048
ROIS, GRID = 128, 6                      # 128 RoIs x 6^3 = 216 grid points
RANGE = np.array([0, -40, -3, 70.4, 40, 1], np.float32)
CONV3_VOXEL = np.array([0.2, 0.2, 0.4], np.float32)      # voxel size 0.05 x 0.05 x 0.1 at stride 4
EXACT = "donot_use_mm_for_euclid_dist"   # cdist's matmul form is off by millimetres at 70 m and would pick other neighbours


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters      # microseconds


def timed_pair(eager, fused, iters, reps=5):
    for _ in range(2):
        eager()
        fused()
    torch.cuda.synchronize()
    te, tf = [], []
    for _ in range(reps):
        te.append(window(eager, iters))
        tf.append(window(fused, 4 * iters))
    me, mf = float(np.median(te)), float(np.median(tf))
    return me, mf, max(max(abs(t / me - 1) for t in te), max(abs(t / mf - 1) for t in tf))


def timed_one(fn, iters, reps=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = [window(fn, iters) for _ in range(reps)]
    m = float(np.median(t))
    return m, max(abs(x / m - 1) for x in t)


def make_frames():
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(0)
    out = []
    for i in range(BATCH):
        pts = syn.make_frame(1, i)["points"][:, :4]
        out.append(pts[rng.choice(pts.shape[0], POINTS, replace=pts.shape[0] < POINTS)])
    return np.ascontiguousarray(np.concatenate(out).astype(np.float32))


def conv3_centres(points):
    """centres of the occupied stride-4 cells of every frame, stacked, and their counts"""
    out, cnt = [], []
    for f in range(BATCH):
        p = points[f * POINTS:(f + 1) * POINTS, :3]
        cells = np.unique(np.floor((p - RANGE[:3]) / CONV3_VOXEL).astype(np.int64), axis=0)
        out.append(((cells + 0.5) * CONV3_VOXEL + RANGE[:3]).astype(np.float32))
        cnt.append(cells.shape[0])
    return np.concatenate(out), cnt


def roi_grid(keypoints, rng):
    """128 car-sized boxes per frame centred on keypoints, 6 x 6 x 6 grid points each"""
    lin = (np.arange(GRID, dtype=np.float32) + 0.5) / GRID - 0.5
    cell = np.stack(np.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3) * np.array([3.9, 1.6, 1.56], np.float32)
    out = []
    for f in range(BATCH):
        centres = keypoints[f * KEYPOINTS + rng.choice(KEYPOINTS, ROIS, replace=False)]
        out.append((centres[:, None, :] + cell[None, :, :]).reshape(-1, 3))
    return np.concatenate(out).astype(np.float32)


def eager_query(xyz, n_cnt, new_xyz, m_cnt, radius, nsample, chunk=4096):
    """-> global rows (M, nsample) and the empty mask, frame by frame"""
    rows, empty, n0, m0 = [], [], 0, 0
    for n, m in zip(n_cnt, m_cnt):
        p = xyz[n0:n0 + n]
        for q0 in range(m0, m0 + m, chunk):
            q = new_xyz[q0:min(q0 + chunk, m0 + m)]
            hit = torch.cdist(q, p, compute_mode=EXACT) < radius
            first = torch.argsort(~hit, dim=1, stable=True)[:, :nsample]
            cnt = hit.sum(dim=1).clamp(max=nsample)
            sel = torch.where(torch.arange(nsample, device=q.device)[None, :] < cnt[:, None], first, first[:, :1])
            rows.append(torch.where(cnt[:, None] > 0, sel, torch.zeros_like(sel)) + n0)
            empty.append(cnt == 0)
        n0, m0 = n0 + n, m0 + m
    return torch.cat(rows), torch.cat(empty)


def eager_group(xyz, feats, new_xyz, rows, empty):
    g_xyz = (xyz[rows].permute(0, 2, 1) - new_xyz[:, :, None]).masked_fill(empty[:, None, None], 0)
    g_f = feats[rows].permute(0, 2, 1).masked_fill(empty[:, None, None], 0)
    return torch.cat([g_xyz, g_f], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet2_stack_bench.log"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from pcdet_amd.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm, pointnet2_utils as pu
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)

    def cnt_t(c):
        return torch.tensor(c, dtype=torch.int32, device=dev)

    pts_np = make_frames()
    raw, raw_f = torch.from_numpy(pts_np[:, :3].copy()).to(dev), torch.from_numpy(pts_np[:, 3:4].copy()).to(dev)
    raw_cnt = [POINTS] * BATCH
    lines = []

    def row(name, te, tf, spread, note=""):
        lines.append("%-64s %11s %11.1f %8s %7.1f%%  %s" % (name, "-" if te is None else "%.1f" % te, tf,
                                                             "-" if te is None else "%.1fx" % (te / tf), 100 * spread, note))

    g_raw_cnt = cnt_t(raw_cnt)
    t, s = timed_one(lambda: pu.stack_farthest_point_sample(raw, g_raw_cnt, KEYPOINTS), args.iters)
    row("stack FPS 4 x 16384 -> 2048", None, t, s, "%.3f us/round" % (t / (KEYPOINTS - 1)))
    kp_idx = pu.stack_farthest_point_sample(raw, cnt_t(raw_cnt), KEYPOINTS).long()
    kp = raw[kp_idx].contiguous()
    kp_cnt = [KEYPOINTS] * BATCH

    vox_np, vox_cnt = conv3_centres(pts_np)
    vox = torch.from_numpy(vox_np).to(dev)
    vox_f = torch.randn(vox.shape[0], 64, device=dev)
    grid = torch.from_numpy(roi_grid(kp.cpu().numpy(), rng)).to(dev)
    grid_cnt = [ROIS * GRID ** 3] * BATCH
    kp_f = torch.randn(kp.shape[0], 128, device=dev)

    def query_group(name, xyz, n_cnt, feats, new_xyz, m_cnt, radius, nsample, backward=False):
        g_n, g_m = cnt_t(n_cnt), cnt_t(m_cnt)
        grouper = pu.QueryAndGroup(radius, nsample)
        rows_e, empty_e = eager_query(xyz, n_cnt, new_xyz, m_cnt, radius, nsample)
        idx_f, empty_f = pu.ball_query(radius, nsample, xyz, g_n, new_xyz, g_m)
        starts = torch.repeat_interleave(torch.cumsum(g_n, 0) - g_n, g_m.long())
        same = float(((idx_f.long() + starts[:, None]) * (~empty_f)[:, None] == rows_e * (~empty_e)[:, None]).all(dim=1)
                     .float().mean())
        te, tf, s = timed_pair(lambda: eager_group(xyz, feats, new_xyz, *eager_query(xyz, n_cnt, new_xyz, m_cnt, radius, nsample)),
                               lambda: grouper(xyz, g_n, new_xyz, g_m, feats), args.iters)
        row(name + " r %.1f ns %d" % (radius, nsample), te, tf, s, "%.4f of the index rows equal" % same)
        if backward:
            go = torch.randn(new_xyz.shape[0], feats.shape[1], nsample, device=dev)
            fl = feats.detach().clone().requires_grad_(True)
            out = pu.grouping_operation(fl, g_n, idx_f, g_m)

            rows_f = (idx_f.long() + starts[:, None]).reshape(-1)

            def eager_bwd():
                return torch.zeros_like(feats).index_add_(0, rows_f, go.permute(0, 2, 1).reshape(-1, feats.shape[1]))

            te, tf, s = timed_pair(eager_bwd, lambda: torch.autograd.grad(out, fl, go, retain_graph=True), args.iters)
            err = float((torch.autograd.grad(out, fl, go, retain_graph=True)[0] - eager_bwd()).abs().max())
            row(name + " r %.1f grouping backward" % radius, te, tf, s, "max |fused - index_add_| %.2e" % err)

    for radius in (0.4, 0.8):
        query_group("keypoints <- raw points (C 1)", raw, raw_cnt, raw_f, kp, kp_cnt, radius, 16)
    for radius, ns in ((1.2, 16), (2.4, 32)):
        query_group("keypoints <- x_conv3 centres (C 64)", vox, vox_cnt, vox_f, kp, kp_cnt, radius, ns)
    for radius in (0.8, 1.6):
        query_group("RoI grid 4 x 27648 <- keypoints (C 128)", kp, kp_cnt, kp_f, grid, grid_cnt, radius, 16, backward=True)

    fp = pm.StackPointnetFPModule(mlp=[128 + 1, 128, 128]).to(dev).eval()
    g_raw, g_kp = cnt_t(raw_cnt), cnt_t(kp_cnt)

    def eager_fp():
        out, n0, m0 = [], 0, 0
        for n, m in zip(raw_cnt, kp_cnt):
            d = torch.cat([torch.cdist(raw[q0:min(q0 + 4096, n0 + n)], kp[m0:m0 + m], compute_mode=EXACT)
                           for q0 in range(n0, n0 + n, 4096)])
            dist, idx = torch.topk(d, 3, dim=1, largest=False)
            recip = 1.0 / (dist + 1e-8)
            w = recip / recip.sum(dim=1, keepdim=True)
            out.append((kp_f[idx + m0] * w[:, :, None]).sum(dim=1))
            n0, m0 = n0 + n, m0 + m
        x = torch.cat([torch.cat(out), raw_f], dim=1)
        return fp.mlp(x.permute(1, 0)[None, :, :, None])

    with torch.no_grad():
        te, tf, s = timed_pair(eager_fp, lambda: fp(raw, g_raw, kp, g_kp, raw_f, kp_f), args.iters)
        err = float((eager_fp().squeeze(0).squeeze(-1).permute(1, 0) - fp(raw, g_raw, kp, g_kp, raw_f, kp_f)).abs().max())
    row("StackPointnetFPModule keypoints -> raw (C 128)", te, tf, s, "max |fused - eager| %.2e" % err)

    head = "%-64s %11s %11s %8s %8s  %s" % ("stacked point ops, batch 4 (us per call)", "eager", "fused", "eager/f", "spread", "")
    text = "\n".join([head] + lines + [
        "Median of 5 alternating windows of %d eager / %d fused calls after 2 warm-up calls of each; spread = largest "
        "|window / median - 1| of either path.  %s" % (args.iters, 4 * args.iters, torch.cuda.get_device_name(0))])
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
