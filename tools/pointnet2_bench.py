"""Times the pointnet2_batch ops (include/spx.h §11) at the fork's shapes with HIP events; prints one table.

  python tools/pointnet2_bench.py [--iters N]

FPS is reported per round and against the VALU-issue floor of the register-resident kernel: the round loop of
k_fps<0, 16> is VALU_PER_ROUND wave-instructions (counted in this build's gfx950 ISA: 221 in the 16-point scan, 56 in
the wave / workgroup reduction); 16 waves share a CU's 4 SIMDs and a wave issues one VALU instruction per 2 cycles, so
one round cannot take less than 4 * VALU_PER_ROUND * 2 cycles.  Ball query is reported as point pairs tested per
second (an upper bound: the scan stops early once every query of a workgroup is full), grouping as a fraction of HBM
bandwidth (bytes that must move: output written, indices read, features read once)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

VALU_PER_ROUND = 221 + 56
CLOCK_HZ = 2.4e9
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


def frames(batch, n, seed=0):
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    out = []
    for i in range(batch):
        pts = syn.make_frame(1, i)["points"][:, :3]
        out.append(pts[rng.choice(pts.shape[0], n, replace=pts.shape[0] < n)])
    return torch.from_numpy(np.ascontiguousarray(np.stack(out).astype(np.float32))).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from pcdet_amd.ops.pointnet2.pointnet2_batch import pointnet2_utils as pu

    rows = []
    floor_us = 4 * VALU_PER_ROUND * 2 / CLOCK_HZ * 1e6

    xyz = frames(16, 16384)
    t = timed(lambda: pu.furthest_point_sample(xyz, 4096), args.iters)
    rows.append(("KITTI d-FPS 16x16384->4096", t, "%.3f us/round, VALU floor %.3f us/round (%.0f%%)"
                 % (t / 4095, floor_us, 100 * floor_us / (t / 4095))))
    idx = pu.furthest_point_sample(xyz, 4096)
    new_xyz = pu.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    w = torch.rand(16, 4096, device=xyz.device)
    t = timed(lambda: pu.furthest_point_sample_weights(new_xyz, w, 512), args.iters)
    rows.append(("KITTI s-FPS 16x4096->512", t, "%.3f us/round" % (t / 512)))
    for r_in, r_out in ((0.0, 0.2), (0.2, 0.4), (0.4, 0.8)):
        t = timed(lambda: pu.ball_query_dilated(r_in, r_out, 32, xyz, new_xyz), args.iters)
        rows.append(("KITTI ball query %.1f-%.1f M=4096 N=16384 ns=32" % (r_in, r_out), t,
                     "<= %.1f G pairs/s" % (16 * 4096 * 16384 / (t * 1e-6) / 1e9)))
    _, bidx = pu.ball_query_dilated(0.4, 0.8, 32, xyz, new_xyz)
    feats = torch.randn(16, 4, 16384, device=xyz.device, requires_grad=True)
    t = timed(lambda: pu.grouping_operation(feats, bidx), args.iters)
    nbytes = 16 * 4 * 4096 * 32 * 4 + 16 * 4096 * 32 * 4 + 16 * 4 * 16384 * 4
    rows.append(("KITTI grouping -> (16,4,4096,32)", t, "%.1f%% of HBM" % (100 * nbytes / (t * 1e-6) / HBM_BPS)))
    out = pu.grouping_operation(feats, bidx)
    go = torch.randn_like(out)
    t = timed(lambda: torch.autograd.grad(out, feats, go, retain_graph=True), args.iters)
    rows.append(("KITTI grouping backward (deterministic)", t, "%.1f%% of HBM (same bytes)"
                 % (100 * nbytes / (t * 1e-6) / HBM_BPS)))
    del xyz, new_xyz, feats, out, go

    rng = np.random.default_rng(1)
    wxyz = torch.from_numpy((rng.uniform(-75, 75, size=(8, 163840, 3)) * np.array([1, 1, 0.04])).astype(np.float32)).cuda()
    t = timed(lambda: pu.furthest_point_sample(wxyz, 16384), 1)
    rows.append(("Waymo d-FPS 8x163840->16384 (general path)", t, "%.3f us/round" % (t / 16383)))

    print("%-50s %14s  %s" % ("op", "time (us)", "rate"))
    for name, t, rate in rows:
        print("%-50s %14.1f  %s" % (name, t, rate))


if __name__ == "__main__":
    main()
