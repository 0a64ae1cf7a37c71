"""Times PV-RCNN's set-abstraction pooling in eval mode: StackSAModuleMSG with fused = False (the torch composition: two
groupings, Conv2d + BatchNorm2d + ReLU twice over (1, C, M, S) tensors, max) against fused = True (one GEMM over the
source rows + spx.ops.sa_mlp2_max, csrc/sa_mlp.hip).  Both paths run the same ball query, which is inside the timings.

  python tools/pv_rcnn_bench.py [--iters N] [--skip-model]

Rows:
  * RoI-grid pooling: batch 4, 4 x 2048 keypoints with 128 features, 100 or 128 car-sized RoIs per frame with a
    6 x 6 x 6 grid each (M = 86 400 / 110 592 queries), 128 -> 64 -> 64, radii 0.8 / 1.6, 16 samples; and the same with a
    tenth of the queries moved into one dense cluster of keypoints (every ball full).
  * each VoxelSetAbstraction source at tools/cfgs/kitti_models/pv_rcnn.yaml's shapes, on the first stage's own outputs
    for batch 4 synthetic KITTI-sized frames.
  * the whole PVRCNN eval forward with post-processing, PFE.FUSED and ROI_GRID_POOL.FUSED off against on; one training
    step (forward + backward), composition only, for the record.
The two paths are compared on the timed inputs before timing.  Times are HIP-event times around windows of back-to-back
calls, the median of five alternating windows, host work included; spread is the worst window's relative distance from
its median."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCH, GRID, KEYPOINTS, C_IN = 4, 6, 2048, 128
CAR = np.array([3.9, 1.6, 1.56])
YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/pv_rcnn.yaml")


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters      # microseconds


def timed(fns, reps=5):
    """fns: list of (callable, iterations per window) -> (median us per call, ...), worst relative spread."""
    for fn, _ in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, (fn, n) in zip(times, fns):
            t.append(window(fn, n))
    med = [float(np.median(t)) for t in times]
    spread = max(max(abs(v / m - 1) for v in t) for t, m in zip(times, med))
    return med, spread


def compare_and_time(tag, run, set_fused, iters, m, n_src):
    """run() -> (M, C) features; set_fused(flag) switches the path."""
    with torch.no_grad():
        set_fused(False)
        a = run()
        set_fused(True)
        b = run()
    err = float((a - b).abs().max())
    assert err <= 1e-4 * float(a.abs().max()), err
    del a, b

    def call(flag):
        set_fused(flag)
        with torch.no_grad():
            return run()

    (te, tf), spread = timed([(lambda: call(False), iters), (lambda: call(True), 4 * iters)])
    set_fused(False)
    print("%-30s %7d %7d | %10.1f %10.1f %7.2fx %6.1f%%" % (tag, m, n_src, te, tf, te / tf, 100 * spread))


def roi_grid_scene(n_rois, dev, cluster, seed=0):
    """-> xyz (B * K, 3) keypoints, features (B * K, C_IN), new_xyz (B * R * 216, 3) and both counts."""
    r = np.random.default_rng(seed)
    centres = np.stack([r.uniform(3, 67, (BATCH, n_rois)), r.uniform(-37, 37, (BATCH, n_rois)),
                        np.full((BATCH, n_rois), -1.0)], -1)                                  # (B, R, 3)
    near = KEYPOINTS * 3 // 4                                                                 # keypoints in and around the RoIs
    pick = r.integers(0, n_rois, (BATCH, near))
    kp_near = np.take_along_axis(centres, pick[..., None], 1) + r.uniform(-0.75, 0.75, (BATCH, near, 3)) * CAR
    kp_far = np.stack([r.uniform(0, 70.4, (BATCH, KEYPOINTS - near)), r.uniform(-40, 40, (BATCH, KEYPOINTS - near)),
                       r.normal(-1.7, 0.05, (BATCH, KEYPOINTS - near))], -1)
    kp = np.concatenate([kp_near, kp_far], 1)
    g = (np.stack(np.meshgrid(*[np.arange(GRID)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5) / GRID - 0.5
    new = (centres[:, :, None, :] + g * CAR).reshape(BATCH, -1, 3)                            # (B, R * 216, 3)
    if cluster:                                  # 200 keypoints of each frame within 0.5 m, a tenth of the queries among them
        spot = np.array([35.0, 0.0, -1.0])
        kp[:, :200] = spot + r.uniform(-0.25, 0.25, (BATCH, 200, 3))
        new[:, ::10] = spot + r.uniform(-0.25, 0.25, new[:, ::10].shape)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.reshape(-1, 3)).astype(np.float32)).to(dev)      # noqa: E731
    feats = torch.randn(BATCH * KEYPOINTS, C_IN, generator=torch.Generator().manual_seed(1)).to(dev)
    cnt = lambda n: torch.full((BATCH,), n, dtype=torch.int32, device=dev)      # noqa: E731
    return dict(xyz=t(kp), xyz_batch_cnt=cnt(KEYPOINTS), new_xyz=t(new), new_xyz_batch_cnt=cnt(new.shape[1]), features=feats)


def bench_roi_grid(iters, dev):
    from pcdet_amd.ops.pointnet2.pointnet2_stack.pointnet2_modules import StackSAModuleMSG
    torch.manual_seed(0)
    mod = StackSAModuleMSG(radii=[0.8, 1.6], nsamples=[16, 16], mlps=[[C_IN, 64, 64], [C_IN, 64, 64]]).to(dev).eval()
    for n_rois in (100, 128):
        for cluster in (False, True):
            s = roi_grid_scene(n_rois, dev, cluster)
            tag = "roi grid, %d rois%s" % (n_rois, ", 1/10 in a cluster" if cluster else "")
            compare_and_time(tag, lambda: mod(**s)[1], lambda flag: setattr(mod, "fused", flag), iters,
                             s["new_xyz"].shape[0], s["xyz"].shape[0])
            del s
            torch.cuda.empty_cache()


def build_model(dev):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=2)
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds).to(dev)
    batch = ds.collate_batch([ds[i] for i in range(BATCH)])
    batch = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    return model, batch


def bench_vsa_sources(model, batch, iters):
    pfe = model.pfe
    model.eval()
    with torch.no_grad():
        b = dict(batch)
        for module in model.module_list:
            if module is pfe:
                break
            b = module(b)
        keypoints = pfe.get_sampled_points(b)
    new_xyz = keypoints[:, 1:4].contiguous()
    new_cnt = torch.full((BATCH,), pfe.model_cfg.NUM_KEYPOINTS, dtype=torch.int32, device=new_xyz.device)
    sources = [("raw_points", pfe.SA_rawpoints, b["points"][:, 1:4].contiguous(), b["points"][:, 4:].contiguous(),
                b["points"][:, 0])]
    for k, name in enumerate(pfe.SA_layer_names):
        sp = b["multi_scale_3d_features"][name]
        sources.append((name, pfe.SA_layers[k], pfe.voxel_centers(sp.indices[:, 1:4], pfe.downsample_times_map[name]),
                        sp.features.contiguous(), sp.indices[:, 0]))
    for name, layer, xyz, feats, bs in sources:
        run = lambda: pfe.aggregate_keypoint_features_from_one_source(      # noqa: E731
            batch_size=BATCH, aggregate_func=layer, xyz=xyz, xyz_features=feats, xyz_bs_idxs=bs, new_xyz=new_xyz,
            new_xyz_batch_cnt=new_cnt)
        compare_and_time("vsa %s" % name, run, lambda flag, layer=layer: setattr(layer, "fused", flag), iters,
                         new_xyz.shape[0], xyz.shape[0])


def bench_model(model, batch, iters):
    layers = model.pfe.sa_modules() + [model.roi_head.roi_grid_pool_layer]

    def set_fused(flag):
        for layer in layers:
            layer.fused = flag

    def eval_step(flag):
        set_fused(flag)
        with torch.no_grad():
            return model(dict(batch))[0]

    def train_step():
        model.zero_grad(set_to_none=True)
        ret, _tb, _disp = model(dict(batch))
        ret["loss"].backward()
        return ret["loss"].detach()

    model.eval()
    (te, tf), spread = timed([(lambda: eval_step(False), iters), (lambda: eval_step(True), iters)])
    print("%-30s | %10.1f %10.1f %7.3fx %6.1f%%" % ("eval forward + post-processing", te, tf, te / tf, 100 * spread))
    set_fused(False)
    model.train()
    loss = float(train_step())
    assert np.isfinite(loss), loss
    (tt,), spread = timed([(train_step, iters)])
    print("%-30s | %10.1f %10s %8s %6.1f%%   (composition only; loss %.4f)" % ("training step", tt, "-", "-", 100 * spread,
                                                                                loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("StackSAModuleMSG in eval mode, batch %d, ball query included (microseconds per call)" % BATCH)
    print("%-30s %7s %7s | %10s %10s %8s %7s" % ("scene", "M", "n_src", "composed", "fused", "speedup", "spread"))
    bench_roi_grid(args.iters, dev)
    if args.skip_model:
        return
    model, batch = build_model(dev)
    bench_vsa_sources(model, batch, args.iters)
    print("PVRCNN (pv_rcnn.yaml), batch %d KITTI-sized frames (microseconds per call)" % BATCH)
    print("%-30s | %10s %10s %8s %7s" % ("", "FUSED off", "FUSED on", "speedup", "spread"))
    bench_model(model, batch, args.iters)


if __name__ == "__main__":
    main()
