"""Part-A2: the RoI-aware pooling of PartA2FCHead as the per-frame composition (RoIAwarePool3d twice per frame, dense
grids, nonzero, gather: kernels of include/spx.h §12 only) against the fused sparse op (§30), and the whole PartA2Net.

  python tools/part_a2_bench.py [--iters N] [--skip-detector]
  python tools/part_a2_bench.py --fc-repeat      (profiles/part_a2_fc_repeat.log)

Batch 4, wall-clock per call with the host work included (synchronised at the window ends), median of 5 windows with
their spread (min .. max).  Rows: the pooling alone, forward and forward + backward, at 4 x 128 RoIs over 4 x 16384
points and at 4 x 100 RoIs over 4 x 40000 points, POOL_SIZE 12, 16 channels; the PartA2Net training step and the eval
forward with post-processing on the synthetic KITTI batch, FUSED off -> on -> static.  Also prints the error of the
pooled part averages against a float64 sum for both paths (the max pool selects values: no rounding)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/PartA2.yaml")
DEV = torch.device("cuda:0")


def windows(fn, iters, n_windows=5):
    """median, min, max over n_windows of the mean wall-clock milliseconds per call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return float(np.median(out)), min(out), max(out)


def scene(batch, m, n_rois, seed=0):
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    pts, rois = [], []
    for i in range(batch):
        f = syn.make_frame(2, i)
        p = f["points"][:, :3]
        p = p[rng.choice(p.shape[0], m, replace=p.shape[0] < m)]
        pts.append(np.concatenate([np.full((m, 1), i, np.float32), p], 1))
        gt = f["gt_boxes"][:, :7]
        base = gt[rng.integers(0, gt.shape[0], n_rois)].astype(np.float64)
        base[:, 0:3] += rng.normal(scale=0.3, size=(n_rois, 3))
        base[:, 3:6] *= rng.uniform(0.9, 1.3, size=(n_rois, 3))
        rois.append(base.astype(np.float32))
    pts = np.concatenate(pts).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    score = rng.uniform(0, 1, pts.shape[0]).astype(np.float32)
    return dict(batch_size=batch, rois=t(np.stack(rois)), point_coords=t(pts),
                point_features=t(rng.normal(size=(pts.shape[0], 16)).astype(np.float32)).requires_grad_(True),
                point_part_offset=t(rng.uniform(0, 1, (pts.shape[0], 3)).astype(np.float32)).requires_grad_(True),
                point_cls_scores=t(score))


def pool_head(m, **over):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.models.roi_heads import PartA2FCHead
    cfg = cfg_from_yaml_file(YAML, AttrDict()).MODEL.ROI_HEAD
    cfg.SHARED_FC = [8]                                     # the FC layers are not timed here
    cfg.ROI_AWARE_POOL.MAX_FRAME_POINTS = m
    for k, v in over.items():
        cfg.ROI_AWARE_POOL[k] = v
    return PartA2FCHead(input_channels=16, model_cfg=cfg, num_class=1).to(DEV).train()


def pooling_rows(iters, rows):
    for batch, n_rois, m in ((4, 128, 16384), (4, 100, 40000)):
        sc = scene(batch, m, n_rois)
        res = {}
        for name, over in (("composition", dict(FUSED=False)), ("fused", dict(FUSED=True))):
            head = pool_head(m, **over)
            fn = head.sparse_pool_fused if head.fused else head.sparse_pool_composed
            targets = dict(rcnn_cls_labels=torch.zeros(batch, n_rois, device=DEV),
                           reg_valid_mask=torch.ones(batch, n_rois, dtype=torch.int64, device=DEV))

            def fwd():
                with torch.no_grad():
                    return fn(dict(sc), dict(targets))

            def fwd_bwd():
                part, rpn, _, _ = fn(dict(sc), dict(targets))
                torch.autograd.grad(part.sum() + rpn.sum(), [sc["point_part_offset"], sc["point_features"]])

            res[name] = (fwd(), windows(fwd, iters), windows(fwd_bwd, iters))
        same = all(torch.equal(a, b) for a, b in zip(res["composition"][0][:3], res["fused"][0][:3]))
        shape = "%d x %d RoIs, %d x %d points, %d live rows, rows equal: %s" % (
            batch, n_rois, batch, m, res["fused"][0][0].shape[0], same)
        for k, what in ((1, "forward"), (2, "forward + backward")):
            a, b = res["composition"][k], res["fused"][k]
            rows.append("pool %-18s %s" % (what, shape))
            rows.append("    composition %8.3f ms (%.3f .. %.3f)   fused %8.3f ms (%.3f .. %.3f)   x%.2f%s"
                        % (a + b + (a[0] / b[0], "" if b[0] <= a[0] else "   LOSES")))
        if m == 16384:
            rows.append(accuracy(sc, res))


def accuracy(sc, res):
    """the pooled part averages of both paths against float64 sums over the same point lists"""
    from spx import ops
    head = pool_head(16384, FUSED=False)
    part = head.part_features(sc).detach()
    part_c, _, coords, _ = res["composition"][0]
    part_f = res["fused"][0][0]
    V = 12 ** 3
    n_per = sc["rois"].shape[1]
    ref = torch.zeros((sc["rois"].shape[0] * n_per * V, 4), dtype=torch.float64, device=DEV)
    cnt = torch.zeros((ref.shape[0],), dtype=torch.float64, device=DEV)
    frame = sc["point_coords"][:, 0]
    for b in range(sc["batch_size"]):
        mask = frame == b
        _, _, pt_cell, _ = ops.roiaware_pool3d_fwd(sc["rois"][b, :, :7].contiguous(), sc["point_coords"][mask, 1:4],
                                                   part[mask], (12, 12, 12), 128, 1)
        r, p = torch.nonzero(pt_cell >= 0, as_tuple=True)
        cell = (b * n_per + r) * V + pt_cell[r, p].long()
        ref.index_add_(0, cell, part[mask][p].double())
        cnt.index_add_(0, cell, torch.ones_like(cell, dtype=torch.float64))
    c = coords.long()
    want = (ref / cnt.clamp(min=1).unsqueeze(1))[((c[:, 0] * 12 + c[:, 1]) * 12 + c[:, 2]) * 12 + c[:, 3]]
    e_c = float((part_c.double() - want).abs().max())
    e_f = float((part_f.double() - want).abs().max())
    return ("accuracy, part averages vs float64 (values in [0, 1]): composition max|err| %.3e, fused max|err| %.3e; "
            "rpn rows are selected values (max pool): bitwise equal = %s" % (e_c, e_f, torch.equal(res["composition"][0][1],
                                                                                                   res["fused"][0][1])))


def detector_rows(iters, rows):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=2)
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, ds).to(DEV)
    batch = ds.collate_batch([ds[i] for i in range(4)])
    batch = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    head = model.roi_head
    res = {"train": {}, "eval": {}}
    for name, fused, static in (("off", False, None), ("on", True, None), ("static", True, 196608)):
        head.fused, head.static_rows = fused, static

        def train_step():
            model.train()
            opt.zero_grad(set_to_none=True)
            ret, _, _ = model(dict(batch))
            ret["loss"].backward()
            opt.step()

        def eval_step():
            model.eval()
            with torch.no_grad():
                model(dict(batch))

        res["train"][name] = windows(train_step, iters)
        res["eval"][name] = windows(eval_step, iters)
    from spx import _lib, ops
    try:
        ops.check_status(DEV)
    except _lib.SpxError as e:
        rows.append("static capacity 196608 rows overflowed (%s): the static rows below are NOT VALID" % e)
    for mode, what in (("train", "PartA2Net training step"), ("eval", "PartA2Net eval forward + post-processing")):
        a = res[mode]["off"]
        rows.append("%s, synthetic KITTI batch 4" % what)
        for name in ("off", "on", "static"):
            b = res[mode][name]
            rows.append("    FUSED %-7s %9.3f ms (%.3f .. %.3f)   x%.3f%s"
                        % ((name,) + b + (a[0] / b[0], "" if b[0] <= a[0] * 1.0 or name == "off" else "   LOSES")))


def fc_repeat():
    """Are the head's dense layers reproducible from one call to the next?  One small head (POOL_SIZE 4, 32 features), the
    composition path, the same batch four times: per stage, whether every run equals the first bit for bit and the largest
    difference.  The sparse conv branches and the dense FC input come from this library; the FC layers go through torch."""
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.models.roi_heads import PartA2FCHead
    cfg = cfg_from_yaml_file(YAML, AttrDict()).MODEL.ROI_HEAD
    cfg.SHARED_FC, cfg.CLS_FC, cfg.REG_FC, cfg.DP_RATIO = [16, 16], [16, 16], [16, 16], 0.0
    cfg.ROI_AWARE_POOL.POOL_SIZE, cfg.ROI_AWARE_POOL.NUM_FEATURES, cfg.ROI_AWARE_POOL.FUSED = 4, 32, False
    torch.manual_seed(3)
    head = PartA2FCHead(input_channels=16, model_cfg=cfg, num_class=1).to(DEV).eval()
    sc = scene(2, 4096, 16)
    runs = []
    for _ in range(4):
        seen = {}
        hooks = [head.conv_part.register_forward_hook(lambda m, i, o: seen.__setitem__("conv_part", o.features.clone())),
                 head.conv_rpn.register_forward_hook(lambda m, i, o: seen.__setitem__("conv_rpn", o.features.clone())),
                 head.shared_fc_layer.register_forward_pre_hook(lambda m, i: seen.__setitem__("dense FC input", i[0].clone())),
                 head.shared_fc_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("shared_fc_layer", o.clone()))]
        with torch.no_grad():
            out = head({k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in sc.items()})
        for h in hooks:
            h.remove()
        seen["batch_cls_preds"], seen["batch_box_preds"] = out["batch_cls_preds"].clone(), out["batch_box_preds"].clone()
        runs.append(seen)
    print("# tools/part_a2_bench.py --fc-repeat, one MI355X: PartA2FCHead (composition, eval), the same batch four times")
    for k in runs[0]:
        same = all(torch.equal(runs[0][k], r[k]) for r in runs[1:])
        diff = max(float((runs[0][k] - r[k]).abs().max()) for r in runs[1:])
        print("%-18s runs bit-equal: %-5s max |difference| %.3e   (max |value| %.3e)" % (k, same, diff, float(runs[0][k].abs().max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fc-repeat", action="store_true", help="only: run-to-run reproducibility of the head's stages")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--skip-detector", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build(verbose=False)
    if args.fc_repeat:
        return fc_repeat()
    rows = []
    pooling_rows(args.iters, rows)
    if args.skip_detector:
        rows.append("PartA2Net training step / eval forward: NOT MEASURED (--skip-detector)")
    else:
        detector_rows(max(args.iters // 2, 3), rows)
    print("# tools/part_a2_bench.py --iters %d, one MI355X (wall-clock ms per call, host work included; median of 5 "
          "windows, min .. max)" % args.iters)
    for r in rows:
        print(r)


if __name__ == "__main__":
    main()
