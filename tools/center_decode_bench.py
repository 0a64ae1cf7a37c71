"""Times the centre head's box decoding: the eager generate_predicted_boxes (the reference's composition: sigmoid, exp,
two topk, six gathers, then per frame a mask, class-agnostic NMS and a cat) against the fused path (POST_PROCESSING.FUSED:
spx.ops.center_decode + spx.ops.point_post_process, csrc/center_decode.hip and csrc/post_process.hip, one host read of the
counts) and against generate_predicted_boxes_static (the same without the read); and CenterPoint's eval forward,
model(batch), against a GraphedCenterPoint replay.  Prints two tables.

  python tools/center_decode_bench.py [--iters N] [--skip-model]

Head rows: both yamls' shapes (KITTI 3 x 200 x 176, Waymo 3 x 188 x 188), batch 4, K = 500, synthetic head outputs whose
heatmap prior is lifted so that about 50 / about 400 of a frame's 500 candidates pass SCORE_THRESH.  Model rows: the two
centerpoint yamls on synthetic batches of 4 frames, the heatmap bias lifted towards the same targets; an untrained
network's heatmap is constant over the empty part of the map, so the lift moves whole plateaus over the threshold and
the `kept` column, not the target, says what the NMS saw.  The paths are compared on the timed inputs before timing
(head table: same counts and labels, boxes within 1e-5; model table: same counts to within two boxes, because the
vendor's dense convolutions differ in the last bits from call to call).  A replay runs every sparse kernel at the
runner's row capacity (min(points, batch x MAX_NUMBER_OF_VOXELS)), the eager forward at the live row counts.  Times are HIP-event times around windows of back-to-back
calls, the median of five alternating windows, host work and host reads included."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

YAMLS = {"kitti": ("tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/centerpoint.yaml", 2, (200, 176)),
         "waymo": ("tsm-det-pointcloud-_amd/tools/cfgs/waymo_models/centerpoint.yaml", 3, (188, 188))}
BATCH = 4
SIZES = np.log(np.array([(4.0, 1.8, 1.6), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73)], np.float32))


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters      # microseconds


def timed(fns, iters, reps=5):
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


def load_cfg(name):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    return cfg_from_yaml_file(os.path.join(ROOT, YAMLS[name][0]), AttrDict())


def lift_for(hm, passing, score_thresh):
    """The shift of the logits after which `passing` values per frame (the mean over frames) exceed the threshold."""
    kth = hm.flatten(1).topk(passing, dim=1)[0][:, -1].mean()
    return float(np.log(score_thresh / (1 - score_thresh)) - kth) + 1e-3


def synthetic_preds(shape, seed, dev):
    h, w = shape
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, 3, (BATCH, 1, h, w), generator=g)
    dim = torch.from_numpy(SIZES)[cls[:, 0]].permute(0, 3, 1, 2) + 0.1 * torch.randn(BATCH, 3, h, w, generator=g)
    pd = {"hm": -2.19 + 0.5 * torch.randn(BATCH, 3, h, w, generator=g), "center": torch.rand(BATCH, 2, h, w, generator=g),
          "center_z": -1.0 + 0.3 * torch.randn(BATCH, 1, h, w, generator=g), "dim": dim,
          "rot": torch.randn(BATCH, 2, h, w, generator=g)}
    return {k: v.float().contiguous().to(dev) for k, v in pd.items()}


def same(a, b):
    for x, y in zip(a, b):
        assert x["pred_boxes"].shape == y["pred_boxes"].shape, (x["pred_boxes"].shape, y["pred_boxes"].shape)
        assert torch.equal(x["pred_labels"], y["pred_labels"])
        assert float((x["pred_boxes"] - y["pred_boxes"]).abs().max()) <= 1e-5 if x["pred_boxes"].numel() else True


def bench_head(name, iters, dev):
    from pcdet_amd.models.dense_heads import CenterHead
    from pcdet_amd.datasets import SyntheticDataset
    cfg = load_cfg(name)
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, False, cfg_id=YAMLS[name][1])
    head = CenterHead(model_cfg=cfg.MODEL.DENSE_HEAD, input_channels=64, num_class=3, class_names=list(cfg.CLASS_NAMES),
                      grid_size=ds.grid_size, point_cloud_range=ds.point_cloud_range, voxel_size=ds.voxel_size,
                      predict_boxes_when_training=False).to(dev).eval()
    post = head.model_cfg.POST_PROCESSING
    base = synthetic_preds(YAMLS[name][2], 5, dev)
    for passing in (50, 400):
        pd = dict(base, hm=base["hm"] + lift_for(base["hm"], passing, post.SCORE_THRESH))

        def eager():
            post.FUSED = False
            return head.generate_predicted_boxes(BATCH, [pd])

        def fused():
            post.FUSED = True
            return head.generate_predicted_boxes(BATCH, [pd])

        def static():
            return head.generate_predicted_boxes_static(BATCH, [pd])

        with torch.no_grad():
            a, b = eager(), fused()
            same(a, b)
            kept = np.mean([d["pred_boxes"].shape[0] for d in b])
            (te, tf, ts), spread = timed([(eager, iters), (fused, 4 * iters), (static, 4 * iters)], iters)
        post.FUSED = False
        print("%-6s %8d %8.0f | %10.1f %10.1f %10.1f %7.1fx %6.1f%%"
              % (name, passing, kept, te, tf, ts, te / tf, 100 * spread))


def bench_model(name, iters, dev):
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    from pcdet_amd.models.inference import GraphedCenterPoint
    cfg = load_cfg(name)
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, False, cfg_id=YAMLS[name][1])
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, ds).to(dev).eval()
    batch = ds.collate_batch([ds[i] for i in range(BATCH)])
    batch = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    post = model.dense_head.model_cfg.POST_PROCESSING
    bias = model.dense_head.heads_list[0].hm[-1].bias
    with torch.no_grad():
        model(dict(batch))
        hm = model.dense_head.forward_ret_dict["pred_dicts"][0]["hm"]
        zero = bias.clone()
        runner = None
        for passing in (50, 400):
            bias.copy_(zero + lift_for(hm, passing, post.SCORE_THRESH))
            if runner is None:
                runner = GraphedCenterPoint(model, BATCH, batch["points"].shape[0], max_gt=batch["gt_boxes"].shape[1])

            def eager():
                post.FUSED = False
                return model(dict(batch))

            def fused():
                post.FUSED = True
                return model(dict(batch))

            def replay():
                runner(batch["points"], batch["gt_boxes"])
                return runner.pred_dicts()

            a, b, c = eager(), fused(), replay()
            # the vendor's dense convolutions differ in the last bits from call to call (tests/test_gpu_center_decode.py
            # holds the three paths bit-equal under cudnn.deterministic): here only the counts, to within a flipped box
            for x, y, z in zip(a[0], b[0], c[0]):
                n = [d["pred_boxes"].shape[0] for d in (x, y, z)]
                assert max(n) - min(n) <= 2, n
            assert runner.overflowed() == {}
            kept = np.mean([d["pred_boxes"].shape[0] for d in c[0]])
            (te, tf, tr), spread = timed([(eager, iters), (fused, iters), (replay, iters)], iters)
            post.FUSED = False
            print("%-6s %8d %8.0f | %10.1f %10.1f %10.1f %7.2fx %6.1f%%"
                  % (name, passing, kept, te, tf, tr, te / tr, 100 * spread))
        bias.copy_(zero)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("CenterHead.generate_predicted_boxes, batch %d, K = 500 (microseconds per call)" % BATCH)
    print("%-6s %8s %8s | %10s %10s %10s %8s %7s" % ("shape", "passing", "kept", "eager", "fused", "static",
                                                     "speedup", "spread"))
    for name in YAMLS:
        bench_head(name, args.iters, dev)
    if args.skip_model:
        return
    print("CenterPoint eval forward, batch %d (microseconds per call)" % BATCH)
    print("%-6s %8s %8s | %10s %10s %10s %8s %7s" % ("yaml", "target", "kept", "model", "model+FUSED", "replay",
                                                     "speedup", "spread"))
    for name in YAMLS:
        bench_model(name, args.iters, dev)


if __name__ == "__main__":
    main()
