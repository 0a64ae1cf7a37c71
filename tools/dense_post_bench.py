"""Eager versus fused post-processing of dense predictions (spx.ops.dense_post_process, include/spx.h §29) on one GPU.

Rows, all at batch 4:
  * Detector3DTemplate.post_processing over an anchor head's outputs -- SECOND (200 x 176 x 6 = 211 200 anchors, three
    per-class thresholds, 4096 / 500) and PointPillars (248 x 216 x 6 = 321 408 anchors, one threshold) -- with about 50
    and about 2 000 rows per frame over the threshold: the eager per-frame loop (FUSED absent), the fused path with its
    one host read (FUSED: True) and post_processing_static (no host read).
  * RoIHeadTemplate.proposal_layer over 211 200 anchors, 9000 / 512 and 1024 / 100, no threshold: the topk + per-frame
    NMS loop against NMS_CONFIG.FUSED.
  * whole model (SECOND, KITTI geometry, random init): a GraphedDetector replay followed by its eager post_process()
    against one GraphedAnchorDetector replay with pred_dicts().
The two paths of a row alternate in one process after warm-up; a figure is the median of --windows windows of --iters
calls, with the spread (min .. max).  The eager and fused results of every row are compared before anything is timed.
Writes profiles/dense_post_bench.log."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = torch.device("cuda:0")
RANGE = (0.0, -40.0, 70.4, 40.0)


def _window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def alternate(fns, iters, windows):
    """{name: [us per call of each window]}, the variants taking turns."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(_window(fn, iters))
    return t


def cell(v):
    return "%9.1f (%8.1f .. %8.1f)" % (statistics.median(v), min(v), max(v))


def head_outputs(b, n, num_class, over, seed):
    """Dense head outputs: car-sized boxes anywhere in the KITTI range, distinct logits of which `over` per frame sit
    above every threshold used here (sigmoid > 0.3) and the rest far below (sigmoid < 0.02)."""
    g = torch.Generator().manual_seed(seed)
    boxes = torch.empty(b, n, 7)
    boxes[..., 0] = torch.rand(b, n, generator=g) * (RANGE[2] - RANGE[0]) + RANGE[0]
    boxes[..., 1] = torch.rand(b, n, generator=g) * (RANGE[3] - RANGE[1]) + RANGE[1]
    boxes[..., 2] = -1.0
    boxes[..., 3:6] = torch.tensor([3.9, 1.6, 1.56]) * (0.8 + 0.4 * torch.rand(b, n, 3, generator=g))
    boxes[..., 6] = (torch.rand(b, n, generator=g) * 2 - 1) * np.pi
    total = b * n * num_class
    logits = torch.linspace(-12.0, -4.0, total)[torch.randperm(total, generator=g)].view(b, n, num_class)
    high = torch.linspace(-0.8, 3.0, b * over)[torch.randperm(b * over, generator=g)].view(b, over)
    for f in range(b):
        rows = torch.randperm(n, generator=g)[:over]
        logits[f, rows, torch.randint(0, num_class, (over,), generator=g)] = high[f]
    assert torch.sigmoid(logits.to(DEV)).unique().numel() == total, "scores tie: pick another seed"
    return boxes.to(DEV), logits.to(DEV)


def detector_stub(score_thresh, pre_max, post_max):
    """A Detector3DTemplate with just what post_processing reads."""
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.detectors.detector3d_template import Detector3DTemplate
    det = Detector3DTemplate.__new__(Detector3DTemplate)
    torch.nn.Module.__init__(det)
    det.num_class = 3
    det.model_cfg = AttrDict(POST_PROCESSING=dict(
        SCORE_THRESH=score_thresh, OUTPUT_RAW_SCORE=False, RECALL_THRESH_LIST=[0.3, 0.5, 0.7],
        NMS_CONFIG=dict(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu", NMS_THRESH=0.01, NMS_PRE_MAXSIZE=pre_max,
                        NMS_POST_MAXSIZE=post_max)))
    return det


def same_preds(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b)
                                    for k in ("pred_boxes", "pred_scores", "pred_labels"))


def post_rows(iters, windows, lines):
    lines += ["Detector3DTemplate.post_processing, batch 4; us per call, median of %d windows of %d calls (min .. max)"
              % (windows, iters), "",
              "%-34s %31s %31s %31s %8s %6s" % ("anchors / thresholds / over thr", "eager", "fused (one host read)",
                                                "static (no host read)", "eager/f", "kept")]
    losing = []
    for name, n, thresh in (("SECOND 211200 / 3 per class", 200 * 176 * 6, [0.3, 0.3, 0.3]),
                            ("PointPillars 321408 / agnostic", 248 * 216 * 6, 0.3)):
        for over in (50, 2000):
            det = detector_stub(thresh, 4096, 500)
            boxes, logits = head_outputs(4, n, 3, over, seed=over)
            bd = dict(batch_size=4, batch_box_preds=boxes, batch_cls_preds=logits, cls_preds_normalized=False)
            cfg = det.model_cfg.POST_PROCESSING

            def eager():
                cfg.pop("FUSED", None)
                return det.post_processing(dict(bd))

            def fused():
                cfg["FUSED"] = True
                return det.post_processing(dict(bd))

            def static():
                cfg["FUSED"] = True
                return det.post_processing_static(dict(bd))

            with torch.no_grad():
                want, got = eager()[0], fused()[0]
                assert same_preds(got, want), name
                kept = sum(p["pred_boxes"].shape[0] for p in got) / 4.0
                t = alternate({"eager": eager, "fused": fused, "static": static}, iters, windows)
            ratio = statistics.median(t["eager"]) / statistics.median(t["fused"])
            label = "%s / %d" % (name, over)
            lines.append("%-34s %s %s %s %7.2fx %6.1f" % (label, cell(t["eager"]), cell(t["fused"]), cell(t["static"]),
                                                        ratio, kept))
            if ratio <= 1.0:
                losing.append(label)
    return losing


def proposal_rows(iters, windows, lines):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads.roi_head_template import RoIHeadTemplate
    head = RoIHeadTemplate.__new__(RoIHeadTemplate)
    lines += ["", "RoIHeadTemplate.proposal_layer over 4 x 211200 anchors, no threshold, NMS_THRESH 0.8; us per call", "",
              "%-34s %31s %31s %8s" % ("pre / post", "topk + per-frame loop", "NMS_CONFIG.FUSED", "loop/f")]
    boxes, logits = head_outputs(4, 200 * 176 * 6, 3, 2000, seed=7)
    losing = []
    for pre, post in ((9000, 512), (1024, 100)):
        loop_cfg = AttrDict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=pre, NMS_POST_MAXSIZE=post,
                            NMS_THRESH=0.8)
        fused_cfg = AttrDict(dict(loop_cfg, FUSED=True))
        bd = dict(batch_size=4, batch_box_preds=boxes, batch_cls_preds=logits)
        want, got = head.proposal_layer(dict(bd), loop_cfg), head.proposal_layer(dict(bd), fused_cfg)
        assert all(torch.equal(want[k], got[k]) for k in ("rois", "roi_scores", "roi_labels")), (pre, post)
        t = alternate({"loop": lambda: head.proposal_layer(dict(bd), loop_cfg),
                       "fused": lambda: head.proposal_layer(dict(bd), fused_cfg)}, iters, windows)
        ratio = statistics.median(t["loop"]) / statistics.median(t["fused"])
        label = "%d / %d" % (pre, post)
        lines.append("%-34s %s %s %7.2fx" % (label, cell(t["loop"]), cell(t["fused"]), ratio))
        if ratio <= 1.0:
            losing.append("proposals " + label)
    return losing


def model_rows(iters, windows, lines):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset, synthetic
    from pcdet_amd.models import build_network
    from pcdet_amd.models.inference import GraphedAnchorDetector, GraphedDetector
    cfg = cfg_from_yaml_file(os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/second.yaml"), AttrDict())
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, training=False, cfg_id=2)
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, ds).to(DEV).eval()
    # A random-init class head puts every anchor within 0.15 of logit -4.6, thousands of them equal.  A forward hook adds a
    # fixed offset to its logits (in both runners): 2 000 anchors per frame are lifted on one class to scores of about
    # 0.12 .. 0.73, distinct, everything else is pushed far below the 0.1 threshold.
    pts = torch.from_numpy(synthetic.make_batch(2, 4)["points"]).to(DEV)
    with torch.no_grad():
        bd = {"points": pts, "batch_size": 4}
        for m in model.module_list:
            bd = m(bd)
    shape = tuple(bd["batch_cls_preds"].shape)
    g = torch.Generator().manual_seed(5)
    offset = torch.full(shape, -20.0)
    for f in range(shape[0]):
        rows = torch.randperm(shape[1], generator=g)[:2000]
        offset[f, rows, torch.randint(0, shape[2], (2000,), generator=g)] = \
            torch.linspace(2.6, 5.6, 2000)[torch.randperm(2000, generator=g)]
    offset = offset.to(DEV)

    def hook(_module, _inputs, out):
        out["batch_cls_preds"] = out["batch_cls_preds"] + offset
        return out

    model.dense_head.register_forward_hook(hook)
    cap = int(pts.shape[0] * 1.05) + 64
    plain, whole = GraphedDetector(model, 4, cap), GraphedAnchorDetector(model, 4, cap)

    def two_step():
        plain(pts)
        return plain.post_process()

    def one_replay():
        whole(pts)
        return whole.pred_dicts()

    a, b = two_step()[0], one_replay()[0]
    # two forward passes: the vendor's dense convolutions repeat to ~1e-7 only, so values are compared to 1e-5
    same = len(a) == len(b) and all(
        x["pred_boxes"].shape == y["pred_boxes"].shape and torch.equal(x["pred_labels"], y["pred_labels"])
        and bool(((x["pred_boxes"] - y["pred_boxes"]).abs() < 1e-5).all())
        and bool(((x["pred_scores"] - y["pred_scores"]).abs() < 1e-5).all()) for x, y in zip(a, b))
    assert same, "the two runners disagree on the detections"
    kept = sum(p["pred_boxes"].shape[0] for p in b) / 4.0
    over = float((torch.sigmoid(whole.out["batch_cls_preds"]).max(dim=-1)[0] >= 0.1).sum()) / 4.0
    t = alternate({"two": two_step, "one": one_replay}, iters, windows)
    ratio = statistics.median(t["two"]) / statistics.median(t["one"])
    lines += ["", "SECOND eval, KITTI geometry, batch 4 x 20000 points, random init with fixed logit offsets (%.0f anchors per "
              "frame over the threshold, %.1f boxes kept); us per batch; detections of the two compared equal to 1e-5"
              % (over, kept), "",
              "%-34s %31s %31s %8s" % ("", "GraphedDetector + post_process()", "GraphedAnchorDetector replay", "two/one"),
              "%-34s %s %s %7.2fx" % ("whole model", cell(t["two"]), cell(t["one"]), ratio)]
    return ["whole model"] if ratio <= 1.0 else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    from spx import _lib
    lines = ["device: %s" % torch.cuda.get_device_name(0), "library: %s" % os.path.relpath(_lib.LIB_PATH, ROOT), ""]
    with torch.no_grad():
        losing = post_rows(args.iters, args.windows, lines)
        losing += proposal_rows(args.iters, args.windows, lines)
        if not args.skip_model:
            losing += model_rows(args.iters, args.windows, lines)
    lines += ["", "eager = the per-frame loop the parent commit runs (FUSED absent); the fused and eager results of every "
              "row compared equal before timing (asserted).", "fused NOT faster than eager at: %s" % (", ".join(losing) or "none")]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "dense_post_bench.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
