"""Batched post-processing without a host read (csrc/post_process.hip, include/spx.h §15) on the GPU.

spx_point_post_process against the plain restatement (tests/post_process_ref.py) and against the eager
model_nms_utils.multi_thresh / class_agnostic_nms path, exactly: every comparison is an integer decision or a copied
value, so there is no tolerance anywhere.  Inputs are KITTI-range boxes drawn around a few cluster centres, so that NMS
really suppresses (asserted on the restatement wherever a frame has enough boxes to form clusters, n >= 70), with
distinct scores (a permuted linspace); the tie rule has a test of its own against the restatement only, because the
eager order of equal scores is unspecified.  spx_recall_count against the restated generate_recall_record.  Detector:
fused against eager pred_dicts, the recall record, and post_processing_static under torch.cuda.graph."""
import ctypes
import types

import numpy as np
import pytest
import torch

import post_process_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
THRESH = [0.5, 0.3, 0.3]
NMS_THRESH = 0.1
RECALL_THRESH = [0.3, 0.5, 0.7]


def make_inputs(b, n, seed, classes=(1, 2, 3), grid=False):
    """(scores (b n), labels (b n) int64, boxes (b n, 7)) on the GPU: per frame max(1, n // 12) cluster centres in the
    KITTI range, car-sized boxes within half a metre of them, any heading; scores distinct over the batch.  grid: centres
    and sizes rounded to multiples of 1/64, which makes the axis-aligned IoU exact up to its division
    (post_process_ref.EXACT_GRID)."""
    g = torch.Generator().manual_seed(seed)
    rows = b * n
    scores = torch.linspace(0.05, 0.95, rows)[torch.randperm(rows, generator=g)]
    labels = torch.tensor(classes)[torch.randint(0, len(classes), (rows,), generator=g)]
    boxes = torch.empty(rows, 7)
    for f in range(b):
        nc = max(1, n // 12)
        ctr = torch.rand(nc, 3, generator=g) * torch.tensor([70.0, 80.0, 1.0]) + torch.tensor([0.0, -40.0, -1.5])
        pick = torch.randint(0, nc, (n,), generator=g)
        fb = boxes[f * n:(f + 1) * n]
        fb[:, :3] = ctr[pick] + torch.randn(n, 3, generator=g) * torch.tensor([0.5, 0.5, 0.1])
        fb[:, 3:6] = torch.tensor([3.9, 1.6, 1.56]) * (0.8 + 0.4 * torch.rand(n, 3, generator=g))
        fb[:, 6] = (torch.rand(n, generator=g) * 2 - 1) * np.pi
    if grid:
        boxes[:, :6] = torch.round(boxes[:, :6] / ref.EXACT_GRID) * ref.EXACT_GRID
    return scores.to(DEV), labels.to(DEV), boxes.to(DEV)


def _nms_cfg(pre_max, post_max, axis_aligned):
    return types.SimpleNamespace(NMS_TYPE="nms_normal_gpu" if axis_aligned else "nms_gpu", NMS_THRESH=NMS_THRESH,
                                 NMS_PRE_MAXSIZE=pre_max, NMS_POST_MAXSIZE=post_max, MULTI_CLASSES_NMS=False)


def eager(scores, labels, boxes, b, thresholds, pre_max, post_max, axis_aligned, per_class):
    """Per frame (sel rows of the batch, scores, labels, boxes) from the eager selection code."""
    from pcdet_amd.models.model_utils import model_nms_utils
    n = scores.shape[0] // b
    cfg = _nms_cfg(pre_max, post_max, axis_aligned)
    out = []
    for f in range(b):
        s, lab, bx = (t[f * n:(f + 1) * n] for t in (scores, labels, boxes))
        if per_class:
            sel, sc = model_nms_utils.multi_thresh(box_scores=s, box_labels=lab, box_preds=bx, nms_config=cfg,
                                                   score_thresh=thresholds)
        else:
            sel, sc = model_nms_utils.class_agnostic_nms(box_scores=s, box_preds=bx, nms_config=cfg,
                                                         score_thresh=thresholds[0])
        sel = torch.as_tensor(sel, dtype=torch.int64, device=DEV)
        out.append((sel + f * n, sc, lab[sel], bx[sel]))
    return out


def check_against(got, want):
    """got: ops.point_post_process dict; want: the restatement's."""
    assert np.array_equal(got["count"].cpu().numpy(), want["count"])
    assert np.array_equal(got["sel"].cpu().numpy(), want["sel"])
    assert np.array_equal(got["boxes"].cpu().numpy(), want["boxes"])
    assert np.array_equal(got["scores"].cpu().numpy(), want["scores"])
    assert np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    assert got["sel"].dtype == torch.int64 and got["labels"].dtype == torch.int64 and got["count"].dtype == torch.int32


CASES = {
    "n1": dict(b=2, n=1),
    "n70_crosses_a_wave": dict(b=2, n=70),
    "b3_n512": dict(b=3, n=512),
    "n4096_cap": dict(b=1, n=4096),
    "empty_frame": dict(b=3, n=70, empty_frame=1),
    "class_without_member": dict(b=2, n=70, classes=(1, 3)),
    "pre_max_16": dict(b=2, n=512, pre_max=16),
    "post_max_4": dict(b=2, n=512, post_max=4),
    "axis_aligned": dict(b=2, n=512, axis_aligned=True),
    "agnostic": dict(b=2, n=512, per_class=False),
    "agnostic_axis_aligned_post_max_4": dict(b=2, n=70, per_class=False, axis_aligned=True, post_max=4),
}


@pytest.mark.parametrize("name", list(CASES))
def test_matches_restatement_and_eager_path(name):
    from spx import ops
    c = dict(CASES[name])
    b, n = c["b"], c["n"]
    pre_max, post_max = c.get("pre_max", 4096), c.get("post_max", 512)
    axis_aligned, per_class = c.get("axis_aligned", False), c.get("per_class", True)
    thresholds = THRESH if per_class else [0.3]
    scores, labels, boxes = make_inputs(b, n, seed=len(name), classes=c.get("classes", (1, 2, 3)), grid=axis_aligned)
    if "empty_frame" in c:
        f = c["empty_frame"]
        scores[f * n:(f + 1) * n] *= 0.25          # all below every threshold, still distinct
    got = ops.point_post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, pre_max, post_max,
                                 axis_aligned=axis_aligned, per_class=per_class)
    want = ref.post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, pre_max, post_max,
                            axis_aligned=axis_aligned, per_class=per_class, margin=ref.EXACT_GRID_MARGIN)
    cap = min(n, len(thresholds) * post_max) if per_class else min(n, post_max)
    assert tuple(got["sel"].shape) == (b, cap) and tuple(got["boxes"].shape) == (b, cap, 7)
    if n >= 70:       # the case is not vacuous: NMS removes more than a quarter of what goes into it
        assert want["suppressed"] > want["entered"] / 4, (want["suppressed"], want["entered"])
    if "empty_frame" in c:
        assert int(want["count"][c["empty_frame"]]) == 0 and int(want["count"].sum()) > 0
    if "classes" in c:
        assert not bool((got["labels"] == 2).any())
    check_against(got, want)
    # padding is exactly -1 / 0
    count = got["count"].cpu().numpy()
    for f in range(b):
        k = int(count[f])
        assert bool((got["sel"][f, k:] == -1).all()) and bool((got["sel"][f, :k] >= f * n).all())
        assert bool((got["sel"][f, :k] < (f + 1) * n).all())
        for key in ("boxes", "scores", "labels"):
            assert bool((got[key][f, k:] == 0).all()), key
    # and the eager path selects the same rows in the same order
    for f, (sel, sc, lab, bx) in enumerate(eager(scores, labels, boxes, b, thresholds, pre_max, post_max, axis_aligned,
                                                 per_class)):
        k = int(count[f])
        assert sel.shape[0] == k
        assert torch.equal(got["sel"][f, :k], sel)
        assert torch.equal(got["scores"][f, :k], sc)
        assert torch.equal(got["labels"][f, :k], lab)
        assert torch.equal(got["boxes"][f, :k], bx)


def test_equal_scores_take_the_lower_row_first_and_runs_repeat_bitwise():
    from spx import ops
    b, n = 2, 512
    scores, labels, boxes = make_inputs(b, n, seed=21)
    scores = (torch.floor(scores * 8) / 8 + 0.0625).contiguous()           # 8 distinct values
    assert scores.unique().numel() == 8
    for per_class, thresholds in ((True, THRESH), (False, [0.3])):
        want = ref.post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, 64, 16, per_class=per_class)
        first = ops.point_post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, 64, 16, per_class=per_class)
        second = ops.point_post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, 64, 16, per_class=per_class)
        assert int(want["count"].min()) > 4
        check_against(first, want)
        for key in first:
            assert torch.equal(first[key], second[key]), key


def test_prefilled_outputs_are_fully_overwritten():
    from spx import _lib, ops
    lib = _lib.load()
    b, n, post_max = 3, 70, 4
    scores, labels, boxes = make_inputs(b, n, seed=5)
    scores[n:2 * n] *= 0.25                                                # frame 1: count 0, all padding
    want = ops.point_post_process(scores, labels, boxes, b, THRESH, NMS_THRESH, 4096, post_max)
    cap = want["sel"].shape[1]
    assert cap == 12 and int(want["count"][1]) == 0 and int(want["count"].max()) < cap
    sel = torch.full((b, cap), -7, dtype=torch.int64, device=DEV)
    count = torch.full((b,), -7, dtype=torch.int32, device=DEV)
    ob = torch.full((b, cap, 7), float("nan"), device=DEV)
    osc = torch.full((b, cap), float("nan"), device=DEV)
    ol = torch.full((b, cap), -7, dtype=torch.int64, device=DEV)
    wsb = lib.spx_point_post_process_ws_bytes(b, n, 3, post_max)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())    # noqa: E731
    lab32 = labels.int()
    rc = lib.spx_point_post_process(p(scores), p(lab32), p(boxes), b, n, _lib.f_arr(THRESH), 3, NMS_THRESH, 4096, post_max,
                                    0, 1, p(sel), p(count), p(ob), p(osc), p(ol), p(ws), wsb, ops._stream(scores))
    torch.cuda.synchronize()
    assert rc == 0
    for a, w in ((sel, want["sel"]), (count, want["count"]), (ob, want["boxes"]), (osc, want["scores"]),
                 (ol, want["labels"])):
        assert torch.equal(a, w)
    assert bool(torch.isfinite(ob).all()) and bool(torch.isfinite(osc).all())
    assert bool((sel[1] == -1).all()) and bool((ob[1] == 0).all()) and bool((ol[1] == 0).all())


def test_shape_mismatch_and_too_many_candidates_raise():
    from spx import _lib, ops
    scores, labels, boxes = make_inputs(2, 8, seed=1)
    with pytest.raises(_lib.SpxError):
        ops.point_post_process(scores, labels[:-1], boxes, 2, THRESH, NMS_THRESH, 16, 8)
    with pytest.raises(_lib.SpxError):
        ops.point_post_process(scores, labels, boxes, 3, THRESH, NMS_THRESH, 16, 8)        # 16 rows, 3 frames
    with pytest.raises(_lib.SpxError):
        ops.point_post_process(scores, labels, boxes[:, :6], 2, THRESH, NMS_THRESH, 16, 8)
    with pytest.raises(_lib.SpxError):
        ops.point_post_process(scores, labels, boxes, 2, THRESH, NMS_THRESH, 16, 8, per_class=False)
    big = torch.zeros(4097, device=DEV)
    with pytest.raises(_lib.SpxError, match="code -5"):
        ops.point_post_process(big, big.long(), torch.zeros(4097, 7, device=DEV), 1, THRESH, NMS_THRESH, 16, 8)
    res = ops.point_post_process(scores, labels, boxes, 2, THRESH, NMS_THRESH, 16, 8)
    with pytest.raises(_lib.SpxError):
        ops.recall_count(res["boxes"], res["count"], torch.zeros(3, 4, 8, device=DEV), RECALL_THRESH)


def _gt_from(kept, g, cols, gen, n_real):
    """(g, cols) gt rows: n_real kept boxes, the first as it is and the others shifted and resized a little so that
    the IoUs spread over (0, 1), then zero rows."""
    gt = torch.zeros(g, cols)
    if n_real:
        src = kept[torch.randint(0, kept.shape[0], (n_real,), generator=gen)].cpu()
        keep0 = src[0].clone()       # row 0 stays an exact copy: recalled at every threshold whatever the box sizes
        src[:, :3] += torch.randn(n_real, 3, generator=gen) * torch.tensor([0.4, 0.2, 0.1])
        src[:, 3:6] *= 0.85 + 0.3 * torch.rand(n_real, 3, generator=gen)
        src[0] = keep0
        gt[:n_real, :7] = src
        if cols > 7:
            gt[:n_real, 7] = 1.0
    return gt


def test_recall_count_matches_restated_recall_record():
    from spx import ops
    b, n = 4, 70
    scores, labels, boxes = make_inputs(b, n, seed=9)
    scores[n:2 * n] *= 0.25                                                # frame 1 keeps no box
    res = ops.point_post_process(scores, labels, boxes, b, THRESH, NMS_THRESH, 4096, 512)
    count = res["count"].cpu().numpy()
    assert count[1] == 0 and count[0] > 2 and count[2] > 2 and count[3] > 2
    gen = torch.Generator().manual_seed(3)
    gt = torch.stack([_gt_from(res["boxes"][0, :count[0]], 9, 8, gen, 6),      # trailing zero rows
                      _gt_from(boxes[n:2 * n], 9, 8, gen, 5),                  # a frame with no kept box
                      _gt_from(None, 9, 8, gen, 0),                            # all zero: row 0 still counts
                      _gt_from(res["boxes"][3, :count[3]], 9, 8, gen, 9)]).to(DEV)   # no padding at all
    recalled, num_gt = ops.recall_count(res["boxes"], res["count"], gt, RECALL_THRESH)
    want_rec, want_gt = ref.recall(res["boxes"], count, gt, RECALL_THRESH)
    assert list(want_gt) == [6, 5, 1, 9]
    assert want_rec[0, 0] > want_rec[0, 2] or want_rec[3, 0] > want_rec[3, 2]      # the thresholds tell boxes apart
    assert want_rec[0, 0] > 0 and not want_rec[1].any() and not want_rec[2].any()
    assert recalled.dtype == torch.int32 and num_gt.dtype == torch.int32
    assert np.array_equal(num_gt.cpu().numpy(), want_gt)
    assert np.array_equal(recalled.cpu().numpy(), want_rec)
    # 7-column gt rows
    gt7 = gt[:, :, :7].contiguous()
    rec2, num2 = ops.recall_count(res["boxes"], res["count"], gt7, RECALL_THRESH)
    w2, g2 = ref.recall(res["boxes"], count, gt7, RECALL_THRESH)
    assert np.array_equal(rec2.cpu().numpy(), w2) and np.array_equal(num2.cpu().numpy(), g2)
    # outputs pre-filled with -7 are fully overwritten (through the C entry point, on the caller's buffers)
    from spx import _lib
    rec3 = torch.full((b, 3), -7, dtype=torch.int32, device=DEV)
    num3 = torch.full((b,), -7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())    # noqa: E731
    rc = _lib.load().spx_recall_count(p(res["boxes"]), p(res["count"]), b, res["boxes"].shape[1], p(gt), gt.shape[1],
                                      gt.shape[2], _lib.f_arr(RECALL_THRESH), 3, p(rec3), p(num3), ops._stream(gt))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(rec3, recalled) and torch.equal(num3, num_gt)


# ------------------------------------------------------------------------------------------------------ detector
@pytest.fixture(scope="module")
def head_out():
    """(net, out): the fast_cpc detector of tests/test_gpu_point_head.py and its head outputs for two frames, with the
    logits replaced by distinct, well separated values so that the thresholds and NMS have work."""
    from test_gpu_point_head import _net, _points
    net = _net(seed=2)
    with torch.no_grad():
        out = {"batch_size": 2, "points": _points(2, 16384, seed=41)}
        for m in net.module_list:
            out = m(out)
    g = torch.Generator().manual_seed(4)
    shape = out["batch_cls_preds"].shape
    out["batch_cls_preds"] = torch.linspace(-3.0, 4.0, shape.numel())[torch.randperm(shape.numel(), generator=g)] \
        .view(shape).to(DEV)
    return net, out


def _post(net, out, fused, raw=False):
    cfg = net.model_cfg.POST_PROCESSING
    cfg["FUSED"], cfg["OUTPUT_RAW_SCORE"] = fused, raw
    try:
        with torch.no_grad():
            return net.post_processing(dict(out))
    finally:
        cfg.pop("FUSED")
        cfg["OUTPUT_RAW_SCORE"] = False


def _same_preds(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_detector_fused_equals_eager_and_reports_recall(head_out, monkeypatch):
    from spx import ops
    net, out = head_out
    assert net._fused_post_plan(out) is not None
    calls = []
    real = ops.point_post_process
    monkeypatch.setattr(ops, "point_post_process", lambda *a, **k: calls.append(1) or real(*a, **k))
    fused, rec = _post(net, out, True)
    assert len(calls) == 1                                  # the fused branch really ran ...
    eager_, rec_e = _post(net, out, False)
    assert len(calls) == 1                                  # ... and FUSED: False keeps off it
    with torch.no_grad():
        auto, _ = net.post_processing(dict(out))            # FUSED not set: 512 candidates per frame go the fused way
    assert len(calls) == 2 and "FUSED" not in net.model_cfg.POST_PROCESSING
    _same_preds(auto, fused)
    assert rec == {} and rec_e == {}
    assert sum(p["pred_boxes"].shape[0] for p in eager_) > 4
    _same_preds(fused, eager_)
    _same_preds(_post(net, out, True, raw=True)[0], _post(net, out, False, raw=True)[0])
    raw_scores = torch.cat([p["pred_scores"] for p in _post(net, out, True, raw=True)[0]])
    assert not torch.equal(raw_scores, torch.cat([p["pred_scores"] for p in fused]))      # logits, not probabilities
    # the recall record, with gt boxes made from the predictions
    gen = torch.Generator().manual_seed(8)
    src = [p["pred_boxes"] if p["pred_boxes"].shape[0] else out["batch_box_preds"][i * 512:(i + 1) * 512]
           for i, p in enumerate(fused)]       # a frame without detections takes its gt from the head's boxes
    gt = torch.stack([_gt_from(src[0], 7, 8, gen, 5), _gt_from(src[1], 7, 8, gen, 3)])
    with_gt = dict(out, gt_boxes=gt.to(DEV))
    fused2, rec = _post(net, with_gt, True)
    eager2, rec_e = _post(net, with_gt, False)
    _same_preds(fused2, eager2)
    _same_preds(fused2, fused)
    keys = {"gt"} | {"%s_%s" % (p, t) for p in ("roi", "rcnn") for t in ("0.3", "0.5", "0.7")}
    assert set(rec) == keys and rec == rec_e
    assert all(type(v) is int for v in rec.values())
    padded = torch.zeros(2, 512, 7, device=DEV)
    count = np.array([p["pred_boxes"].shape[0] for p in fused])
    for i, p in enumerate(fused):
        padded[i, :count[i]] = p["pred_boxes"]
    want_rec, want_gt = ref.recall(padded, count, with_gt["gt_boxes"], RECALL_THRESH)
    assert rec["gt"] == int(want_gt.sum()) == 8
    for i, t in enumerate(RECALL_THRESH):
        assert rec["rcnn_%s" % t] == int(want_rec[:, i].sum()) and rec["roi_%s" % t] == 0
    assert rec["rcnn_0.3"] > 0
    # a batch the fused path cannot take (frames of different lengths) falls back to the eager code
    uneven = dict(out)
    uneven["batch_index"] = out["batch_index"].clone()
    uneven["batch_index"][500:512] = 1.0
    _same_preds(_post(net, uneven, True)[0], _post(net, uneven, False)[0])


def test_static_post_processing_captures_and_replays(head_out):
    net, out = head_out
    static_in = dict(out)
    static_in["batch_cls_preds"] = out["batch_cls_preds"].clone()
    static_in["batch_box_preds"] = out["batch_box_preds"].clone()
    gen = torch.Generator().manual_seed(12)
    static_in["gt_boxes"] = torch.stack([_gt_from(out["batch_box_preds"][:512], 6, 8, gen, 4),
                                         _gt_from(out["batch_box_preds"][512:], 6, 8, gen, 6)]).to(DEV)
    with torch.no_grad():
        first = net.post_processing_static(static_in)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net.post_processing_static(static_in)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = net.post_processing_static(static_in)
        # a second input through the captured pointers
        perm = torch.randperm(1024, generator=torch.Generator().manual_seed(13)).to(DEV)
        static_in["batch_cls_preds"].copy_(out["batch_cls_preds"][perm])
        static_in["batch_box_preds"][:, :2].add_(0.05)
        graph.replay()
        torch.cuda.synchronize()
        fresh = net.post_processing_static(static_in)
        pred_dicts, recall = net.post_processing(static_in)
    assert set(captured) == set(fresh) == {"sel", "count", "pred_boxes", "pred_scores", "pred_labels", "layout_ok",
                                            "recalled", "num_gt"}
    for k in fresh:
        assert torch.equal(captured[k], fresh[k]), k
    assert bool(fresh["layout_ok"]) and int(fresh["count"].sum()) > 4
    assert not torch.equal(fresh["sel"], first["sel"])
    for i, p in enumerate(pred_dicts):
        k = int(fresh["count"][i])
        assert torch.equal(p["pred_boxes"], fresh["pred_boxes"][i, :k])
    assert recall["gt"] == int(fresh["num_gt"].sum())
