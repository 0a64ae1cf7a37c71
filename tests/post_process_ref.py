"""Plain restatement of spx_point_post_process and spx_recall_count (include/spx.h §15) for the tests.

Ordering is a stable descending sort, so equal scores keep the lower row first.  The pair IoUs come from the library's
own IoU matrix (ops.boxes_iou_bev, entry [i, j] = iou(box i, box j)), read as [earlier, later]; the greedy loops run on
the host.  That matrix is pinned to a float64 reference of its own, and the three NMS paths to one decision per pair, in
tests/box_iou_ref.py / tests/test_gpu_box_iou.py.  The axis-aligned IoU has no matrix entry point: it is restated in float64 and the caller must give inputs
whose IoUs keep clear of the NMS threshold (checked here), so that fp32 rounding cannot change a decision.
Recall follows the reference's generate_recall_record with iou3d_nms_utils.boxes_iou3d_gpu."""
import numpy as np
import torch

# How far every axis-aligned IoU must stay from the NMS threshold.  General KITTI-range boxes: the fp32 edges carry half
# an ulp of ~70 m (4e-6), which reaches the IoU of car-sized boxes as ~1.5e-5, hence 2e-5.  Boxes whose centres and sizes
# are multiples of 1/64 (EXACT_GRID): edges, overlaps, areas and the union are exact in fp32 (at most 20 significant bits,
# contraction or not), only the final division rounds (6e-8 relative), hence 1e-7.
GENERAL_MARGIN = 2e-5
EXACT_GRID_MARGIN = 1e-7
EXACT_GRID = 1.0 / 64


def iou_matrix(boxes, axis_aligned, nms_thresh, margin=GENERAL_MARGIN):
    """boxes (n, 7) cuda fp32 -> (n, n) numpy IoU, [i, j] = iou(i, j)."""
    if not axis_aligned:
        from spx import ops
        return ops.boxes_iou_bev(boxes, boxes).cpu().numpy()
    b = boxes.double().cpu().numpy()
    x0, x1 = b[:, 0] - b[:, 3] / 2, b[:, 0] + b[:, 3] / 2
    y0, y1 = b[:, 1] - b[:, 4] / 2, b[:, 1] + b[:, 4] / 2
    w = np.maximum(np.minimum(x1[:, None], x1[None]) - np.maximum(x0[:, None], x0[None]), 0)
    h = np.maximum(np.minimum(y1[:, None], y1[None]) - np.maximum(y0[:, None], y0[None]), 0)
    inter = w * h
    area = b[:, 3] * b[:, 4]
    iou = inter / np.maximum(area[:, None] + area[None] - inter, 1e-8)
    assert np.abs(iou - nms_thresh).min() > margin, "an axis-aligned IoU sits on the threshold"
    return iou


def greedy(iou, order, thresh):
    """order: rows in score order -> (kept rows in that order, number suppressed)."""
    sub = iou[np.ix_(order, order)]
    m = len(order)
    removed = np.zeros(m, dtype=bool)
    later = np.arange(m)
    kept = []
    for i in range(m):
        if removed[i]:
            continue
        kept.append(order[i])
        removed |= (sub[i] > np.float32(thresh)) & (later > i)
    return np.asarray(kept, dtype=np.int64), int(removed.sum())


def _ordered(rows, scores):
    """rows by score descending, equal scores lower row first (a stable sort of the rows in ascending order)."""
    rows = np.sort(rows)
    return rows[np.argsort(-scores[rows], kind="stable")]


def post_process(scores, labels, boxes, batch_size, thresholds, nms_thresh, pre_max, post_max, axis_aligned=False,
                 per_class=True, margin=GENERAL_MARGIN):
    """Same arguments as ops.point_post_process (cuda tensors; margin: see GENERAL_MARGIN) -> dict of numpy arrays sel, count, boxes, scores, labels,
    and `entered` / `suppressed`: boxes that went into an NMS and boxes an NMS removed, over the batch."""
    s = scores.float().cpu().numpy()
    lab = labels.cpu().numpy().astype(np.int64)
    bx = boxes[:, :7].float().cpu().numpy()
    b = int(batch_size)
    n = s.shape[0] // b
    nt = len(thresholds)
    cap = min(n, nt * post_max) if per_class else min(n, post_max)
    out = {"sel": np.full((b, cap), -1, np.int64), "count": np.zeros(b, np.int32),
           "boxes": np.zeros((b, cap, 7), np.float32), "scores": np.zeros((b, cap), np.float32),
           "labels": np.zeros((b, cap), np.int64), "entered": 0, "suppressed": 0}
    for f in range(b):
        lo = f * n
        fs, fl = s[lo:lo + n], lab[lo:lo + n]
        iou = iou_matrix(boxes[lo:lo + n, :7].float().contiguous(), axis_aligned, nms_thresh, margin)
        survivors = []
        for c in range(nt):
            member = fs >= np.float32(thresholds[c])
            if per_class:
                member &= fl == c + 1
            order = _ordered(np.nonzero(member)[0], fs)[:pre_max]
            kept, gone = greedy(iou, order, nms_thresh)
            out["entered"] += len(order)
            out["suppressed"] += gone
            survivors.append(kept[:post_max])
        final = np.concatenate(survivors) if survivors else np.zeros(0, np.int64)
        if per_class:
            final, gone = greedy(iou, _ordered(final, fs), nms_thresh)
            out["suppressed"] += gone
        k = len(final)
        out["count"][f] = k
        out["sel"][f, :k] = final + lo
        out["boxes"][f, :k] = bx[final + lo]
        out["scores"][f, :k] = s[final + lo]
        out["labels"][f, :k] = lab[final + lo]
    return out


def recall(out_boxes, count, gt_boxes, thresholds):
    """out_boxes (B, K, 7), count (B), gt_boxes (B, G, >= 7) cuda tensors -> (recalled (B, T), num_gt (B)) numpy."""
    from pcdet_amd.ops.iou3d_nms import iou3d_nms_utils
    b = out_boxes.shape[0]
    recalled = np.zeros((b, len(thresholds)), np.int32)
    num_gt = np.zeros(b, np.int32)
    for f in range(b):
        cur_gt = gt_boxes[f]
        k = cur_gt.shape[0] - 1
        while k > 0 and float(cur_gt[k].sum()) == 0:
            k -= 1
        cur_gt = cur_gt[:k + 1]
        num_gt[f] = cur_gt.shape[0]
        pred = out_boxes[f, :int(count[f])]
        if cur_gt.shape[0] == 0 or pred.shape[0] == 0:
            continue
        iou3d = iou3d_nms_utils.boxes_iou3d_gpu(pred[:, 0:7].contiguous(), cur_gt[:, 0:7].contiguous())
        best = iou3d.max(dim=0)[0]
        for i, t in enumerate(thresholds):
            recalled[f, i] = int((best > t).sum().item())
    return recalled, num_gt
