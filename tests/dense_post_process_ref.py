"""Plain restatement of spx_dense_select and spx_dense_post_process (include/spx.h §29) for the tests.

Selection runs over all n rows of a frame with np.lexsort (score descending, equal scores lower row first; -0.0 equals
0.0; a NaN is never a member).  The IoU matrix is built over the SELECTED rows only (a frame may have 3e5 rows), by the
library's own matrix (ops.boxes_iou_bev) or the float64 axis-aligned form of tests/post_process_ref.py, whose greedy
loop, ordering rule and margins are reused as they are."""
import numpy as np
import torch

import post_process_ref as ref


def _members(fs, fl, c, thresholds, per_class):
    member = ~np.isnan(fs)
    if thresholds is not None:
        with np.errstate(invalid="ignore"):
            member &= fs >= np.float32(thresholds[c])
    if per_class:
        member &= fl == c + 1
    return np.nonzero(member)[0]


def _select_frame(fs, fl, nt, thresholds, pre_max, per_class):
    out = []
    for c in range(nt):
        rows = _members(fs, fl, c, thresholds, per_class)
        out.append(rows[np.lexsort((rows, -fs[rows]))][:pre_max])
    return out


def select(scores, labels, batch_size, thresholds, pre_max, per_class=True):
    """Same arguments as ops.dense_select (tensors anywhere) -> (cand (B, T, pre_max) int64, count (B, T) int32)."""
    s = scores.float().cpu().numpy()
    lab = labels.cpu().numpy().astype(np.int64)
    b = int(batch_size)
    n = s.shape[0] // b if b else 0
    nt = 1 if thresholds is None else len(thresholds)
    cand = np.full((b, nt, pre_max), -1, np.int64)
    count = np.zeros((b, nt), np.int32)
    for f in range(b):
        for c, rows in enumerate(_select_frame(s[f * n:(f + 1) * n], lab[f * n:(f + 1) * n], nt, thresholds, pre_max,
                                               per_class)):
            cand[f, c, :len(rows)] = rows + f * n
            count[f, c] = len(rows)
    return cand, count


def post_process(scores, labels, boxes, batch_size, thresholds, nms_thresh, pre_max, post_max, axis_aligned=False,
                 per_class=True, margin=ref.GENERAL_MARGIN):
    """Same arguments as ops.dense_post_process (cuda tensors) -> the dict of post_process_ref.post_process, plus
    `final_suppressed`: boxes the cross-class NMS removed."""
    s = scores.float().cpu().numpy()
    lab = labels.cpu().numpy().astype(np.int64)
    bx = boxes[:, :7].float()
    b = int(batch_size)
    n = s.shape[0] // b
    nt = 1 if thresholds is None else len(thresholds)
    cap = min(n, nt * min(post_max, n)) if per_class else min(n, post_max)
    out = {"sel": np.full((b, cap), -1, np.int64), "count": np.zeros(b, np.int32),
           "boxes": np.zeros((b, cap, 7), np.float32), "scores": np.zeros((b, cap), np.float32),
           "labels": np.zeros((b, cap), np.int64), "entered": 0, "suppressed": 0, "final_suppressed": 0}
    for f in range(b):
        lo = f * n
        fs, fl = s[lo:lo + n], lab[lo:lo + n]
        orders = _select_frame(fs, fl, nt, thresholds, pre_max, per_class)
        used = np.unique(np.concatenate(orders)) if orders else np.zeros(0, np.int64)
        if len(used) == 0:
            continue
        sub = bx[torch.as_tensor(used + lo, device=bx.device)].contiguous()      # boxes of the selected rows only
        iou = ref.iou_matrix(sub, axis_aligned, nms_thresh, margin)
        us = fs[used]
        survivors = []
        for order in orders:
            local = np.searchsorted(used, order)
            kept, gone = ref.greedy(iou, local, nms_thresh)
            out["entered"] += len(local)
            out["suppressed"] += gone
            survivors.append(kept[:post_max])
        final = np.concatenate(survivors)
        if per_class:
            final, gone = ref.greedy(iou, ref._ordered(final, us), nms_thresh)
            out["suppressed"] += gone
            out["final_suppressed"] += gone
        rows = used[final] + lo
        k = len(rows)
        out["count"][f] = k
        out["sel"][f, :k] = rows
        out["boxes"][f, :k] = bx[torch.as_tensor(rows, device=bx.device)].cpu().numpy()
        out["scores"][f, :k] = s[rows]
        out["labels"][f, :k] = lab[rows]
    return out
