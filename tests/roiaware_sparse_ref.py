"""float32 numpy restatement of the batched sparse RoI-aware pooling (include/spx.h §30, csrc/roiaware_sparse.hip), built
on the functions of roiaware_ref.py: the batch loop (RoI row r = b * N + n sees the points of frame b only), the
non-zero-sum emit rule, the row order of nonzero(), the fake branch, static capacity, and the backward in its fixed
order; and the ragged points-in-boxes."""
import numpy as np

import roiaware_ref as ref

F32 = np.float32


def frame_spans(frame_cnt):
    """counts (B) -> starts (B): frame b owns the rows [start[b], start[b] + cnt[b])."""
    cnt = np.asarray(frame_cnt, np.int64)
    return np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)


def points_in_boxes_stack(points_bxyz, boxes):
    """points (P, 4) [frame, x, y, z] in any order, boxes (B, M, 7) -> (P) int32: the first box of the point's own frame
    holding it, -1 when none or when the frame is outside [0, B)."""
    pts = np.asarray(points_bxyz, F32)
    boxes = np.asarray(boxes, F32)
    out = np.full((pts.shape[0],), -1, np.int32)
    for b in range(boxes.shape[0]):
        sel = np.nonzero((pts[:, 0] >= F32(b)) & (pts[:, 0] < F32(b + 1)))[0]    # (int) of the float frame value
        if sel.size and boxes.shape[1]:
            out[sel] = ref.points_in_boxes(pts[None, sel, 1:4], boxes[b:b + 1])[0]
    return out


def collect(rois, points, frame_cnt, part, out_size, max_pts):
    """Per RoI row r: the frame's pool over the 4 part channels (avg), the emitted cells and what the backward reads.
    -> list over r of dict(start, pt_cell (P_b), vox_cnt (V), part (V, 4), emit (V) bool, lists)."""
    rois = np.asarray(rois, F32)
    pts = np.asarray(points, F32)
    part = np.asarray(part, F32)
    b, n = rois.shape[:2]
    starts = frame_spans(frame_cnt)
    V = int(np.prod(out_size))
    per = []
    for f in range(b):
        s, e = int(starts[f]), int(starts[f]) + int(frame_cnt[f])
        avg, _, pt_cell, vox_cnt = ref.pool_fwd(rois[f], pts[s:e, 1:4], part[s:e], out_size, max_pts, 1)
        _, _, lists = ref.collect(rois[f], pts[s:e, 1:4], out_size, max_pts)
        avg = avg.reshape(n, V, 4)
        vox_cnt = vox_cnt.reshape(n, V)
        with np.errstate(invalid="ignore"):
            tot = ((avg[..., 0] + avg[..., 1]) + avg[..., 2]) + avg[..., 3]
        emit = (vox_cnt > 0) & (tot != 0)                                      # NaN != 0, as nonzero() has it
        for i in range(n):
            per.append({"start": s, "pt_cell": pt_cell[i], "vox_cnt": vox_cnt[i], "part": avg[i], "emit": emit[i],
                        "lists": lists[i]})
    return per


def pool(rois, points, frame_cnt, part, rpn, out_size, max_pts, rows=None):
    """-> dict(n_rows, faked, coords (rows, 4), part (rows, 4), rpn (rows, C), arg (rows, C) global point rows, cnt
    (rows), row_of_cell (B * N * V), overflow, per): rows None = exactly n_rows; rows at and past n_rows are dead
    (features 0, cnt 0, arg -1, coords -1); rows past the capacity are dropped (overflow True)."""
    rpn = np.asarray(rpn, F32)
    c = rpn.shape[1]
    ox, oy, oz = out_size
    V = ox * oy * oz
    per = collect(rois, points, frame_cnt, part, out_size, max_pts)
    R = len(per)
    n_emit = sum(int(p["emit"].sum()) for p in per)
    faked = n_emit < 3
    cells = [(r, 0) for r in range(R)] if faked else [(r, int(v)) for r in range(R) for v in np.nonzero(per[r]["emit"])[0]]
    n_rows = len(cells)
    cap = n_rows if rows is None else int(rows)
    out = {"n_rows": n_rows, "faked": int(faked), "overflow": n_rows > cap, "per": per,
           "coords": np.full((cap, 4), -1, np.int32), "part": np.zeros((cap, 4), F32), "rpn": np.zeros((cap, c), F32),
           "arg": np.full((cap, c), -1, np.int32), "cnt": np.zeros((cap,), np.int32),
           "row_of_cell": np.full((R * V,), -1, np.int32)}
    for row, (r, v) in enumerate(cells[:cap]):
        p = per[r]
        out["coords"][row] = (r, v // (oy * oz), (v // oz) % oy, v % oz)
        out["row_of_cell"][r * V + v] = row
        L = p["lists"].get(v)
        if L is None:                                                        # the fake row of an empty cell
            continue
        L = L + p["start"]                                                   # global point rows, ascending
        out["cnt"][row] = L.size
        out["part"][row] = p["part"][v]
        vals = rpn[L]
        m = np.where(np.isnan(vals), -np.inf, vals)
        best = m.max(axis=0)
        first = np.argmax(m == best[None], axis=0)                           # strict > in list order: the first maximum
        win = best > -np.inf
        out["arg"][row] = np.where(win, L[first], -1)
        out["rpn"][row] = np.where(win, m[first, np.arange(c)], F32(0))
    return out


def pool_bwd(fwd, grad, n_points, n_per, mode):
    """grad (rows, C) -> grad_in (P, C): from 0.0f, the RoI rows of the point's frame in ascending r; mode 0 = max
    (grad where arg == p), 1 = avg (grad * (1 / max(cnt, 1)))."""
    g = np.asarray(grad, F32)
    c = g.shape[1]
    per = fwd["per"]
    V = fwd["row_of_cell"].size // max(len(per), 1)
    grad_in = np.zeros((n_points, c), F32)
    for r, p in enumerate(per):
        q = np.nonzero(p["pt_cell"] >= 0)[0]
        if q.size == 0:
            continue
        row = fwd["row_of_cell"][r * V + p["pt_cell"][q]]
        q, row = q[row >= 0], row[row >= 0]
        gp = q + p["start"]
        if mode == 0:
            add = np.where(fwd["arg"][row] == gp[:, None], g[row], F32(0))
        else:
            scale = F32(1) / np.maximum(fwd["cnt"][row].astype(F32), F32(1))
            add = g[row] * scale[:, None]
        grad_in[gp] = grad_in[gp] + add
    return grad_in
