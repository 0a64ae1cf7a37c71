"""float32 numpy restatement of the roiaware_pool3d op set (include/spx.h §12, csrc/roiaware_pool3d.hip): the inside
test at both margins, the cell encoding, the capped ordered collection, both pools and the ascending-RoI backward.
Every rounding step is spelled out: float32 operations round after each operation, the box limits are compared in
float64, cos / sin are taken in float64 of the float32 angle and rounded once."""
import numpy as np

F32, F64 = np.float32, np.float64
GPU_MARGIN = F64(F32(1e-5))
CPU_MARGIN = F64(F32(1e-2))


def box_consts(boxes):
    """(..., 7) float32 -> dict of per-box constants, each (..., 1) to broadcast against points."""
    b = np.asarray(boxes, F32)
    c = {k: b[..., i, None] for i, k in enumerate(("cx", "cy", "cz", "dx", "dy", "dz", "rz"))}
    c["cosa"] = np.cos(-c["rz"].astype(F64)).astype(F32)
    c["sina"] = np.sin(-c["rz"].astype(F64)).astype(F32)
    return c


def in_box(pts, boxes, margin=GPU_MARGIN):
    """pts (P, 3), boxes (N, 7) -> inside (N, P) bool, local_x, local_y (N, P) float32."""
    p = np.asarray(pts, F32)
    c = box_consts(boxes)
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    sx, sy = x - c["cx"], y - c["cy"]
    lx = sx * c["cosa"] + sy * (-c["sina"])
    ly = sx * c["sina"] + sy * c["cosa"]
    with np.errstate(invalid="ignore"):
        zin = ~(np.abs(z - c["cz"]).astype(F64) > c["dz"].astype(F64) / 2.0)
        inside = zin & (np.abs(lx).astype(F64) < c["dx"].astype(F64) / 2.0 + margin) \
            & (np.abs(ly).astype(F64) < c["dy"].astype(F64) / 2.0 + margin)
    return inside, lx, ly


def points_in_boxes(pts, boxes):
    """pts (B, M, 3), boxes (B, T, 7) -> (B, M) int32: the first box index holding each point, else -1."""
    pts, boxes = np.asarray(pts, F32), np.asarray(boxes, F32)
    b, m = pts.shape[:2]
    t = boxes.shape[1]
    out = np.full((b, m), -1, np.int32)
    if t == 0:
        return out
    chunk = max(1, (1 << 20) // t)                                     # (box, point) pairs held at once
    for i in range(b):
        for s in range(0, m, chunk):
            ins = in_box(pts[i, s:s + chunk], boxes[i])[0]            # (T, chunk)
            any_ = ins.any(axis=0)
            out[i, s:s + chunk] = np.where(any_, ins.argmax(axis=0), -1)
    return out


def points_in_boxes_cpu(pts, boxes):
    """The reference's host op: (N, P) int32 0/1 mask at margin 1e-2."""
    return in_box(pts, boxes, CPU_MARGIN)[0].astype(np.int32)


def f2i_sat(f):
    """float32 -> int32 as the hardware convert does it: truncate, saturate, NaN -> 0."""
    t = np.trunc(np.asarray(f, F32).astype(F64))
    t = np.where(np.isnan(t), 0.0, np.clip(t, -2147483648.0, 2147483647.0))
    return t.astype(np.int64)


def cell_axis(local, d, o):
    """int((local + d / 2) / (d / o)) stored unsigned and clamped with an unsigned min to o - 1."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        res = d / F32(o)
        f = (local + d / F32(2)) / res
    u = f2i_sat(f) & 0xFFFFFFFF
    return np.minimum(u, o - 1).astype(np.int64)


def cell_codes(rois, pts, out_size):
    """(N, P) int64: linear cell (x*oy + y)*oz + z of each in-box (RoI, point), -1 outside (GPU margin)."""
    ox, oy, oz = out_size
    pts = np.asarray(pts, F32)
    ins, lx, ly = in_box(pts, rois)
    c = box_consts(rois)
    lz = pts[None, :, 2] - c["cz"]
    code = (cell_axis(lx, c["dx"], ox) * oy + cell_axis(ly, c["dy"], oy)) * oz + cell_axis(lz, c["dz"], oz)
    return np.where(ins, code, -1)


def collect(rois, pts, out_size, max_pts):
    """The capped ordered collection -> pt_cell (N, P) int32 (cell of each kept point, else -1), vox_cnt (N, V) int32 and
    lists: per RoI a dict cell -> ascending array of the kept point indices."""
    code = cell_codes(rois, pts, out_size)
    n, npt = code.shape
    V = int(np.prod(out_size))
    cap = max_pts - 1
    pt_cell = np.full((n, npt), -1, np.int32)
    vox_cnt = np.zeros((n, V), np.int32)
    lists = []
    for r in range(n):
        idx = np.nonzero(code[r] >= 0)[0]                          # ascending point index
        cells = code[r, idx]
        order = np.argsort(cells, kind="stable")
        sc, si = cells[order], idx[order]
        start = np.searchsorted(sc, sc, side="left")
        rank = np.arange(sc.size) - start
        keep = rank < cap
        pt_cell[r, si[keep]] = sc[keep]
        uc, cnt = np.unique(sc[keep], return_counts=True)
        vox_cnt[r, uc] = cnt
        lists.append({int(v): si[keep][sc[keep] == v] for v in uc})
    return pt_cell, vox_cnt, lists


def pool_fwd(rois, pts, feats, out_size, max_pts, mode):
    """-> pooled (N, ox, oy, oz, C) float32, argmax (same, int32; None for avg), pt_cell (N, P), vox_cnt (N, ox, oy, oz)."""
    feats = np.asarray(feats, F32)
    n, c = len(rois), feats.shape[1]
    V = int(np.prod(out_size))
    pt_cell, vox_cnt, lists = collect(rois, pts, out_size, max_pts)
    pooled = np.zeros((n, V, c), F32)
    argmax = np.full((n, V, c), -1, np.int32)
    for r in range(n):
        for v, L in lists[r].items():
            vals = feats[L]                                          # (k, C) in list order
            if mode == 0:
                m = np.where(np.isnan(vals), -np.inf, vals)
                best = m.max(axis=0)
                first = np.argmax(m == best[None], axis=0)           # the first maximum: strict > in list order
                win = best > -np.inf
                argmax[r, v] = np.where(win, L[first], -1)
                pooled[r, v] = np.where(win, m[first, np.arange(c)], F32(0))
            else:
                s = np.zeros(c, F32)
                for k in range(vals.shape[0]):
                    s = s + vals[k]
                pooled[r, v] = s / F32(vals.shape[0])
    shp = (n,) + tuple(out_size)
    return (pooled.reshape(shp + (c,)), argmax.reshape(shp + (c,)) if mode == 0 else None, pt_cell,
            vox_cnt.reshape(shp))


def pool_bwd(grad_out, argmax, pt_cell, vox_cnt, mode):
    """grad_in (P, C): from 0.0f, RoI r = 0, 1, ... adds its contribution to each point it keeps."""
    g = np.asarray(grad_out, F32)
    n, c = g.shape[0], g.shape[-1]
    g = g.reshape(n, -1, c)
    am = None if argmax is None else np.asarray(argmax).reshape(n, -1, c)
    cnt = np.asarray(vox_cnt).reshape(n, -1)
    npt = pt_cell.shape[1]
    grad_in = np.zeros((npt, c), F32)
    for r in range(n):
        p = np.nonzero(pt_cell[r] >= 0)[0]
        if p.size == 0:
            continue
        v = pt_cell[r, p]
        if mode == 0:
            add = np.where(am[r, v] == p[:, None], g[r, v], F32(0))
        else:
            scale = F32(1) / np.maximum(cnt[r, v].astype(F32), F32(1))
            add = g[r, v] * scale[:, None]
        grad_in[p] = grad_in[p] + add
    return grad_in
