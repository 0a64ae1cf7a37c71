"""numpy restatement of the reference's roipoint_pool3d (roipoint_pool3d_kernel.cu behind roipoint_pool3d_utils.py) and,
in canonical form, of PointRCNNHead.roipool3d_gpu: what a HIP op for it has to reproduce.

Semantics:
  * the box is grown to (dx + wx, dy + wy, dz + wz), float32 adds (enlarge_box3d runs in float32 before the reference's
    kernel sees the box); centre and heading unchanged;
  * the inside test is check_pt_in_box3d, restated in roiaware_ref.in_box at the GPU margin: the z test and the 1e-5
    margin compare in float64, |z - cz| == dz / 2 is inside, x / y are strict against d / 2 + 1e-5;
  * per (frame, box) the first min(cnt, S) inside points in ascending point index fill the first slots; with
    0 < cnt < S slot k >= cnt repeats slot k % cnt;
  * cnt == 0: flag 1 and a block of zeros; otherwise flag 0;
  * an all-zero RoI is an ordinary box of zero size.
Plain rows are [x, y, z, features], bit copies.  Canonical rows are [x', y', z', score, depth, features], with the point
minus the RoI centre rotated by -heading about z and depth = |p| / depth_normalizer - 0.5; `canonical` evaluates the four
computed columns in float64 from the float32 inputs (the yardstick for a float32 implementation)."""
import numpy as np

import roiaware_ref

F32, F64 = np.float32, np.float64


def _widths(extra_width):
    w = np.asarray(extra_width, F32).reshape(-1)
    return np.broadcast_to(w, (3,)) if w.size == 1 else w


def grow(boxes3d, extra_width):
    """(…, >= 7) float32 -> (…, 7) float32 with the three sizes grown by float32 adds."""
    b = np.array(np.asarray(boxes3d, F32)[..., :7], F32)
    b[..., 3:6] = b[..., 3:6] + _widths(extra_width)
    return b


def pooled_indices(points, boxes3d, extra_width, s):
    """points (B, N, 3), boxes3d (B, M, >= 7) -> idx (B, M, S) int64 (-1 in every slot of an empty RoI), cnt (B, M) int64
    (the number of inside points, not capped)."""
    points = np.asarray(points, F32)
    boxes = grow(boxes3d, extra_width)
    b, m = boxes.shape[:2]
    idx = np.full((b, m, s), -1, np.int64)
    cnt = np.zeros((b, m), np.int64)
    for i in range(b):
        inside = roiaware_ref.in_box(points[i], boxes[i])[0] if points.shape[1] else np.zeros((m, 0), bool)
        for j in range(m):
            first = np.nonzero(inside[j])[0]
            cnt[i, j] = first.size
            if first.size:
                first = first[:s]
                idx[i, j] = first[np.arange(s) % first.size]
    return idx, cnt


def roipoint_pool3d(points, point_features, boxes3d, extra_width, s):
    """-> pooled_features (B, M, S, 3 + C) float32, pooled_empty_flag (B, M) int32."""
    points, feats = np.asarray(points, F32), np.asarray(point_features, F32)
    idx, cnt = pooled_indices(points, boxes3d, extra_width, s)
    b, m = idx.shape[:2]
    out = np.zeros((b, m, s, 3 + feats.shape[2]), F32)
    for i in range(b):
        live = cnt[i] > 0
        out[i, live] = np.concatenate([points[i][idx[i, live]], feats[i][idx[i, live]]], axis=-1)
    return out, (cnt == 0).astype(np.int32)


def canonical(points, point_features, point_scores, boxes3d, extra_width, s, depth_normalizer):
    """-> pooled (B * M, S, 5 + C) float64: the feature and score columns hold float32 values exactly, the xyz and depth
    columns are the float64 evaluation; flag (B, M) int32."""
    points, feats = np.asarray(points, F32), np.asarray(point_features, F32)
    scores = np.asarray(point_scores, F32).reshape(points.shape[:2])
    boxes = np.asarray(boxes3d, F32)
    idx, cnt = pooled_indices(points, boxes, extra_width, s)
    b, m = idx.shape[:2]
    out = np.zeros((b, m, s, 5 + feats.shape[2]), F64)
    for i in range(b):
        for j in range(m):
            if cnt[i, j] == 0:
                continue
            p = points[i][idx[i, j]].astype(F64)                       # (S, 3)
            d = p - boxes[i, j, :3].astype(F64)
            a = -F64(boxes[i, j, 6])
            ca, sa = np.cos(a), np.sin(a)
            out[i, j, :, 0] = d[:, 0] * ca - d[:, 1] * sa
            out[i, j, :, 1] = d[:, 0] * sa + d[:, 1] * ca
            out[i, j, :, 2] = d[:, 2]
            out[i, j, :, 3] = scores[i][idx[i, j]]
            out[i, j, :, 4] = np.sqrt((p * p).sum(axis=1)) / F64(depth_normalizer) - 0.5
            out[i, j, :, 5:] = feats[i][idx[i, j]]
    return out.reshape(b * m, s, -1), (cnt == 0).astype(np.int32)


def brute_force(points, point_features, boxes3d, extra_width, s):
    """The same result by plain loops written from the semantics, one point and one box at a time, with its own inside
    test (no code shared with the functions above)."""
    points, feats, boxes = np.asarray(points, F32), np.asarray(point_features, F32), np.asarray(boxes3d, F32)
    w = _widths(extra_width)
    b, n = points.shape[:2]
    m, c = boxes.shape[1], feats.shape[2]
    out = np.zeros((b, m, s, 3 + c), F32)
    flag = np.zeros((b, m), np.int32)
    margin = F64(F32(1e-5))
    for i in range(b):
        for j in range(m):
            cx, cy, cz, dx, dy, dz, rz = boxes[i, j, :7]
            dx, dy, dz = F32(dx + w[0]), F32(dy + w[1]), F32(dz + w[2])
            cosa, sina = F32(np.cos(-F64(rz))), F32(np.sin(-F64(rz)))
            chosen = []
            for k in range(n):
                if len(chosen) == s:
                    break
                x, y, z = points[i, k]
                if F64(abs(F32(z - cz))) > F64(dz) / 2.0:
                    continue
                sx, sy = F32(x - cx), F32(y - cy)
                lx = F32(F32(sx * cosa) + F32(sy * F32(-sina)))
                ly = F32(F32(sx * sina) + F32(sy * cosa))
                if F64(abs(lx)) < F64(dx) / 2.0 + margin and F64(abs(ly)) < F64(dy) / 2.0 + margin:
                    chosen.append(k)
            if not chosen:
                flag[i, j] = 1
                continue
            for k in range(s):
                src = chosen[k % len(chosen)]
                out[i, j, k, :3] = points[i, src]
                out[i, j, k, 3:] = feats[i, src]
    return out, flag
