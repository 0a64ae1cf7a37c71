"""float32 numpy restatement of the point-head target assignment (include/spx.h §16, csrc/point_targets.hip): the three
labelling modes, the first-hit box index, the box / centre rows, the PointBinResidualCoder code and the centerness.
The inside test is roiaware_ref.in_box.  Every rounding step is spelled out: float32 operations round after each
operation (numpy float32 arithmetic never contracts), constants are the float32 roundings of the Python doubles, and
the three log columns are the correctly rounded float32 of a float64 log (what a float32 logf is compared against)."""
import numpy as np

import roiaware_ref as rr

F32, F64 = np.float32, np.float64
PLAIN, IGNORE_RING, BALL = 0, 1, 2
MIN_SIZE = F32(1e-5)
EPS = F32(1e-6)


def floor_rem(a, b):
    """torch.remainder of float32 by the float32 scalar b as the CPU kernel takes it: fmod (exact), then + b when the
    result is non-zero and its sign differs from b's."""
    a, b = np.asarray(a, F32), F32(b)
    m = np.fmod(a, b)
    return np.where((m != 0) & ((b < 0) != (m < 0)), m + b, m).astype(F32)


def bin_consts(bins):
    two_pi = np.pi * 2.0
    apc = two_pi / float(bins)
    return F32(two_pi), F32(apc), F32(apc / 2.0)


def encode(boxes, pts, bins):
    """boxes (R, 7), pts (R, 3) -> (R, 6 + 2 * bins): PointBinResidualCoder.encode_torch with use_mean_size False."""
    g, p = np.asarray(boxes, F32), np.asarray(pts, F32)
    r = g.shape[0]
    out = np.zeros((r, 6 + 2 * bins), F32)
    out[:, 0:3] = g[:, 0:3] - p
    size = np.where(g[:, 3:6] < MIN_SIZE, MIN_SIZE, g[:, 3:6])
    out[:, 3:6] = np.log(size.astype(F64)).astype(F32)
    two_pi, apc, half = bin_consts(bins)
    angle = floor_rem(g[:, 6], two_pi)
    shifted = floor_rem(angle + half, two_pi)
    cf = np.floor(shifted / apc)
    res = (shifted - (cf * apc + half)) / apc
    k = np.arange(bins, dtype=F32)[None, :]
    at_bin = k == cf[:, None]
    out[:, 6:6 + bins] = at_bin.astype(F32)
    out[:, 6 + bins:] = np.where(at_bin, res[:, None], F32(0) * res[:, None])
    return out


def centerness(boxes, pts, dtype=F32):
    """generate_centerness_label of rows: boxes (R, 7), pts (R, 3) -> (R).  dtype float64 gives the evaluation the GPU
    result is compared with (the float32 inputs are exact in it)."""
    g, p = np.asarray(boxes, F32).astype(dtype), np.asarray(pts, F32).astype(dtype)
    c = p - g[:, 0:3]
    ca, sa = np.cos(-g[:, 6]), np.sin(-g[:, 6])
    rx = c[:, 0] * ca + c[:, 1] * (-sa)
    ry = c[:, 0] * sa + c[:, 1] * ca
    two = dtype(2)
    with np.errstate(invalid="ignore", divide="ignore"):
        prod = None
        for d, v in ((g[:, 3], rx), (g[:, 4], ry), (g[:, 5], c[:, 2])):
            lo, hi = d / two - v, d / two + v
            ratio = np.minimum(lo, hi) / np.maximum(lo, hi)
            prod = ratio if prod is None else prod * ratio
        prod = np.where(prod < dtype(EPS), dtype(EPS), prod)
        return np.power(prod, dtype(1) / dtype(3) if dtype is F64 else F32(1.0 / 3.0)).astype(dtype)


def grow(boxes7, extra_width):
    g = np.array(boxes7, F32, copy=True)
    g[..., 3:6] = g[..., 3:6] + np.asarray(extra_width, F32)
    return g


def first_hit(inside):
    """inside (M, P) bool -> (P) int32: the first box holding each point, else -1."""
    if inside.shape[0] == 0:
        return np.full(inside.shape[1], -1, np.int32)
    return np.where(inside.any(axis=0), inside.argmax(axis=0), -1).astype(np.int32)


def assign(points, gt_boxes, mode, extra_width=(0.0, 0.0, 0.0), central_radius=0.0, num_class=1, bins=0):
    """points (B, N, 3), gt_boxes (B, M, >= 8) -> dict over the B * N points: cls_labels int64, box_idx int32,
    box_labels (., 7), center_labels (., 3), reg_labels (., 6 + 2 * bins) (bins > 0), centerness (.) float32, and fg
    (.) bool, the points whose label is > 0."""
    points, gt_boxes = np.asarray(points, F32), np.asarray(gt_boxes, F32)
    b, n = points.shape[:2]
    cls = np.zeros((b, n), np.int64)
    idx = np.full((b, n), -1, np.int32)
    box = np.zeros((b, n, 7), F32)
    reg = np.zeros((b, n, 6 + 2 * bins), F32) if bins > 0 else None
    ctr = np.zeros((b, n), F32)
    radius = F32(central_radius)
    for f in range(b):
        p, g = points[f], gt_boxes[f]
        grown_boxes = grow(g[:, :7], extra_width)
        if mode == PLAIN:
            hit = first_hit(rr.in_box(p, grown_boxes)[0])
        else:
            hit = first_hit(rr.in_box(p, g[:, :7])[0])
        idx[f] = hit
        has = hit >= 0
        hb = g[np.where(has, hit, 0)] if g.shape[0] else np.zeros((n, gt_boxes.shape[2]), F32)
        klass = np.ones(n, np.int64) if num_class == 1 else np.trunc(hb[:, 7]).astype(np.int64)
        label = np.where(has, klass, 0)
        if mode == IGNORE_RING:
            any_grown = rr.in_box(p, grown_boxes)[0].any(axis=0) if g.shape[0] else np.zeros(n, bool)
            label = np.where(has, klass, np.where(any_grown, -1, 0))
        elif mode == BALL:
            e = hb[:, 0:3] - p
            dist = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
            label = np.where(has, np.where(dist < radius, klass, -1), 0)
        cls[f] = label
        fg = label > 0
        box[f, fg] = hb[fg, :7]
        if bins > 0:
            reg[f, fg] = encode(hb[fg, :7], p[fg], bins)
        ctr[f, fg] = centerness(hb[fg, :7], p[fg])
    out = {"cls_labels": cls.reshape(-1), "box_idx": idx.reshape(-1), "box_labels": box.reshape(-1, 7),
           "center_labels": np.ascontiguousarray(box[:, :, 0:3]).reshape(-1, 3), "centerness": ctr.reshape(-1),
           "fg": (cls > 0).reshape(-1)}
    if bins > 0:
        out["reg_labels"] = reg.reshape(b * n, -1)
    return out


def ulp_distance(a, b):
    """Distance in float32 units in the last place between two arrays of finite float32 values."""
    def ordered(x):
        i = np.asarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ------------------------------------------------------------------------------------------------- shared test inputs

def make_case(m, ld=8, b=3, n=300, seed=0):
    """The inputs of the GPU tests and of the CPU composition test: points (b, n, 3), gt_boxes (b, m, ld) float32 and
    loc, a dict of the rows placed on purpose.  For m >= 5 every frame holds: two overlapping boxes (0 and 1, the same
    centre, box 1 smaller, so the first-hit order decides), headings across (-4 pi, 4 pi), a box with dx below 1e-5
    (box 2), and box m - 1 zero-padded (all-zero row, class 0).  Points: most are drawn in box-local coordinates at
    <= 0.9 of a half-size of a box (rows loc["local"], each drawn in box loc["local_box"]: the centerness set comes from
    them), some in the grown-only ring, some far away; point 0 is the origin, point 1 lies on the top z face of box 0,
    point 2 at the centre of the thin box."""
    rng = np.random.default_rng(1000 * m + 10 * ld + seed)
    gt = np.zeros((b, m, ld), F32)
    pts = (rng.uniform(-40, 40, size=(b, n, 3)) * np.array([1, 1, 0.05])).astype(F32)
    loc = {"origin": 0, "z_face": 1, "thin": 2, "local": [], "local_box": []}
    for f in range(b):
        real = m - 1 if m >= 5 else m
        for k in range(real):
            gt[f, k, 0:3] = rng.uniform(-30, 30, 3) * np.array([1, 1, 0.03])
            gt[f, k, 3:6] = rng.uniform(1.0, 5.0, 3)
            gt[f, k, 6] = rng.uniform(-4 * np.pi, 4 * np.pi)
            gt[f, k, 7] = 1 + rng.integers(0, 3)
            if ld > 8:
                gt[f, k, 8:] = rng.normal(size=ld - 8)
        if m >= 1:
            gt[f, 0, 2], gt[f, 0, 5] = 0.5, 2.0             # the top face is at z = 1.5 exactly
        if m >= 5:
            gt[f, 1, 0:3] = gt[f, 0, 0:3]
            gt[f, 1, 3:6] = gt[f, 0, 3:6] * F32(0.6)
            gt[f, 1, 6] = gt[f, 0, 6] + F32(0.3)
            gt[f, 1, 7] = 1 + (int(gt[f, 0, 7]) % 3)
            gt[f, 2, 3] = 5e-6
        pts[f, 0] = 0.0
        if m >= 1:
            pts[f, 1] = gt[f, 0, 0:3] + np.array([0, 0, gt[f, 0, 5] / F32(2)], F32)
        if m >= 5:
            pts[f, 2] = gt[f, 2, 0:3]
        if real == 0:
            continue
        # box-local points: |local| <= 0.9 * half-size of a box; then ring points at 1.0 .. 1.4 of the half-size
        for j in range(3, n):
            u = rng.random()
            if u > 0.75:
                continue
            k = int(rng.integers(0, min(real, 8)))
            c, d, rz = gt[f, k, 0:3].astype(F64), gt[f, k, 3:6].astype(F64), float(gt[f, k, 6])
            if u < 0.55:
                local = rng.uniform(-0.9, 0.9, 3) * d / 2
                loc["local"].append(f * n + j)
                loc["local_box"].append(k)
            else:
                local = rng.uniform(-1.0, 1.0, 3) * d / 2
                ax = int(rng.integers(0, 2))
                local[ax] = np.sign(local[ax] or 1.0) * rng.uniform(1.02, 1.4) * d[ax] / 2
            ca, sa = np.cos(rz), np.sin(rz)
            pts[f, j] = (c + np.array([local[0] * ca - local[1] * sa, local[0] * sa + local[1] * ca, local[2]])).astype(F32)
    loc["local"] = np.asarray(loc["local"], np.int64)
    loc["local_box"] = np.asarray(loc["local_box"], np.int32)
    return pts, gt, loc


CASES = [(0, 8), (1, 8), (5, 10), (300, 8)]          # (m, ld): no box, one box, the placed rows, a second LDS chunk
EXTRA_WIDTH = (0.5, 0.5, 0.3)
RADIUS = 1.2                                          # below the half-diagonal of most boxes: the ball cuts corners off


def face_distances(boxes, pts):
    """float64 distances of pts (R, 3) to the six faces of their boxes (R, 7) -> (R, 6)."""
    g, p = np.asarray(boxes, F32).astype(F64), np.asarray(pts, F32).astype(F64)
    c = p - g[:, 0:3]
    ca, sa = np.cos(-g[:, 6]), np.sin(-g[:, 6])
    local = np.stack([c[:, 0] * ca - c[:, 1] * sa, c[:, 0] * sa + c[:, 1] * ca, c[:, 2]], axis=1)
    return np.concatenate([g[:, 3:6] / 2 - local, g[:, 3:6] / 2 + local], axis=1)


def centerness_rows(points, loc, res):
    """The rows on which centerness is compared with the float64 evaluation: foreground rows of loc["local"] that were
    assigned the box they were drawn in, when that box has half-sizes >= 0.5 m.  They were drawn at <= 0.9 of each
    half-size, so every face is >= 0.05 m away; returns (rows, the smallest face distance) for the test to assert it."""
    rows = loc["local"]
    rows = rows[res["fg"][rows] & (res["box_idx"][rows] == loc["local_box"])]
    rows = rows[res["box_labels"][rows, 3:6].min(axis=1) / 2 >= 0.5]
    if rows.size == 0:
        return rows, np.inf
    return rows, face_distances(res["box_labels"][rows], np.asarray(points, F32).reshape(-1, 3)[rows]).min()
