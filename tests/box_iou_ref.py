"""Plain float64 references for the rotated-BEV pair test (csrc/box_iou.h) and for every NMS built on it.

Two references of the same quantity, on purpose:

  overlap_ref / iou_ref   a float64 restatement of box_iou.h's ALGORITHM, quirks included: edge/edge crossings with
                          strict straddle tests, corners of one box inside the other with the 1e-2 margin, the kEps
                          branch of the crossing point and its move onto the shared rectangle, a stable ascending angle sort about the centroid, the shoelace
                          sum from vertex 0, (earlier, later) argument order, IoU = so / max(sa + sb - so, kEps)
                          clamped to 1.  Inputs are the fp32 boxes promoted to float64, so what the HIP kernel is
                          compared with differs from it only by fp32 rounding - except where a corner sits on the
                          margin boundary (below).
  clip_area               exact convex clipping (Sutherland-Hodgman) in float64: no margin, no quirks, the geometric
                          truth.  The two agree wherever no corner lies in the margin band.

margin_clearance: per pair, the smallest distance from zero of any corner's |rx| - (dx/2 + 1e-2) or |ry| - (dy/2 + 1e-2).
That predicate is the only one whose flip changes the area discontinuously (a flipped strict crossing only adds or drops
a vertex that coincides with an included corner), so a pair is *margin-stable* when its clearance exceeds
STABLE_CLEARANCE, and only margin-stable pairs are compared by value.  Each family states the share of pairs it may leave
out as unstable (UNSTABLE_CAP): a condition on the inputs, met by the reference alone.

numpy only; `clustered` replays the draw of tests/test_gpu_kernels.py::test_boxes_iou_bev_vs_oracle, which needs torch's
generator, and imports torch for that alone."""
import numpy as np

K_EPS = float(np.float32(1e-8))
K_MARGIN = float(np.float32(1e-2))
STABLE_CLEARANCE = 1e-4

# GPU tolerance per family: TOL[f] = max(4 * E_f, 1e-6), E_f = max |fp32 C oracle - float64 reference| over the family's
# margin-stable pairs, measured on the host (tests/test_box_iou_ref.py::test_oracle_fp32_error_fits_tol, run recorded in
# profiles/box_iou_accuracy.log).  The factor 4 covers what the host run cannot see: device sinf / cosf / atan2f an ulp
# or two from libm, FMA contraction in the cross products.  "iou" bounds IoUs, "overlap" bounds areas (m^2).
TOL = {
    "clustered":         {"iou": 1.4e-05, "overlap": 5.4e-05},   # E_f 3.35e-06, 1.35e-05
    "identical":         {"iou": 7.0e-05, "overlap": 1.2e-04},   # E_f 1.75e-05, 2.88e-05   (above today's 2e-5)
    "near_identical":    {"iou": 1.0e-06, "overlap": 6.0e-05},   # E_f 0.00e+00, 1.50e-05   (every IoU is capped at 1)
    "grid_axis":         {"iou": 1.0e-06, "overlap": 1.0e-06},   # E_f 2.97e-08, 0.00e+00
    "grid_axis_rotated": {"iou": 2.4e-06, "overlap": 3.6e-06},   # E_f 5.96e-07, 8.99e-07   (worst of the five angles)
    "octagon":           {"iou": 2.3e-05, "overlap": 8.4e-05},   # E_f 5.59e-06, 2.08e-05   (above today's 2e-5)
    "wrapped_heading":   {"iou": 1.6e-05, "overlap": 5.4e-05},   # E_f 3.79e-06, 1.35e-05
    "far":               {"iou": 1.9e-04, "overlap": 4.2e-04},   # E_f 4.74e-05, 1.03e-04   (half an ulp of 150 m is 7.6e-6)
    "thin":              {"iou": 2.6e-05, "overlap": 3.9e-05},   # E_f 6.45e-06, 9.55e-06   (above today's 2e-5)
    "sub_margin":        {"iou": 1.5e-02, "overlap": 1.0e-06},   # E_f 3.52e-03, 6.52e-10   (unions down to kEps)
}

# share of pairs a family may leave out as margin-unstable
UNSTABLE_CAP = {"clustered": 0.02, "identical": 0.0, "near_identical": 0.02, "grid_axis": 0.0, "grid_axis_rotated": 0.0,
                "octagon": 0.0, "wrapped_heading": 0.02, "far": 0.02, "thin": 0.02, "sub_margin": 0.02}


def family_key(name):
    """Key of TOL / UNSTABLE_CAP / CLOSED_FORM_INPUT_ERR: the five grid_axis_rotated_<angle> families share one entry."""
    return "grid_axis_rotated" if name.startswith("grid_axis_rotated") else name


# ------------------------------------------------------------------------------------------- the restated algorithm
def _corners(b):
    """(P, 7) -> (P, 5, 2): the four corners in box_iou.h's order, the first repeated."""
    hx, hy = b[:, 3] / 2, b[:, 4] / 2
    ca, sa = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    px = b[:, 0:1] + np.stack([-hx, hx, hx, -hx], 1)
    py = b[:, 1:2] + np.stack([-hy, -hy, hy, hy], 1)
    x = (px - b[:, 0:1]) * ca + (py - b[:, 1:2]) * (-sa) + b[:, 0:1]
    y = (px - b[:, 0:1]) * sa + (py - b[:, 1:2]) * ca + b[:, 1:2]
    c = np.stack([x, y], 2)
    return np.concatenate([c, c[:, :1]], 1)


def _cross3(p1, p2, p0):
    return (p1[:, 0] - p0[:, 0]) * (p2[:, 1] - p0[:, 1]) - (p2[:, 0] - p0[:, 0]) * (p1[:, 1] - p0[:, 1])


def _in_box(box, p):
    """-> (inside (P) bool, clearance (P)): the margin test of one corner per pair."""
    ca, sa = np.cos(-box[:, 6]), np.sin(-box[:, 6])
    rx = (p[:, 0] - box[:, 0]) * ca + (p[:, 1] - box[:, 1]) * (-sa)
    ry = (p[:, 0] - box[:, 0]) * sa + (p[:, 1] - box[:, 1]) * ca
    vx = np.abs(rx) - (box[:, 3] / 2 + K_MARGIN)
    vy = np.abs(ry) - (box[:, 4] / 2 + K_MARGIN)
    inside = (vx < 0) & (vy < 0)
    # how far the pair (vx, vy) is from the other verdict: an inside corner leaves when either value reaches zero, an
    # outside one enters only when every positive value has come down to zero
    return inside, np.where(inside, np.minimum(-vx, -vy), np.maximum(vx, vy))


def _seg_cross(p1, p0, q1, q0):
    """-> (crosses (P) bool, point (P, 2)): strict straddling, the kEps branch for the point."""
    lo, hi = np.minimum, np.maximum
    bbox = (lo(p0[:, 0], p1[:, 0]) <= hi(q0[:, 0], q1[:, 0])) & (lo(q0[:, 0], q1[:, 0]) <= hi(p0[:, 0], p1[:, 0])) & \
           (lo(p0[:, 1], p1[:, 1]) <= hi(q0[:, 1], q1[:, 1])) & (lo(q0[:, 1], q1[:, 1]) <= hi(p0[:, 1], p1[:, 1]))
    s1, s2 = _cross3(q0, p1, p0), _cross3(p1, q1, p0)
    s3, s4 = _cross3(p0, q1, q0), _cross3(q1, p1, q0)
    ok = bbox & (s1 * s2 > 0) & (s3 * s4 > 0)
    s5 = _cross3(q1, p1, p0)
    with np.errstate(divide="ignore", invalid="ignore"):
        main = np.stack([(s5 * q0[:, 0] - s1 * q1[:, 0]) / (s5 - s1), (s5 * q0[:, 1] - s1 * q1[:, 1]) / (s5 - s1)], 1)
        t = np.fmin(np.fmax(s1 / (s1 - s5), 0.0), 1.0)           # kEps branch: on q by construction; NaN -> 0
        alt = np.stack([q0[:, 0] + t * (q1[:, 0] - q0[:, 0]), q0[:, 1] + t * (q1[:, 1] - q0[:, 1])], 1)
    pt = np.where((np.abs(s5 - s1) > K_EPS)[:, None], main, alt)
    # onto the rectangle both segments' bounding boxes share (not empty: bbox holds); NaN goes to its lower end
    for k in (0, 1):
        low, high = hi(lo(p0[:, k], p1[:, k]), lo(q0[:, k], q1[:, k])), lo(hi(p0[:, k], p1[:, k]), hi(q0[:, k], q1[:, k]))
        pt[:, k] = np.fmin(np.fmax(pt[:, k], low), high)
    return ok, pt


def _overlap_pairs(a, b):
    """a, b (P, 7) float64, pair p = (a[p], b[p]) -> (area (P), clearance (P), vertex count (P))."""
    n = a.shape[0]
    ca, cb = _corners(a), _corners(b)
    pts = np.zeros((n, 24, 2))
    valid = np.zeros((n, 24), dtype=bool)
    for i in range(4):
        for j in range(4):
            valid[:, i * 4 + j], pts[:, i * 4 + j] = _seg_cross(ca[:, i + 1], ca[:, i], cb[:, j + 1], cb[:, j])
    clear = np.full(n, np.inf)
    for k in range(4):
        for slot, box, p in ((16 + 2 * k, a, cb[:, k]), (17 + 2 * k, b, ca[:, k])):
            valid[:, slot], c = _in_box(box, p)
            pts[:, slot] = p
            clear = np.minimum(clear, c)
    cnt = valid.sum(1)
    pts = np.where(valid[:, :, None], pts, 0.0)
    centre = pts.sum(1) / np.maximum(cnt, 1)[:, None]
    ang = np.where(valid, np.arctan2(pts[:, :, 1] - centre[:, None, 1], pts[:, :, 0] - centre[:, None, 0]), np.inf)
    order = np.argsort(ang, axis=1, kind="stable")       # the bubble sort with `>` is a stable ascending sort
    pts = np.take_along_axis(pts, order[:, :, None], 1)
    live = np.take_along_axis(valid, order, 1)
    rel = np.where(live[:, :, None], pts - pts[:, :1], 0.0)            # slots past cnt count as vertex 0: no area
    area = (rel[:, :-1, 0] * rel[:, 1:, 1] - rel[:, :-1, 1] * rel[:, 1:, 0]).sum(1)
    return np.where(cnt > 0, np.abs(area) / 2.0, 0.0), clear, cnt


def _all_pairs(a, b, chunk=1 << 16):
    """Every pair of a x b.  Pairs whose circumscribed circles are more than 0.05 apart skip the polygon: no bounding boxes
    meet and no corner is inside, so the kernel counts no vertex and returns 0; every corner is then outside the other's
    margin box by the gap less the margin's corner, which (over sqrt 2, as a bound on the larger coordinate) is the
    clearance reported for them: above 2e-2."""
    a, b = np.asarray(a, np.float64)[:, :7], np.asarray(b, np.float64)[:, :7]
    n, m = a.shape[0], b.shape[0]
    gap = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]) \
        - (np.hypot(a[:, 3], a[:, 4]) / 2)[:, None] - (np.hypot(b[:, 3], b[:, 4]) / 2)[None]
    area, cnt = np.zeros(n * m), np.zeros(n * m, np.int64)
    clear = ((gap - np.sqrt(2) * K_MARGIN) / np.sqrt(2)).reshape(-1)
    near = np.nonzero(gap.reshape(-1) <= 0.05)[0]
    for lo in range(0, len(near), chunk):
        t = near[lo:lo + chunk]
        area[t], clear[t], cnt[t] = _overlap_pairs(a[t // m], b[t % m])
    return area.reshape(n, m), clear.reshape(n, m), cnt.reshape(n, m)


def overlap_ref(a, b):
    """a (n, 7), b (m, 7) -> (intersection area (n, m) float64, margin_clearance (n, m)); [i, j] = (a[i], b[j])."""
    area, clear, _ = _all_pairs(a, b)
    return area, clear


def vertex_count_ref(a, b):
    """(n, m) number of polygon vertices the algorithm collects (at most 16: pts[16] in box_iou.h)."""
    return _all_pairs(a, b)[2]


def iou_ref(a, b, overlap_only=False):
    """-> (IoU or intersection area (n, m) float64, margin_clearance (n, m))."""
    area, clear = overlap_ref(a, b)
    if overlap_only:
        return area, clear
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sa, sb = (a[:, 3] * a[:, 4])[:, None], (b[:, 3] * b[:, 4])[None]
    return np.minimum(area / np.maximum(sa + sb - area, K_EPS), 1.0), clear


def stable(clearance):
    return clearance > STABLE_CLEARANCE


# ------------------------------------------------------------------------------------------------ geometric truth
def _clip_one(subject, clip):
    """Sutherland-Hodgman: subject polygon (list of points) clipped by a convex counter-clockwise polygon."""
    out = subject
    for k in range(len(clip)):
        e0, e1 = clip[k], clip[(k + 1) % len(clip)]
        side = lambda p: (e1[0] - e0[0]) * (p[1] - e0[1]) - (e1[1] - e0[1]) * (p[0] - e0[0])   # noqa: E731
        src, out = out, []
        for i in range(len(src)):
            p, q = src[i], src[(i + 1) % len(src)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if not out:
            return []
    return out


def _ccw_corners(b):
    hx, hy, c, s = b[3] / 2, b[4] / 2, np.cos(b[6]), np.sin(b[6])
    return [(b[0] + ox * c - oy * s, b[1] + ox * s + oy * c) for ox, oy in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]


def clip_area(a, b):
    """(n, 7), (m, 7) -> (n, m) exact intersection areas in float64; pairs too far apart to touch are 0 without clipping."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((a.shape[0], b.shape[0]))
    ra, rb = np.hypot(a[:, 3], a[:, 4]) / 2, np.hypot(b[:, 3], b[:, 4]) / 2
    dist = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    for i, j in zip(*np.nonzero(dist <= ra[:, None] + rb[None])):
        poly = _clip_one(_ccw_corners(a[i]), _ccw_corners(b[j]))
        if len(poly) >= 3:
            x, y = np.array([p[0] for p in poly]), np.array([p[1] for p in poly])
            out[i, j] = abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))) / 2
    return out


# --------------------------------------------------------------------------------------- axis-aligned and 3-D twins
def iou_normal_ref(a, b):
    """float64 twin of box_iou.h's iou_normal (heading ignored)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    lo = lambda k, s: np.maximum((a[:, k] - a[:, s] / 2)[:, None], (b[:, k] - b[:, s] / 2)[None])   # noqa: E731
    hi = lambda k, s: np.minimum((a[:, k] + a[:, s] / 2)[:, None], (b[:, k] + b[:, s] / 2)[None])   # noqa: E731
    inter = np.maximum(hi(0, 3) - lo(0, 3), 0) * np.maximum(hi(1, 4) - lo(1, 4), 0)
    return inter / np.maximum((a[:, 3] * a[:, 4])[:, None] + (b[:, 3] * b[:, 4])[None] - inter, K_EPS)


def axis_overlap(a, b):
    """Closed-form intersection area w * h of heading-0 boxes."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = np.minimum((a[:, 0] + a[:, 3] / 2)[:, None], (b[:, 0] + b[:, 3] / 2)[None]) - \
        np.maximum((a[:, 0] - a[:, 3] / 2)[:, None], (b[:, 0] - b[:, 3] / 2)[None])
    h = np.minimum((a[:, 1] + a[:, 4] / 2)[:, None], (b[:, 1] + b[:, 4] / 2)[None]) - \
        np.maximum((a[:, 1] - a[:, 4] / 2)[:, None], (b[:, 1] - b[:, 4] / 2)[None])
    return np.maximum(w, 0) * np.maximum(h, 0)


def iou3d_ref(a, b):
    """float64 twin of iou3d_nms_utils.boxes_iou3d_gpu -> (3-D IoU (n, m), margin_clearance (n, m))."""
    area, clear = overlap_ref(a, b)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    top = np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None])
    bot = np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None])
    o3 = area * np.maximum(top - bot, 0)
    va, vb = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None]
    return o3 / np.maximum(va + vb - o3, 1e-6), clear


# ------------------------------------------------------------------------------------------------------- greedy NMS
def greedy_ref(iou, thresh):
    """iou (n, n) read as [earlier, later], rows in score order -> kept positions: a kept box removes every later box
    whose IoU with it is strictly above thresh; a removed box removes nothing."""
    n = iou.shape[0]
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= iou[i, i + 1:] > thresh
    return np.asarray(keep, dtype=np.int64)


def gap_threshold(iou, lo, hi):
    """-> (threshold, half gap): the midpoint of the widest gap between the sorted IoUs of the pairs (earlier, later) that
    lie in [lo, hi], lo and hi closing the ends.  No IoU of the matrix is nearer to the threshold than the half gap."""
    v = iou[np.triu_indices(iou.shape[0], 1)]
    v = np.unique(np.concatenate([[lo, hi], v[(v >= lo) & (v <= hi)]]))
    k = int(np.argmax(np.diff(v)))
    return float((v[k] + v[k + 1]) / 2), float((v[k + 1] - v[k]) / 2)


# --------------------------------------------------------------------------------------------------------- families
def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _box(xy, dims, heading):
    n = len(heading)
    return np.concatenate([np.asarray(xy, np.float64).reshape(n, 2), np.zeros((n, 1)),
                           np.asarray(dims, np.float64).reshape(n, 2), np.full((n, 1), 1.5),
                           np.asarray(heading, np.float64).reshape(n, 1)], 1)


def _clustered64():
    """The draw of test_boxes_iou_bev_vs_oracle (torch generator, seed 21), cut to 256 x 256."""
    import torch
    g = torch.Generator().manual_seed(21)
    n = 300
    centres = torch.rand(max(n // 40, 1), 2, generator=g) * 30.0
    xy = centres[torch.randint(0, centres.shape[0], (n,), generator=g)] + torch.randn(n, 2, generator=g) * 0.7
    dims = torch.rand(n, 2, generator=g) * torch.tensor([3.5, 1.5]) + torch.tensor([0.6, 0.5])
    a = torch.cat([xy, torch.zeros(n, 1), dims, torch.ones(n, 1) * 1.5, (torch.rand(n, 1, generator=g) - 0.5) * 6.3], 1)
    b = a[:257].clone()
    b[:, :2] += torch.randn(257, 2, generator=g) * 0.8
    b[:, 6] += torch.randn(257, generator=g)
    return a[:256].numpy(), b[:256].numpy()


def clustered():
    return _clustered64()


def _spread(n, gap=8.0):
    """n centres `gap` apart on a square lattice about the origin: boxes with diagonals under gap - 0.1 reach only their
    own partner."""
    k = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    return np.stack([(i % k - k // 2) * gap, (i // k - k // 2) * gap], 1)


def _exact(boxes):
    """float64 boxes that fp32 holds exactly."""
    return _f32(boxes).astype(np.float64)


def _identical64():
    rng = np.random.default_rng(101)
    n = 192
    dims = rng.uniform([0.6, 0.5], [4.1, 2.0], (n, 2))
    dims[128:, 1] = dims[128:, 0]
    a = _exact(_box(_spread(n), dims, rng.uniform(-3.1, 3.1, n)))
    b = a.copy()
    b[64:128, 6] += np.pi
    b[128:, 6] += np.pi / 2
    return a, b


def identical():
    """b[i] is a[i] again (i < 64), a[i] turned by pi (64 <= i < 128) and, for squares, by pi / 2 (i >= 128); other pairs
    are out of reach of each other.  a is exact in fp32; the turned headings of b are rounded."""
    a, b = _identical64()
    return _f32(a), _f32(b)


def near_identical():
    """b[i] = a[i] turned by 1e-3 rad and moved by 1e-3 m: up to 8 crossings + 8 margin corners = 16 vertices."""
    rng = np.random.default_rng(102)
    n = 128
    a = _box(_spread(n), rng.uniform([0.6, 0.5], [4.1, 2.0], (n, 2)), rng.uniform(-3.1, 3.1, n))
    b = a.copy()
    phi = rng.uniform(0, 2 * np.pi, n)
    b[:, 0] += 1e-3 * np.cos(phi)
    b[:, 1] += 1e-3 * np.sin(phi)
    b[:, 6] += np.where(rng.random(n) < 0.5, 1e-3, -1e-3)
    return _f32(a), _f32(b)


GRID = 1.0 / 64


def _grid_axis64():
    """Heading-0 boxes with centres on multiples of 1/64 and sizes on multiples of 1/32 (so every edge lies on a multiple
    of 1/64: two edges coincide or are 1/64 > 1e-2 apart, never inside the margin band), sizes 0.5 .. 2, centres within
    1.5 of the origin: pairs that share an edge or a corner, nested pairs (flush and not) and partial overlaps."""
    rng = np.random.default_rng(103)
    fixed = [  # (x, y, dx, dy)
        (0, 0, 1, 1), (1, 0, 1, 1), (1, 1, 1, 1), (0.5, 0, 2, 1), (0, 0, 2, 2), (0.25, 0.25, 0.5, 0.5),
        (0.5, 0.5, 1, 1), (0, 0.75, 1, 0.5), (-0.75, 0, 0.5, 2), (0, 0, 0.5, 2), (0, 0, 2, 0.5), (1.25, -0.25, 0.5, 0.5),
    ]
    n = 96
    xy = np.round(rng.uniform(-1.5, 1.5, (n, 2)) / GRID) * GRID
    dims = np.round(rng.uniform(0.5, 2.0, (n, 2)) / (2 * GRID)) * (2 * GRID)
    f = np.array(fixed, np.float64)
    box = _box(np.concatenate([f[:, :2], xy]), np.concatenate([f[:, 2:], dims]), np.zeros(n + len(fixed)))
    return box, box.copy()


def grid_axis():
    a, b = _grid_axis64()
    return _f32(a), _f32(b)


GRID_ANGLES = {"pi6": np.pi / 6, "pi4": np.pi / 4, "pi2": np.pi / 2, "1.0": 1.0, "2.5": 2.5}


def rotate_about_origin(boxes, angle, shift=(0.0, 0.0)):
    """float64 boxes turned about the origin by `angle` (centres and headings), then moved by `shift`."""
    out = np.array(boxes, np.float64)
    c, s = np.cos(angle), np.sin(angle)
    out[:, 0] = boxes[:, 0] * c - boxes[:, 1] * s + shift[0]
    out[:, 1] = boxes[:, 0] * s + boxes[:, 1] * c + shift[1]
    out[:, 6] = boxes[:, 6] + angle
    return out


def grid_axis_rotated(angle):
    """The pairs of grid_axis with both boxes turned about the origin by a common angle (one family per angle of
    GRID_ANGLES, "grid_axis_rotated_<angle>"): centres and headings are then rounded to fp32."""
    a, b = _grid_axis64()
    return _f32(rotate_about_origin(a, angle)), _f32(rotate_about_origin(b, angle))


def _octagon64():
    rng = np.random.default_rng(105)
    n = 128
    s = rng.uniform(0.5, 4.0, 64)
    dims = np.concatenate([np.stack([s, s], 1), np.tile([4.0, 1.0], (64, 1))])
    a = _exact(_box(_spread(n), dims, rng.uniform(-3.1, 3.1, n)))
    b = a.copy()
    b[:64, 6] += np.pi / 4
    b[64:, 6] += np.pi / 2
    return a, b


def octagon():
    """i < 64: equal squares of side s, b turned by pi / 4 about the common centre (overlap 2 (sqrt 2 - 1) s^2);
    i >= 64: 4 x 1 boxes, b turned by pi / 2 (overlap 1).  Other pairs are out of reach of each other.  a is exact in
    fp32; the turned headings of b are rounded."""
    a, b = _octagon64()
    return _f32(a), _f32(b)


def wrapped_heading():
    """clustered, 36 boxes per k in -3 .. 3, with 2 pi k added to the headings of both operands."""
    a, b = _clustered64()
    k = np.repeat(np.arange(-3, 4), 36)
    a, b = a[:252].astype(np.float64), b[:252].astype(np.float64)
    a[:, 6] += 2 * np.pi * k
    b[:, 6] += 2 * np.pi * k
    return _f32(a), _f32(b)


FAR_SHIFTS = ((75.0, 75.0), (75.0, -75.0), (-75.0, 75.0), (-75.0, -75.0), (150.0, -150.0))


def far():
    """clustered, 51 boxes per translation of FAR_SHIFTS, both operands moved alike."""
    a, b = _clustered64()
    t = np.repeat(np.array(FAR_SHIFTS), 51, 0)
    a, b = a[:255].astype(np.float64), b[:255].astype(np.float64)
    a[:, :2] += t
    b[:, :2] += t
    return _f32(a), _f32(b)


def thin():
    """20 x 0.05 boxes: a through the origin region at any heading; b[:96] cross them at any heading, b[96:] run within
    0.02 rad of a partner of a, up to 5 along and 0.3 across from it."""
    rng = np.random.default_rng(107)
    n = 128
    dims = np.tile([20.0, 0.05], (n, 1))
    a = _box(rng.uniform(-3, 3, (n, 2)), dims, rng.uniform(-3.1, 3.1, n))
    b = _box(rng.uniform(-3, 3, (n, 2)), dims, rng.uniform(-3.1, 3.1, n))
    k = np.arange(96, n)
    along, across = rng.uniform(-5, 5, len(k)), rng.uniform(-0.3, 0.3, len(k))
    c, s = np.cos(a[k, 6]), np.sin(a[k, 6])
    b[k, 0] = a[k, 0] + along * c - across * s
    b[k, 1] = a[k, 1] + along * s + across * c
    b[k, 6] = a[k, 6] + rng.uniform(-0.02, 0.02, len(k))
    return _f32(a), _f32(b)


def sub_margin():
    """Sizes in [0, 0.02] (a quarter of them exactly 0), all centres within 0.015 of one point near the origin, so within
    0.03 of each other.  Seven boxes in eight are smaller still (sizes up to 0.006, centres within 0.002 of the point):
    every corner of those lies well inside the other's margin, which keeps the share of pairs with a corner on the margin
    boundary under the cap; the others put corners on both sides of it."""
    rng = np.random.default_rng(109)
    n = 96

    def draw():
        deep = rng.random(n) < 0.88
        dims = rng.uniform(0, 1, (n, 2)) * np.where(deep, 0.006, 0.02)[:, None] * (rng.random((n, 2)) > 0.25)
        r, phi = np.where(deep, 0.002, 0.015) * np.sqrt(rng.random(n)), rng.uniform(0, 2 * np.pi, n)
        return _box(np.stack([0.5 + r * np.cos(phi), -0.25 + r * np.sin(phi)], 1), dims, rng.uniform(-3.1, 3.1, n))

    return _f32(draw()), _f32(draw())


FAMILIES = {"clustered": clustered, "identical": identical, "near_identical": near_identical, "grid_axis": grid_axis,
            "octagon": octagon, "wrapped_heading": wrapped_heading, "far": far,
            "thin": thin, "sub_margin": sub_margin}
for _k, _angle in GRID_ANGLES.items():
    FAMILIES["grid_axis_rotated_" + _k] = (lambda t: lambda: grid_axis_rotated(t))(_angle)


def closed_form(name):
    """-> (known (n, m) bool, overlap area (n, m) float64) of the family's pairs with a closed-form intersection, stated
    for the ideal (unrounded) boxes; None for a family without one."""
    if name.startswith("grid_axis"):
        a, b = _grid_axis64()
        area = axis_overlap(a, b)
        return np.ones(area.shape, bool), area
    if name == "identical":
        a, _ = _identical64()
        return np.ones((len(a), len(a)), bool), np.diag(a[:, 3] * a[:, 4])
    if name == "octagon":
        a, _ = _octagon64()
        s = a[:, 3]
        return np.ones((len(a), len(a)), bool), np.diag(np.where(np.arange(len(a)) < 64, 2 * (np.sqrt(2) - 1) * s * s, 1.0))
    return None


# How far the closed form, stated for the ideal boxes, may lie from the IoU of the fp32 boxes the kernel is given.
# grid_axis holds its boxes exactly.  In identical and octagon a is exact and b differs from it by the turn alone, whose
# heading is rounded to fp32: by at most half an ulp of 6.25, 2.4e-7 rad.
# octagon: both areas are stationary in the relative heading (the octagon by symmetry, the cross as 1 / sin), so the error
#   is of second order: < 1e-12.
# identical: the turn error moves b's corners by at most 2.4e-7 times a half diagonal <= 2.3: delta = 5.5e-7, and the
#   bound of grid_axis_rotated below, 16 delta, holds here too (w, h >= 0.5).
# grid_axis_rotated: centres (|x|, |y| < 4: half an ulp 2.4e-7 per coordinate, 3.4e-7 per box) and headings (half an ulp
#   of 2.5 is 1.2e-7 rad, times a half diagonal <= 1.42: 1.7e-7 per box) are rounded: the two boxes of a pair move by at
#   most delta = 2 (3.4e-7 + 1.7e-7) = 1.0e-6 against each other.  The intersection changes by at most its perimeter times
#   delta, the perimeter is at most the smaller box's, 2 (w + h), and the union at least w h, so with w, h >= 0.5 the IoU
#   changes by at most (1 + IoU) 2 (1 / w + 1 / h) delta <= 16 delta.
CLOSED_FORM_INPUT_ERR = {"grid_axis": 0.0, "identical": 16 * 5.5e-7, "octagon": 1e-12, "grid_axis_rotated": 16 * 1.0e-6}


# -------------------------------------------------------------------------------------------------------- NMS draws
NMS_SIZES = (63, 64, 65, 127, 128, 129, 1025)
NMS_SEEDS = {63: 0, 64: 0, 65: 0, 127: 1, 128: 0, 129: 0, 1025: 8}


def nms_boxes(n, grid=False):
    """n car-sized boxes in score order around max(1, n // 3) cluster centres of a square (30 m up to 128 boxes, then growing with n to keep the density), any heading, with the seed
    of NMS_SEEDS[n]: chosen so that every pair of the draw is margin-stable (tests/test_box_iou_ref.py).  grid: centres and
    sizes rounded to multiples of 1/64, which makes the axis-aligned IoU exact up to its division."""
    rng = np.random.default_rng(1000 * NMS_SEEDS[n] + n)
    nc = max(1, n // 3)
    ctr = rng.uniform(0, 30.0 * max(1.0, n / 128) ** 0.5, (nc, 2))
    xy = ctr[rng.integers(0, nc, n)] + rng.normal(0, 0.5, (n, 2))
    dims = np.array([3.9, 1.6]) * rng.uniform(0.8, 1.2, (n, 2))
    box = _box(xy, dims, rng.uniform(-np.pi, np.pi, n))
    if grid:
        box[:, :6] = np.round(box[:, :6] / GRID) * GRID
    return _f32(box)


# known-answer structures on exact-grid boxes, heading 0, in score order
def chain(n):
    """1 x 1 boxes 0.5 apart: neighbours IoU 1/3, second neighbours touch (IoU 0) -> at 0.2 the even positions stay."""
    return _f32(_box(np.stack([0.5 * np.arange(n), np.zeros(n)], 1), np.ones((n, 2)), np.zeros(n)))


def star(n):
    """Box 0 covers all the others, which are 1 x 1 and 2 apart: IoU(0, i) = 1 / area(0) > 0 -> keep [0] below it."""
    side = 2.0 * n + 2
    xy = np.stack([2.0 * np.arange(n) - (n - 1), np.zeros(n)], 1)
    xy[0] = 0
    dims = np.ones((n, 2))
    dims[0] = [side, 2.0]
    return _f32(_box(xy, dims, np.zeros(n)))


def all_identical(n):
    return _f32(_box(np.tile([3.0, -2.0], (n, 1)), np.tile([2.0, 1.0], (n, 1)), np.zeros(n)))


def all_disjoint(n):
    return _f32(_box(np.stack([2.0 * np.arange(n), np.zeros(n)], 1), np.ones((n, 2)), np.zeros(n)))


def late_hit(n):
    """All disjoint, but the last box lies on box 0 (IoU 1/3): keep everything except the last."""
    box = all_disjoint(n)
    box[n - 1, :2] = [0.5, 0.0]
    return box


def nested_flush():
    """A 2 x 1 box and a 1 x 1 box flush inside it: axis-aligned IoU exactly 0.5 in fp32."""
    return _f32(_box([[0.0, 0.0], [-0.5, 0.0]], [[2.0, 1.0], [1.0, 1.0]], np.zeros(2)))
