"""Plain float64 restatements of the second stage (numpy only), and the inputs the GPU tests run them on.

  sample / sample_frame   RoI / GT matching and fg / hard-bg / easy-bg sampling of the reference's ProposalTargetLayer
                          (proposal_target_layer.py:64-228) with its random numbers as inputs: fg_keys (argsort = its
                          np.random.permutation) and slot_u (the uniforms behind np.random.rand and torch.randint).  These
                          are the rules of include/spx.h §26.
  targets                 forward's labels (reg_valid_mask, rcnn_cls_labels of both kinds) and RoIHeadTemplate
                          .assign_targets' canonical transform (roi_head_template.py:121-151).
  roi_grid_pool           SECONDHead.roi_grid_pool (second_head.py:53-110): theta rounded to float32 (the reference's
                          .float()), then affine_grid and grid_sample with align_corners=False, bilinear, zero padding.
The 3-D IoU is tests/box_iou_ref.iou3d_ref, the float64 twin of box_iou.h.  tests/test_roi_head_ref.py pins all of it to
what the reference recorded (tests/golden/roi_head.npz)."""
import functools

import numpy as np

import box_iou_ref as R

DEFAULT_CFG = dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou",
                   CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
REG_ABOVE_CLS = dict(DEFAULT_CFG, REG_FG_THRESH=0.8, CLS_FG_THRESH=0.6)       # fg and hard bg overlap on [0.6, 0.8)
MARGIN = 1e-3      # 5 x the loosest per-family IoU tolerance of DESIGN.md §8 (far: 1.9e-4)


# ------------------------------------------------------------------------------------------------ matching and sampling
def trim(gt):
    """Number of GT rows kept: trailing rows whose sum is 0 go; row 0 always stays, interior zero rows stay."""
    k = len(gt) - 1
    while k > 0 and gt[k].sum() == 0:
        k -= 1
    return k + 1


def match(rois, roi_labels, gt, by_class, iou_fn=None):
    """-> (max_overlaps (R), gt_assignment (R), iou (R, n_gt)).  Largest IoU, lowest row on ties; by_class: only rows of
    the RoI's class count, a RoI without one gets (0, 0), one whose rows all have IoU 0 the first of them."""
    iou_fn = iou_fn or (lambda a, b: R.iou3d_ref(a, b)[0])
    gt = gt[:trim(gt)]
    iou = iou_fn(np.asarray(rois[:, :7], np.float64), np.asarray(gt[:, :7], np.float64))
    if by_class:
        same = np.asarray(roi_labels).reshape(-1, 1) == gt[:, -1].astype(np.int64).reshape(1, -1)
        masked = np.where(same, iou, -1.0)
        has = same.any(1)
        return np.where(has, masked.max(1), 0.0), np.where(has, masked.argmax(1), 0), iou
    return iou.max(1), iou.argmax(1), iou          # numpy's argmax is the first maximum


def sample_frame(max_overlaps, cfg, fg_keys, slot_u):
    """-> sampled RoI rows (M).  fg with bg present: without replacement, ascending (key, index); every other slot s:
    entry min(floor(slot_u[s] * n), n - 1) of its list; order fg, hard bg, easy bg."""
    m = int(cfg["ROI_PER_IMAGE"])
    fg_per_image = int(np.round(cfg["FG_RATIO"] * m))
    fg_thresh = min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])
    fg = np.nonzero(max_overlaps >= fg_thresh)[0]
    easy = np.nonzero(max_overlaps < cfg["CLS_BG_THRESH_LO"])[0]
    hard = np.nonzero((max_overlaps < cfg["REG_FG_THRESH"]) & (max_overlaps >= cfg["CLS_BG_THRESH_LO"]))[0]
    u = np.asarray(slot_u, np.float64)

    def draw(lst, lo, hi):
        return lst[np.minimum(np.floor(u[lo:hi] * len(lst)).astype(np.int64), len(lst) - 1)]

    if len(fg) > 0 and len(hard) + len(easy) == 0:
        return draw(fg, 0, m)
    assert len(hard) + len(easy) > 0
    n_take = min(fg_per_image, len(fg))
    order = np.lexsort((fg, np.asarray(fg_keys)[fg]))              # primary key fg_keys, then the RoI index
    parts = [fg[order[:n_take]]]
    bg = m - n_take
    if len(hard) > 0 and len(easy) > 0:
        n_hard = min(int(bg * cfg["HARD_BG_RATIO"]), len(hard))
    else:
        n_hard = bg if len(hard) > 0 else 0
    if n_hard:
        parts.append(draw(hard, n_take, n_take + n_hard))
    if bg - n_hard:
        parts.append(draw(easy, n_take + n_hard, m))
    return np.concatenate(parts)


def sample(rois, roi_labels, gt_boxes, cfg, fg_keys, slot_u, iou_fn=None):
    """Batch -> dict(sampled_inds (B, M), roi_ious (B, M), gt_inds (B, M))."""
    out = dict(sampled_inds=[], roi_ious=[], gt_inds=[])
    for b in range(len(rois)):
        ovl, asg, _ = match(rois[b], roi_labels[b], gt_boxes[b], cfg.get("SAMPLE_ROI_BY_EACH_CLASS", False), iou_fn)
        s = sample_frame(ovl, cfg, fg_keys[b], slot_u[b])
        out["sampled_inds"].append(s), out["roi_ious"].append(ovl[s]), out["gt_inds"].append(asg[s])
    return {k: np.stack(v) for k, v in out.items()}


# --------------------------------------------------------------------------------------------- labels and the transform
def _rotate_z(points, angle):
    """common_utils.rotate_points_along_z with the matrix rounded to float32, as the reference's .float() does."""
    c = np.cos(angle).astype(np.float32).astype(np.float64)
    s = np.sin(angle).astype(np.float32).astype(np.float64)
    x, y = points[..., 0], points[..., 1]
    out = points.copy()
    out[..., 0], out[..., 1] = x * c - y * s, x * s + y * c
    return out


def targets(rois, roi_scores, roi_labels, gt_boxes, picked, cfg):
    """The targets_dict of assign_targets from the sampled rows: float64 everywhere."""
    b = np.arange(len(rois))[:, None]
    s, g = picked["sampled_inds"], picked["gt_inds"]
    out = dict(rois=np.asarray(rois, np.float64)[b, s], gt_of_rois_src=np.asarray(gt_boxes, np.float64)[b, g],
               gt_iou_of_rois=picked["roi_ious"], roi_scores=np.asarray(roi_scores, np.float64)[b, s],
               roi_labels=np.asarray(roi_labels)[b, s])
    iou = out["gt_iou_of_rois"]
    out["reg_valid_mask"] = (iou > cfg["REG_FG_THRESH"]).astype(np.int64)
    if cfg["CLS_SCORE_TYPE"] == "cls":
        lab = (iou > cfg["CLS_FG_THRESH"]).astype(np.int64)
        lab[(iou > cfg["CLS_BG_THRESH"]) & (iou < cfg["CLS_FG_THRESH"])] = -1
    else:
        fg, bg = iou > cfg["CLS_FG_THRESH"], iou < cfg["CLS_BG_THRESH"]
        lab = np.where(~fg & ~bg, (iou - cfg["CLS_BG_THRESH"]) / (cfg["CLS_FG_THRESH"] - cfg["CLS_BG_THRESH"]),
                       fg.astype(np.float64))
    out["rcnn_cls_labels"] = lab
    gt = out["gt_of_rois_src"].copy()
    ry = out["rois"][..., 6] % (2 * np.pi)
    gt[..., 0:3] -= out["rois"][..., 0:3]
    gt[..., 6] -= ry
    gt = _rotate_z(gt, -ry)
    h = gt[..., 6] % (2 * np.pi)
    opposite = (h > np.pi * 0.5) & (h < np.pi * 1.5)
    h = np.where(opposite, (h + np.pi) % (2 * np.pi), h)
    h = np.where(h > np.pi, h - 2 * np.pi, h)
    gt[..., 6] = np.clip(h, -np.pi / 2, np.pi / 2)
    out["gt_of_rois"] = gt
    return out


# ------------------------------------------------------------------------------------------------------- RoI pooling
def roi_grid_pool(rois, feat, g, min_x, min_y, step_x, step_y):
    """rois (B, N, >= 7), feat (B, C, H, W) -> (B * N, C, G, G) float64."""
    rois, feat = np.asarray(rois, np.float64), np.asarray(feat, np.float64)
    bsz, n = rois.shape[:2]
    c, h, w = feat.shape[1:]
    f32 = lambda v: v.astype(np.float32).astype(np.float64)      # noqa: E731
    out = np.zeros((bsz * n, c, g, g))
    base = (2.0 * np.arange(g) + 1.0) / g - 1.0
    bx, by = np.meshgrid(base, base)                                 # [i, j]: x varies along j, y along i
    for b in range(bsz):
        r = rois[b]
        x1, x2 = (r[:, 0] - r[:, 3] / 2 - min_x) / step_x, (r[:, 0] + r[:, 3] / 2 - min_x) / step_x
        y1, y2 = (r[:, 1] - r[:, 4] / 2 - min_y) / step_y, (r[:, 1] + r[:, 4] / 2 - min_y) / step_y
        ca, sa = np.cos(r[:, 6]), np.sin(r[:, 6])
        t00, t01, t02 = f32((x2 - x1) / (w - 1) * ca), f32((x2 - x1) / (w - 1) * (-sa)), f32((x1 + x2 - w + 1) / (w - 1))
        t10, t11, t12 = f32((y2 - y1) / (h - 1) * sa), f32((y2 - y1) / (h - 1) * ca), f32((y1 + y2 - h + 1) / (h - 1))
        for k in range(n):
            gx = t00[k] * bx + t01[k] * by + t02[k]
            gy = t10[k] * bx + t11[k] * by + t12[k]
            ix, iy = ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2
            with np.errstate(invalid="ignore"):
                ok = (ix > -1) & (ix < w) & (iy > -1) & (iy < h)     # NaN / inf coordinates sample nothing
            ix, iy = np.where(ok, ix, -1.0), np.where(ok, iy, -1.0)
            x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
            wx1, wy1 = ix - x0, iy - y0
            acc = np.zeros((c, g, g))
            for dx, dy, wgt in ((0, 0, (1 - wx1) * (1 - wy1)), (1, 0, wx1 * (1 - wy1)), (0, 1, (1 - wx1) * wy1),
                                (1, 1, wx1 * wy1)):
                xx, yy = x0 + dx, y0 + dy
                inside = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                v = feat[b][:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
                acc += np.where(inside, wgt, 0.0)[None] * np.where(inside[None], v, 0.0)
            out[b * n + k] = acc
    return out


def taps_all_outside(rois, h, w, g, min_x, min_y, step_x, step_y):
    """(B * N, G, G) bool: cells whose four bilinear taps all lie outside the map (the output there is exactly 0)."""
    probe = roi_grid_pool(rois, np.ones((len(rois), 1, h, w)), g, min_x, min_y, step_x, step_y)
    return probe[:, 0] == 0


# ------------------------------------------------------------------------------------------- inputs of the GPU tests
POOL = dict(h=5, w=7, min_x=0.0, min_y=-1.0, step_x=0.4, step_y=0.4)     # the map covers x 0 .. 2.8, y -1 .. 1


def pool_rois(n, seed=0):
    """(2, n, 7) float32: the named RoIs first (as many as fit), then random ones around the map."""
    named = np.array([
        [1.4, 0.0, 0, 1.2, 0.8, 1, 0.0],                  # axis-aligned, inside
        [1.4, 0.0, 0, 1.6, 0.8, 1, np.pi / 6],            # 30 degrees
        [1.2, 0.1, 0, 1.0, 0.6, 1, np.pi],                # heading +pi
        [1.2, 0.1, 0, 1.0, 0.6, 1, -np.pi],               # heading -pi
        [0.0, 0.0, 0, 1.0, 0.8, 1, 0.2],                  # straddles x = min
        [2.8, 0.2, 0, 1.0, 0.8, 1, -0.3],                 # straddles x = max
        [1.0, -1.0, 0, 1.0, 0.8, 1, 0.1],                 # straddles y = min
        [1.8, 1.0, 0, 1.0, 0.8, 1, 1.2],                  # straddles y = max
        [9.0, 9.0, 0, 1.0, 1.0, 1, 0.4],                  # wholly outside
        [-5.0, 0.0, 0, 0.5, 0.5, 1, 0.0],                 # wholly outside
        [1.3, 0.3, 0, 0.0, 0.0, 1, 0.7],                  # zero extent: every sample at the centre
        [0.0, 0.0, 0, 0.0, 0.0, 0, 0.0],                  # the proposal layer's padding row
    ], np.float64)
    rng = np.random.default_rng(100 + seed)
    out = np.zeros((2, n, 7))
    for b in range(2):
        rnd = np.stack([rng.uniform(-0.5, 3.3, n), rng.uniform(-1.5, 1.5, n), np.zeros(n), rng.uniform(0.1, 2.0, n),
                        rng.uniform(0.1, 1.5, n), np.ones(n), rng.uniform(-4, 4, n)], 1)
        rows = np.concatenate([np.roll(named, -b * 5, 0), rnd])[:n]      # n == 1: frame 0 inside, frame 1 border
        out[b] = rows
    return out.astype(np.float32)


def pool_features(c, seed=0):
    return np.random.default_rng(200 + seed).normal(size=(2, c, POOL["h"], POOL["w"])).astype(np.float32)


# RoI bands by the fraction f of the box length a copy of a GT is shifted along its axis: IoU ~ (1 - f) / (1 + f)
_BANDS = {"fg": (0.02, 0.08), "mid": (0.17, 0.2), "hard": (0.35, 0.6), "easy": (0.86, 0.95), "zero": None}
_KINDS = {
    "many_fg": ["fg", "fg", "fg", "mid", "fg", "hard", "easy", "fg", "zero", "fg"],
    "few_fg": ["hard", "easy", "zero", "hard", "easy", "hard", "zero", "easy", "hard", "easy"],     # + 3 fg rows, below
    "fg_only": ["fg", "mid"],
    "bg_only": ["hard", "easy", "zero", "hard"],
    "hard_only": ["hard"],
    "easy_only": ["easy", "zero"],
}
GMAX = 7


def _gt(kind, rng):
    """(GMAX, 8) float32.  none: all zero.  one: one car.  several: two cars, an interior zero row, two adjacent
    class-2 boxes 1.3 m apart (they overlap: a RoI on one also meets the other), trailing zero rows."""
    gt = np.zeros((GMAX, 8))
    if kind == "none":
        return gt.astype(np.float32)
    car = lambda x, y, yaw, cls: [x, y, -1.0, 3.9, 1.6, 1.5, yaw, cls]      # noqa: E731
    if kind == "one":
        gt[0] = car(12.0, 3.0, 0.3, 1)
    else:
        gt[0] = car(10.0, -8.0, 0.0, 1)
        gt[1] = car(22.0, 6.0, rng.uniform(-1, 1), 1)
        gt[3] = car(30.0, -4.0, 0.1, 2)
        gt[4] = car(30.0, -2.7, 0.1, 2)
    return gt.astype(np.float32)


_ALL_THRESHOLDS = (0.1, 0.25, 0.55, 0.6, 0.75, 0.8)       # of DEFAULT_CFG and REG_ABOVE_CLS


def _violates(rois, gt):
    """(R) bool: rows with a pair that is margin-unstable, within MARGIN of a threshold, or whose two best IoUs are closer
    than MARGIN without both being 0 (the input condition of check_input_condition, per RoI)."""
    gt = gt[:trim(gt)]
    iou, clear = R.iou3d_ref(rois[:, :7].astype(np.float64), gt[:, :7].astype(np.float64))
    bad = ~(R.stable(clear) | (iou == 0)).all(1)
    for t in _ALL_THRESHOLDS:
        bad |= ~((iou == 0) | (np.abs(iou - t) >= MARGIN)).all(1)
    if iou.shape[1] > 1:
        top = np.sort(iou, 1)[:, -2:]
        bad |= ~((top[:, 1] == 0) | (top[:, 1] - top[:, 0] >= MARGIN))
    return bad


def _roi(i, kind, gt_kind, gt, live, rng):
    bands = _KINDS[kind]
    band = bands[i % len(bands)]
    if kind == "few_fg" and i in (1, 4, 6):
        band = "fg"
    if not live or band == "zero":
        return [rng.uniform(45, 60), rng.uniform(-30, 30), -1.0, 3.9, 1.6, 1.5, rng.uniform(-3, 3)], 1 + i % 2
    j = live[i % len(live)]
    lo, hi = _BANDS[band]
    f = rng.uniform(lo, hi) * (1 if i % 4 < 2 else -1)
    yaw = float(gt[j, 6])
    box = gt[j, :7].astype(np.float64).copy()
    box[0] += f * box[3] * np.cos(yaw)
    box[1] += f * box[3] * np.sin(yaw)
    box[6] += rng.uniform(0.015, 0.03) * (1 if i % 2 else -1)       # corners well clear of box_iou.h's 1e-2 margin band
    label = int(gt[j, 7])
    if gt_kind == "several" and kind in ("many_fg", "few_fg", "bg_only") and i % 10 == 9:
        label = 3                                          # a class with no GT: overlap 0 when sampling by class
    return box, label


def _frame(kind, gt_kind, r, rng):
    """One frame's RoIs: every RoI is redrawn until all its pairs meet the input condition."""
    gt = _gt(gt_kind, rng)
    live = [i for i in range(GMAX) if gt[i].any()]
    rois, labels = np.zeros((r, 7), np.float32), np.ones(r, np.int64)
    todo = np.arange(r)
    for _ in range(100):
        for i in todo:
            rois[i], labels[i] = _roi(i, kind, gt_kind, gt, live, rng)
        todo = todo[_violates(rois[todo], gt)]
        if len(todo) == 0:
            return rois, labels, gt
    raise AssertionError("no admissible RoI found")


_TRIPLES = {
    "t1": (("many_fg", "several"), ("fg_only", "one"), ("easy_only", "none")),
    "t2": (("few_fg", "several"), ("hard_only", "one"), ("easy_only", "several")),
    "t3": (("bg_only", "several"), ("many_fg", "one"), ("fg_only", "several")),
}


@functools.lru_cache(maxsize=None)
def sampling_cases():
    """name -> dict(rois (3, R, 7), roi_labels, gt_boxes (3, GMAX, 8), cfg, fg_keys (3, R), slot_u (3, M), kinds).
    Cached: callers must not write to the arrays."""
    out = {}
    for r in (1, 7, 513):
        for m in (4, 128):
            for by_class in (True, False):
                for t, frames in _TRIPLES.items():
                    cfgs = [("", DEFAULT_CFG)] + ([("_reg_above_cls", REG_ABOVE_CLS)] if t == "t1" and r > 1 else [])
                    for tag, base in cfgs:
                        name = "r%d_m%d_%s_%s%s" % (r, m, "cls" if by_class else "all", t, tag)
                        rng = np.random.default_rng(r * 1000 + m * 10 + by_class * 5 + int(t[1]))
                        fr = [_frame(k, g, r, rng) for k, g in frames]
                        out[name] = dict(rois=np.stack([f[0] for f in fr]), roi_labels=np.stack([f[1] for f in fr]),
                                         gt_boxes=np.stack([f[2] for f in fr]),
                                         cfg=dict(base, ROI_PER_IMAGE=m, SAMPLE_ROI_BY_EACH_CLASS=by_class),
                                         fg_keys=rng.random((3, r)).astype(np.float32),
                                         slot_u=rng.random((3, m)).astype(np.float32), kinds=frames)
    return out


def check_input_condition(case):
    """Asserts, in float64 and for EVERY RoI / GT pair of the case: the pair is margin-stable or disjoint, its IoU is
    exactly 0 or at least MARGIN from every threshold, and the two largest IoUs of a RoI differ by at least MARGIN unless
    both are exactly 0.  Returns the per-frame (n_fg, n_hard, n_easy)."""
    cfg = case["cfg"]
    thresholds = [cfg[k] for k in ("REG_FG_THRESH", "CLS_FG_THRESH", "CLS_BG_THRESH", "CLS_BG_THRESH_LO")]
    counts = []
    for b in range(len(case["rois"])):
        gt = case["gt_boxes"][b][:trim(case["gt_boxes"][b])]
        iou, clear = R.iou3d_ref(case["rois"][b][:, :7].astype(np.float64), gt[:, :7].astype(np.float64))
        assert (R.stable(clear) | (iou == 0)).all()
        for t in thresholds:
            assert ((iou == 0) | (np.abs(iou - t) >= MARGIN)).all(), (b, t)
        if iou.shape[1] > 1:
            top = np.sort(iou, 1)[:, -2:]
            assert ((top[:, 1] == 0) | (top[:, 1] - top[:, 0] >= MARGIN)).all(), b
        ovl = match(case["rois"][b], case["roi_labels"][b], case["gt_boxes"][b], cfg["SAMPLE_ROI_BY_EACH_CLASS"])[0]
        fg = ovl >= min(cfg["REG_FG_THRESH"], cfg["CLS_FG_THRESH"])
        hard = (ovl < cfg["REG_FG_THRESH"]) & (ovl >= cfg["CLS_BG_THRESH_LO"])
        counts.append((int(fg.sum()), int(hard.sum()), int((ovl < cfg["CLS_BG_THRESH_LO"]).sum())))
    return counts
