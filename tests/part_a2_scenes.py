"""Scene builders shared by the Part-A2 / sparse RoI-aware pooling tests, the golden recorder
(tests/golden/make_golden_part_a2.py) and tests/part_a2_ref.py.  Not a test module: the recorded data depends on these
functions staying as they are."""
import numpy as np

F32 = np.float32


def scene(seed, cnt, n, c=3, zero_frac=0.2):
    """Frames of cnt[b] points around a few rotated boxes; part in [0, 1) with exact zeros; integer-valued rpn."""
    rng = np.random.default_rng(seed)
    b = len(cnt)
    rois = np.zeros((b, n, 7), F32)
    pts = []
    for f in range(b):
        ctr = rng.uniform(-4, 4, size=(n, 3)) * [1, 1, 0.2]
        rois[f, :, :3] = ctr
        rois[f, :, 3:6] = rng.uniform(1.5, 4.0, size=(n, 3))
        rois[f, :, 6] = rng.uniform(-3.2, 3.2, size=n)
        p = ctr[rng.integers(0, n, cnt[f])] + rng.normal(scale=1.2, size=(cnt[f], 3))
        pts.append(np.concatenate([np.full((cnt[f], 1), f), p], axis=1))
    pts = np.concatenate(pts).astype(F32)
    part = rng.uniform(0, 1, size=(pts.shape[0], 4)).astype(F32)
    part[rng.uniform(size=pts.shape[0]) < zero_frac] = 0
    rpn = rng.integers(-8, 9, size=(pts.shape[0], c)).astype(F32)
    return rois, pts, np.asarray(cnt, np.int32), part, rpn


def grid_scene(cells, zero_cells=(), n_rois=2):
    """One frame, n_rois unit-cell RoIs of out size 2 x 2 x 2 far apart; RoI 0 gets one point in each of `cells`
    (part 0.5) and `zero_cells` (part exactly 0)."""
    rois = np.zeros((1, n_rois, 7), F32)
    rois[0, :, 0] = np.arange(n_rois) * 10.0
    rois[0, :, 3:6] = 2.0
    pts, part = [], []
    for v in list(cells) + list(zero_cells):
        x, y, z = v // 4, (v // 2) % 2, v % 2
        pts.append([0, x - 0.5, y - 0.5, z - 0.5])
        part.append([0.5, 0, 0, 0] if v in cells else [0, 0, 0, 0])
    pts = np.asarray(pts, F32).reshape(-1, 4)
    part = np.asarray(part, F32).reshape(-1, 4)
    rpn = np.arange(1, pts.shape[0] * 2 + 1, dtype=F32).reshape(-1, 2)
    return rois, pts, np.asarray([pts.shape[0]], np.int32), part, rpn
