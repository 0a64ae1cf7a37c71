"""Inputs of the roipoint_pool3d tests (tests/test_roipoint_pool3d_ref.py): a random sweep over the shape grid, one
hand-built scene with every edge of the inside test and of the slot rule, and one long scene (2 500 points, S = 600).
All float32 numpy; the truth comes from tests/roipoint_pool3d_ref.py."""
import numpy as np

F32 = np.float32

SWEEP_N, SWEEP_M, SWEEP_C, SWEEP_S = (1, 63, 130), (1, 5), (1, 64, 130), (1, 8, 64, 600)
EDGE_S = 8
# (1 + 0.1f) rounds up in float32: a point at |z - cz| = fl32(1 + 0.1f) / 2 is inside only if the box grew by a float32 add
ROUNDING_WIDTH = (0.1, 0.1, 0.1)
ROUNDING_HALF = F32(F32(1.0) + F32(0.1)) / F32(2)


def sweep_case(n, m, c, stride, seed):
    """Two different frames: points in [-2, 2]^3; box 0 of frame 0 holds every point, box 1 none, boxes 2, 3, 4 have
    headings pi, -pi and 30 degrees, the rest random."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(-2, 2, (2, n, 3)).astype(F32)
    feats = rng.standard_normal((2, n, c)).astype(F32)
    scores = rng.uniform(0, 1, (2, n)).astype(F32)
    boxes = np.zeros((2, m, stride), F32)
    boxes[..., :3] = rng.uniform(-1, 1, (2, m, 3))
    boxes[..., 3:6] = rng.uniform(0.5, 4, (2, m, 3))
    boxes[..., 6] = rng.uniform(-3, 3, (2, m))
    boxes[..., 7:] = rng.uniform(-5, 5, (2, m, stride - 7))           # columns the op must not read
    boxes[0, 0, :7] = (0, 0, 0, 20, 20, 20, 0.3)
    if m > 1:
        boxes[0, 1, :3] = (50, 50, 50)
        boxes[:, 2, 6], boxes[:, 3, 6], boxes[:, 4, 6] = F32(np.pi), F32(-np.pi), F32(np.pi / 6)
    return dict(points=points, feats=feats, scores=scores, boxes=boxes)


def edge_case(c=5, stride=9, seed=3):
    """One scene, S = EDGE_S = 8.  Boxes (all of size 1 unless said), frame 0; frame 1 is the same scene with other
    features, without the point on the origin and with its points in another order:
      0: S - 1 points   1: S points   2: S + 1 points   3: one point   4: empty
      5: dz = 1, a point at z = cz + 0.5 exactly (inside) and one a float32 step above (outside)
      6: dx = 2, heading 0: points at local x = 1 exactly and one float32 step past it (inside through the 1e-5 margin) and
         at 1 + 2e-5 (outside)
      7: the all-zero padding RoI; frame 0 has a point on the origin, frame 1 has not
      8, 9, 10: headings pi, -pi, 30 degrees over one random cluster
      11: centre z = 0, dz = 1: a point at z = ROUNDING_HALF, inside only with ROUNDING_WIDTH added in float32.
    -> dict(points (2, N, 3), feats (2, N, C), scores (2, N), boxes (2, 12, stride), expected={box: cnt at width 0})."""
    rng = np.random.default_rng(seed)
    s = EDGE_S
    pts = []
    for k, cnt in enumerate((s - 1, s, s + 1, 1)):
        pts.append(np.array([10.0 * (k + 1), 0, 0]) + rng.uniform(-0.3, 0.3, (cnt, 3)))
    up = np.nextafter(F32(0.5), F32(1))
    pts.append(np.array([[60, 0, 0.5], [60, 0, up]]))
    x1 = F32(71)
    pts.append(np.array([[x1, 0, 0], [np.nextafter(x1, F32(100)), 0, 0], [F32(71 + 2e-5), 0, 0]]))
    pts.append(np.array([[0, 0, 0]]))                                                 # the last but one block: the origin
    cluster = np.array([90.0, 5, 1]) + rng.uniform(-1.5, 1.5, (24, 3))
    pts.append(cluster)
    pts.append(np.array([[110, 0, ROUNDING_HALF]]))
    pts = np.concatenate(pts).astype(F32)
    origin_row = (s - 1) + s + (s + 1) + 1 + 2 + 3
    n = len(pts)
    boxes = np.zeros((12, stride), F32)
    for k in range(4):
        boxes[k, :7] = (10.0 * (k + 1), 0, 0, 1, 1, 1, 0.2 * k)
    boxes[4, :7] = (50, 0, 0, 1, 1, 1, 0)
    boxes[5, :7] = (60, 0, 0, 1, 1, 1, 0)
    boxes[6, :7] = (70, 0, 0, 2, 1, 1, 0)
    for k, h in zip((8, 9, 10), (np.pi, -np.pi, np.pi / 6)):
        boxes[k, :7] = (90, 5, 1, 2.0, 1.2, 1.6, h)
    boxes[11, :7] = (110, 0, 0, 1, 1, 1, 0)
    boxes[:, 7:] = rng.uniform(-5, 5, (12, stride - 7))
    boxes[7] = 0
    frames_p, frames_b = [], []
    for f in range(2):
        p = pts.copy()
        if f == 1:
            p[origin_row] = (100, 100, 100)
        order = np.random.default_rng(seed + 10 + f).permutation(n)
        frames_p.append(p[order])
        frames_b.append(boxes)
    points = np.stack(frames_p)
    feats = rng.standard_normal((2, n, c)).astype(F32)
    scores = rng.uniform(0, 1, (2, n)).astype(F32)
    expected = {0: (s - 1, s - 1), 1: (s, s), 2: (s + 1, s + 1), 3: (1, 1), 4: (0, 0), 5: (1, 1), 6: (2, 2), 7: (1, 0),
                11: (0, 0)}
    return dict(points=points, feats=feats, scores=scores, boxes=np.stack(frames_b), expected=expected)


def long_case(n=2500, c=3, seed=5):
    """A long frame with S = 600: box 0 holds every point, box 1 about a third of them (more than S), box 2 a few dozen
    spread over the frame (repeats), box 3 none."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(-2, 2, (2, n, 3)).astype(F32)
    feats = rng.standard_normal((2, n, c)).astype(F32)
    scores = rng.uniform(0, 1, (2, n)).astype(F32)
    boxes = np.zeros((2, 4, 7), F32)
    boxes[:, 0] = (0, 0, 0, 9, 9, 9, 0.4)
    boxes[:, 1] = (0.2, 0, 0, 2.9, 2.6, 2.7, 1.1)
    boxes[:, 2] = (-1, 1, 0.5, 0.9, 0.8, 1.0, -2.0)
    boxes[:, 3] = (30, 0, 0, 1, 1, 1, 0.7)
    boxes[1, :, :3] += F32(0.1)
    return dict(points=points, feats=feats, scores=scores, boxes=boxes)
