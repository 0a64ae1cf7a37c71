"""Plain numpy restatement of spx_center_decode (include/spx.h §21) for the tests, and the table of cases.

Selection: a stable sort of the frame's C*H*W values by (-value, flat index), -0 equal to +0, through the same
order-preserving integer key the op uses (so that even NaN bit patterns have one answer); the first K are the rows.
x and y are float32 arithmetic in the reference's association, ((cell + offset) * stride) * voxel_size + range_lo, every
operation rounded; z and vel are copied.  The transcendental columns (sigmoid, exp, atan2) are evaluated in float64 and
returned both as float64 (what the GPU test measures ulps against) and rounded once to float32 (what `boxes` / `scores`
hold).  The masks use the float32-rounded score; check_margins() asserts that no case comes near enough to a threshold
for the rounding of anyone's fp32 sigmoid to matter."""
import numpy as np

F32 = np.float32
STRIDE = 8
VOXEL_SIZE = [0.05, 0.05, 0.1]
RANGE_LO = [0.0, -4.0]                 # metres; one heatmap cell is 0.4 m
SCORE_MARGIN = 1e-5                    # relative distance of every candidate's float64 sigmoid from score_thresh
XY_MARGIN = 1e-4                       # metres between every candidate's x, y and the limits


def ordered_key(v):
    """float32 array -> int64 array whose order is the float order, -0 counted as +0."""
    u = (np.ascontiguousarray(v, F32) + F32(0.0)).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def select(hm, k):
    """hm (B, C, H, W) -> (B, k) flat indices c*H*W + y*W + x, best first."""
    b = hm.shape[0]
    key = ordered_key(hm).reshape(b, -1)
    return np.stack([np.argsort(-key[f], kind="stable")[:k] for f in range(b)])


def decode(hm, center, center_z, dim, rot, vel, k, limit, score_thresh=None, raw=True, stride=STRIDE,
           voxel_size=VOXEL_SIZE, range_lo=RANGE_LO):
    """Arrays as spx.ops.center_decode takes them -> dict of numpy arrays: boxes (B, k, 7|9) float32, scores, labels
    int32, cells int64, keep uint8, count int32, and score64 (B, k), dims64 (B, k, 3), angle64 (B, k) in float64."""
    hm, center, center_z, dim, rot = (np.ascontiguousarray(a, F32) for a in (hm, center, center_z, dim, rot))
    b, c, h, w = hm.shape
    hw = h * w
    idx = select(hm, k)
    labels, cells = idx // hw, idx % hw
    ys_i, xs_i = cells // w, cells % w
    fr = np.arange(b)[:, None]
    take = lambda m, ch: m.reshape(b, -1, hw)[fr, ch, cells]                     # noqa: E731
    v = hm.reshape(b, -1)[fr, idx]
    xs = (xs_i.astype(F32) + take(center, 0)) * F32(stride) * F32(voxel_size[0]) + F32(range_lo[0])
    ys = (ys_i.astype(F32) + take(center, 1)) * F32(stride) * F32(voxel_size[1]) + F32(range_lo[1])
    assert xs.dtype == F32 and ys.dtype == F32
    z = take(center_z, 0)
    d = np.stack([take(dim, q) for q in range(3)], axis=-1)
    with np.errstate(over="ignore"):
        dims64 = np.exp(d.astype(np.float64)) if raw else d.astype(np.float64)
        score64 = 1.0 / (1.0 + np.exp(-v.astype(np.float64))) if raw else v.astype(np.float64)
    angle64 = np.arctan2(take(rot, 1).astype(np.float64), take(rot, 0).astype(np.float64))
    scores = score64.astype(F32)
    cols = [xs, ys, z, dims64[..., 0].astype(F32), dims64[..., 1].astype(F32), dims64[..., 2].astype(F32),
            angle64.astype(F32)]
    if vel is not None:
        vel = np.ascontiguousarray(vel, F32)
        cols += [take(vel, 0), take(vel, 1)]
    boxes = np.stack(cols, axis=-1).astype(F32)
    lim = np.asarray(limit, F32)
    keep = (boxes[..., :3] >= lim[:3]).all(-1) & (boxes[..., :3] <= lim[3:]).all(-1)
    if score_thresh is not None:
        keep &= scores > F32(score_thresh)
    return {"boxes": boxes, "scores": scores, "labels": labels.astype(np.int32), "cells": cells.astype(np.int64),
            "keep": keep.astype(np.uint8), "count": keep.sum(1).astype(np.int32), "score64": score64, "dims64": dims64,
            "angle64": angle64}


def decode_case(case):
    return decode(case["hm"], case["center"], case["center_z"], case["dim"], case["rot"], case["vel"], case["k"],
                  case["limit"], case["score_thresh"], case["raw"])


def _spread(rng, n, lo, hi):
    """n pairwise distinct float32 values, evenly spaced over [lo, hi], shuffled: far enough apart (>= 6e-5 here) for
    their float32 sigmoids to stay distinct."""
    return rng.permutation(np.linspace(lo, hi, n)).astype(F32)


def _maps(rng, shape, vel):
    b, _c, h, w = shape
    out = {"center": rng.random((b, 2, h, w)).astype(F32),
           "center_z": rng.normal(-1.0, 0.5, (b, 1, h, w)).astype(F32),
           "dim": rng.normal(0.0, 0.3, (b, 3, h, w)).astype(F32),
           "rot": rng.normal(0.0, 1.0, (b, 2, h, w)).astype(F32),
           "vel": rng.normal(0.0, 2.0, (b, 2, h, w)).astype(F32) if vel else None}
    return out


def _wide(shape):
    """A centre range that holds every cell of the map in x and y."""
    _b, _c, h, w = shape
    return [-5.0, -9.0, -3.0, 0.4 * w + 5.0, 0.4 * h + 5.0, 3.0]


def _case(rng, shape, k, hm, vel=False, score_thresh=0.1, limit=None, raw=True, distinct=False, z_on_limit=False):
    case = _maps(rng, shape, vel)
    case.update(hm=np.ascontiguousarray(hm, F32).reshape(shape), k=k, score_thresh=score_thresh,
                limit=_wide(shape) if limit is None else limit, raw=raw, distinct=distinct, z_on_limit=z_on_limit)
    return case


def cases():
    """name -> case.  `distinct`: the float32 sigmoids of the frame's best 2K values are pairwise distinct, so the
    reference's two-stage topk has one admissible answer and the restatement must equal it."""
    rng = np.random.default_rng(20)
    n = lambda s: int(np.prod(s))                                                # noqa: E731
    out = {}
    s = (1, 1, 4, 4)
    out["all_selected"] = _case(rng, s, 16, _spread(rng, n(s), -4, 3), distinct=True)
    s = (2, 3, 5, 7)
    out["odd_sizes"] = _case(rng, s, 9, _spread(rng, n(s), -4, 3), vel=True, distinct=True)
    s = (3, 2, 40, 44)
    out["several_tiles"] = _case(rng, s, 64, _spread(rng, n(s), -6, 3), score_thresh=None, distinct=True,
                                 limit=[2.0, -1.0, -1.5, 14.0, 11.0, 3.0])
    s = (2, 3, 200, 176)
    hm = np.stack([rng.permutation(np.concatenate([np.linspace(-8, 0, n(s[1:]) - 600), np.linspace(1, 4, 600)]))
                   for _ in range(2)])      # per frame 600 values above the rest, about 360 of them over the threshold
    out["kitti"] = _case(rng, s, 500, hm, vel=True, score_thresh=0.9, distinct=True,
                         limit=[5.0, -2.0, -1.8, 65.0, 70.0, 0.2])
    s = (1, 2, 190, 175)        # 9 first-round lists, K = 1024 merges 8: a middle round
    out["middle_round"] = _case(rng, s, 1024, rng.normal(-2.0, 1.5, n(s)), score_thresh=0.2, distinct=True)
    s = (1, 3, 60, 50)          # two first-round lists; every winner sits in the first
    out["constant"] = _case(rng, s, 100, np.full(n(s), -1.5), score_thresh=0.1)
    s = (2, 2, 6, 9)
    hm = _spread(rng, n(s), -5, -1).reshape(2, -1)
    hm[:, 3:7] = [2.0, 1.5, 1.0, 0.5]
    hm[0, 20:60:3] = 0.25       # 14 equal values after 4 larger ones: ranks 5..18 around K = 10
    hm[1, 80:100] = 0.25
    out["tie_across_k"] = _case(rng, s, 10, hm, vel=True)
    s = (1, 2, 6, 8)
    hm = -np.abs(rng.normal(1.0, 1.0, n(s))) - 0.01
    hm[5:60:5] = 0.0
    hm[10:60:10] = -0.0         # the zeros tie whatever their sign: index order
    out["signed_zeros"] = _case(rng, s, 16, hm, score_thresh=0.4)
    s = (2, 3, 5, 7)
    out["all_negative"] = _case(rng, s, 12, _spread(rng, n(s), -9, -0.5), score_thresh=0.05, distinct=True)
    s = (1, 2, 6, 6)
    hm = _spread(rng, n(s), 105, 120) * np.where(np.arange(n(s)) % 3 == 0, 1, -1).astype(F32)
    out["saturated"] = _case(rng, s, 36, hm, score_thresh=0.1)
    s = (2, 2, 8, 9)
    hm = np.concatenate([_spread(rng, n(s) // 2, -9, -3), _spread(rng, n(s) // 2, 1, 5)])
    out["none_and_all"] = _case(rng, s, 20, hm, vel=True, score_thresh=0.1, distinct=True)   # frame 0: none, 1: all
    s = (1, 1, 6, 7)
    case = _case(rng, s, 8, _spread(rng, n(s), -4, 3), score_thresh=None, limit=[-5.0, -9.0, -2.0, 9.0, 9.0, 0.5],
                 distinct=True, z_on_limit=True)
    best = select(case["hm"], 8)[0] % 42
    z = case["center_z"].reshape(-1)
    z[best[:4]] = [F32(0.5), np.nextafter(F32(0.5), F32(1)), F32(-2.0), np.nextafter(F32(-2.0), F32(-3))]
    out["z_on_limit"] = case
    return out


def check_margins(table):
    """Asserts, on the restatement alone, that no case can be decided by a rounding: every selected row's float64 score
    is at least SCORE_MARGIN (relative) away from the threshold (raw cases: the others compare given numbers), and every
    x and y at least XY_MARGIN away from its limits (z is a copied number and may sit exactly on one).  Returns the
    smallest two margins seen."""
    worst_s, worst_xy = np.inf, np.inf
    for name, case in table.items():
        got = decode_case(case)
        if case["score_thresh"] is not None and case["raw"]:
            t = float(F32(case["score_thresh"]))
            rel = np.abs(got["score64"] - t) / t
            assert rel.min() >= SCORE_MARGIN, (name, rel.min())
            worst_s = min(worst_s, rel.min())
        lim = np.asarray(case["limit"], np.float64)
        xy = got["boxes"][..., :2].astype(np.float64)
        gap = min(np.abs(xy - lim[0:2]).min(), np.abs(xy - lim[3:5]).min())
        assert gap >= XY_MARGIN, (name, gap)
        worst_xy = min(worst_xy, gap)
    return worst_s, worst_xy


def top_sigmoids_distinct(case):
    """True when, in every frame, the float32 sigmoids (torch's, on the CPU) of the best 2K values are pairwise distinct."""
    import torch
    sig = torch.from_numpy(case["hm"]).sigmoid().flatten(1)
    m = min(2 * case["k"], sig.shape[1])
    top = torch.topk(sig, m, dim=1)[0].numpy()
    return all(len(np.unique(top[f])) == m for f in range(top.shape[0]))


def ulp_error(got32, want64):
    """Largest error of float32 `got32` against float64 `want64` in units of the float32 spacing at |want64| (the
    spacing of the smallest normal below it): 0.5 is what a correctly rounded result reaches."""
    got = np.asarray(got32, np.float64).reshape(-1)
    want = np.asarray(want64, np.float64).reshape(-1)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all() and np.isfinite(want).all()
    mag = np.maximum(np.abs(want), float(np.finfo(F32).tiny))
    ulp = 2.0 ** (np.floor(np.log2(mag)) - 23)
    return float((np.abs(got - want) / ulp).max())
