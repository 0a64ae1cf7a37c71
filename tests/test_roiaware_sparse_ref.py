"""tests/roiaware_sparse_ref.py (the restatement the HIP op of include/spx.h §30 is compared with, bit for bit) against a
brute-force scalar loop written from the semantics: every edge of the emit rule, caps of 1 and 2 kept points, an RoI
without points, two identical RoIs, a frame without points, a zero-score cell, the fake branch at 0, 1 and 2 cells,
static capacity and overflow, the fixed-order backward, and the ragged points-in-boxes."""
import numpy as np
import pytest

import roiaware_sparse_ref as sref
from part_a2_scenes import grid_scene as _grid_scene, scene as _scene

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ brute force

def _inside_cell(box, xyz, out_size):
    """One point against one box, scalar float32 steps: -> linear cell, or -1 outside."""
    cx, cy, cz, dx, dy, dz, rz = (F32(v) for v in box)
    x, y, z = (F32(v) for v in xyz)
    if F64(abs(F32(z - cz))) > F64(dz) / 2.0:
        return -1
    cosa, sina = F32(np.cos(-F64(rz))), F32(np.sin(-F64(rz)))
    sx, sy = F32(x - cx), F32(y - cy)
    lx = F32(F32(sx * cosa) + F32(sy * F32(-sina)))
    ly = F32(F32(sx * sina) + F32(sy * cosa))
    margin = F64(F32(1e-5))
    if not (F64(abs(lx)) < F64(dx) / 2.0 + margin and F64(abs(ly)) < F64(dy) / 2.0 + margin):
        return -1
    idx = []
    for l, d, o in ((lx, dx, out_size[0]), (ly, dy, out_size[1]), (F32(z - cz), dz, out_size[2])):
        with np.errstate(all="ignore"):
            f = F32(F32(l + F32(d / F32(2))) / F32(d / F32(o)))
        i = 0 if np.isnan(f) else int(np.clip(np.trunc(F64(f)), -2147483648.0, 2147483647.0))
        idx.append(min(i & 0xFFFFFFFF, o - 1))
    return (idx[0] * out_size[1] + idx[1]) * out_size[2] + idx[2]


def brute(rois, points, cnt, part, rpn, out_size, max_pts, rows=None):
    rois, points, part, rpn = (np.asarray(a, F32) for a in (rois, points, part, rpn))
    b, n = rois.shape[:2]
    c = rpn.shape[1]
    V = int(np.prod(out_size))
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(int)
    kept = []                                                   # per RoI row: cell -> global point rows, ascending
    for r in range(b * n):
        f = r // n
        cells = {}
        for p in range(starts[f], starts[f] + int(cnt[f])):
            v = _inside_cell(rois[f, r % n], points[p, 1:4], out_size)
            if v >= 0 and len(cells.setdefault(v, [])) < max_pts - 1:
                cells[v].append(p)
        kept.append({v: L for v, L in cells.items() if L})
    def pooled(r, v):
        L = kept[r].get(v, [])
        avg = np.zeros(4, F32)
        if L:
            s = np.zeros(4, F32)
            for p in L:
                s = s + part[p]
            avg = s / F32(len(L))
        best, arg = np.zeros(c, F32), np.full(c, -1, np.int32)
        for ch in range(c):
            cur, am = F32(-np.inf), -1
            for p in L:
                if rpn[p, ch] > cur:
                    cur, am = rpn[p, ch], p
            if am >= 0:
                best[ch], arg[ch] = cur, am
        return avg, best, arg, len(L)
    emitted = []
    for r in range(b * n):
        for v in sorted(kept[r]):
            avg = pooled(r, v)[0]
            if F32(F32(F32(avg[0] + avg[1]) + avg[2]) + avg[3]) != 0:
                emitted.append((r, v))
    faked = len(emitted) < 3
    if faked:
        emitted = [(r, 0) for r in range(b * n)]
    cap = len(emitted) if rows is None else rows
    out = {"n_rows": len(emitted), "faked": int(faked), "coords": np.full((cap, 4), -1, np.int32),
           "part": np.zeros((cap, 4), F32), "rpn": np.zeros((cap, c), F32), "arg": np.full((cap, c), -1, np.int32),
           "cnt": np.zeros(cap, np.int32), "row_of_cell": np.full(b * n * V, -1, np.int32), "kept": kept}
    oy, oz = out_size[1], out_size[2]
    for row, (r, v) in enumerate(emitted[:cap]):
        out["coords"][row] = (r, v // (oy * oz), (v // oz) % oy, v % oz)
        out["part"][row], out["rpn"][row], out["arg"][row], out["cnt"][row] = pooled(r, v)
        out["row_of_cell"][r * V + v] = row
    return out


def brute_bwd(fwd, grad, n_points, n_per, V, mode):
    g = np.asarray(grad, F32)
    gi = np.zeros((n_points, g.shape[1]), F32)
    for p in range(n_points):
        for ch in range(g.shape[1]):
            acc = F32(0)
            for r, cells in enumerate(fwd["kept"]):                       # ascending r; other frames never list p
                for v, L in cells.items():
                    row = fwd["row_of_cell"][r * V + v]
                    if p in L and row >= 0:
                        if mode == 0:
                            if fwd["arg"][row, ch] == p:
                                acc = F32(acc + g[row, ch])
                        else:
                            acc = F32(acc + F32(g[row, ch] * F32(F32(1) / F32(max(fwd["cnt"][row], 1)))))
            gi[p, ch] = acc
    return gi


def _same(got, want, keys=("coords", "part", "rpn", "arg", "cnt", "row_of_cell")):
    assert got["n_rows"] == want["n_rows"] and got["faked"] == want["faked"]
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------------ scenes

@pytest.mark.parametrize("cnt,n,out_size,max_pts", [
    ((130, 63), 5, (2, 3, 4), 128),
    ((130, 63), 5, (4, 4, 4), 3),          # a cap of 2 kept points
    ((90, 77), 3, (2, 2, 2), 2),           # a cap of 1 kept point
    ((0, 77), 2, (3, 3, 3), 4),            # a frame with 0 points
    ((40, 0), 1, (2, 2, 2), 128),
])
def test_restatement_equals_brute_force(cnt, n, out_size, max_pts):
    rois, pts, cnt, part, rpn = _scene(3, cnt, n)
    got = sref.pool(rois, pts, cnt, part, rpn, out_size, max_pts)
    want = brute(rois, pts, cnt, part, rpn, out_size, max_pts)
    _same(got, want)
    assert got["n_rows"] >= 3 and not got["faked"]
    rng = np.random.default_rng(1)
    V = int(np.prod(out_size))
    for mode, ch in ((0, rpn.shape[1]), (1, 4)):
        g = rng.integers(-4, 5, size=(got["n_rows"], ch)).astype(F32) if mode == 0 else \
            rng.normal(size=(got["n_rows"], ch)).astype(F32)
        gi = sref.pool_bwd(got, g, pts.shape[0], n, mode)
        assert np.array_equal(gi, brute_bwd(want, g, pts.shape[0], n, V, mode))


def test_roi_without_points_identical_rois_and_other_frames_points():
    rois, pts, cnt, part, rpn = _scene(5, (60, 50), 3)
    rois[0, 1] = rois[0, 0]                                     # two identical RoIs: identical rows, both emitted
    rois[1, 2, :3] = 100.0                                      # an RoI without points
    rois[1, 0] = rois[0, 0]                                     # frame 0's box in frame 1: sees frame 1's points only
    got = sref.pool(rois, pts, cnt, part, rpn, (3, 3, 3), 128)
    _same(got, brute(rois, pts, cnt, part, rpn, (3, 3, 3), 128))
    r = got["coords"][:, 0]
    assert (r == 0).sum() > 0 and (r == 5).sum() == 0
    a, b = got["coords"][r == 0], got["coords"][r == 1]
    assert np.array_equal(a[:, 1:], b[:, 1:]) and np.array_equal(got["rpn"][r == 0], got["rpn"][r == 1])
    assert (got["arg"][r == 3] >= 60).all()                     # global rows of frame 1
    assert np.array_equal(got["coords"], got["coords"][np.lexsort(got["coords"].T[::-1])])   # ascending (r, x, y, z)


def test_emit_rule_edges_and_zero_score_cell():
    rois, pts, cnt, part, rpn = _grid_scene(cells=(0, 3, 5, 6), zero_cells=(1, 7))
    got = sref.pool(rois, pts, cnt, part, rpn, (2, 2, 2), 128)
    _same(got, brute(rois, pts, cnt, part, rpn, (2, 2, 2), 128))
    assert got["n_rows"] == 4 and not got["faked"]
    assert [tuple(c) for c in got["coords"]] == [(0, 0, 0, 0), (0, 0, 1, 1), (0, 1, 0, 1), (0, 1, 1, 0)]
    assert got["row_of_cell"][1] == -1 and got["row_of_cell"][7] == -1      # points, but an exactly zero sum
    assert got["row_of_cell"][2] == -1                                       # no point
    # one point of a zero-score cell gets a non-zero offset: the cell is emitted
    part[4, 2] = 1e-30
    again = sref.pool(rois, pts, cnt, part, rpn, (2, 2, 2), 128)
    assert again["n_rows"] == 5 and again["row_of_cell"][1] == 1
    # a mixed cell: a zero point and a non-zero point average to non-zero
    pts2 = np.concatenate([pts, pts[4:5]])
    part2 = np.concatenate([part * 0 + part, np.asarray([[0, 0.25, 0, 0]], F32)])
    part2[4] = 0
    mixed = sref.pool(rois, pts2, np.asarray([7], np.int32), part2, np.concatenate([rpn, rpn[:1]]), (2, 2, 2), 128)
    _same(mixed, brute(rois, pts2, np.asarray([7], np.int32), part2, np.concatenate([rpn, rpn[:1]]), (2, 2, 2), 128))
    assert mixed["row_of_cell"][1] >= 0 and mixed["cnt"][mixed["row_of_cell"][1]] == 2


@pytest.mark.parametrize("cells", [(), (5,), (0, 6)])
def test_fake_branch_at_0_1_and_2_cells(cells):
    rois, pts, cnt, part, rpn = _grid_scene(cells=cells, zero_cells=(3,), n_rois=3)
    got = sref.pool(rois, pts, cnt, part, rpn, (2, 2, 2), 128)
    _same(got, brute(rois, pts, cnt, part, rpn, (2, 2, 2), 128))
    assert got["faked"] == 1 and got["n_rows"] == 3
    assert [tuple(c) for c in got["coords"]] == [(0, 0, 0, 0), (1, 0, 0, 0), (2, 0, 0, 0)]
    assert np.array_equal(got["row_of_cell"].reshape(3, 8)[:, 0], [0, 1, 2]) and (got["row_of_cell"].reshape(3, 8)[:, 1:] == -1).all()
    if 0 in cells:                                               # the fake row holds cell 0's pooled values
        assert got["cnt"][0] == 1 and got["part"][0, 0] == F32(0.5) and got["arg"][0, 0] == 0
    else:
        assert got["cnt"][0] == 0 and not got["part"][0].any() and (got["arg"][0] == -1).all()
    assert not got["part"][1:].any() and not got["rpn"][1:].any()
    g = np.ones((3, 2), F32)
    gi = sref.pool_bwd(got, g, pts.shape[0], 3, 0)
    assert np.array_equal(gi, brute_bwd(brute(rois, pts, cnt, part, rpn, (2, 2, 2), 128), g, pts.shape[0], 3, 8, 0))
    assert gi.any() == (0 in cells)


def test_three_cells_is_not_faked():
    rois, pts, cnt, part, rpn = _grid_scene(cells=(1, 2, 4))
    got = sref.pool(rois, pts, cnt, part, rpn, (2, 2, 2), 128)
    assert got["faked"] == 0 and got["n_rows"] == 3


def test_static_capacity_dead_rows_and_overflow():
    rois, pts, cnt, part, rpn = _scene(7, (130, 63), 5)
    exact = sref.pool(rois, pts, cnt, part, rpn, (2, 3, 4), 4)
    n = exact["n_rows"]
    big = sref.pool(rois, pts, cnt, part, rpn, (2, 3, 4), 4, rows=n + 9)
    _same(big, brute(rois, pts, cnt, part, rpn, (2, 3, 4), 4, rows=n + 9))
    assert not big["overflow"] and (big["coords"][n:] == -1).all() and not big["part"][n:].any() \
        and not big["rpn"][n:].any() and (big["arg"][n:] == -1).all() and not big["cnt"][n:].any()
    for k in ("coords", "part", "rpn", "arg", "cnt"):
        assert np.array_equal(big[k][:n], exact[k])
    small = sref.pool(rois, pts, cnt, part, rpn, (2, 3, 4), 4, rows=n - 5)
    _same(small, brute(rois, pts, cnt, part, rpn, (2, 3, 4), 4, rows=n - 5))
    assert small["overflow"] and small["n_rows"] == n and small["row_of_cell"].max() == n - 6
    g = np.ones((n - 5, 3), F32)
    assert np.array_equal(sref.pool_bwd(small, g, pts.shape[0], 5, 0),
                          brute_bwd(brute(rois, pts, cnt, part, rpn, (2, 3, 4), 4, rows=n - 5), g, pts.shape[0], 5, 24, 0))


def test_points_in_boxes_stack_ragged_first_hit_and_bad_frames():
    rois, pts, cnt, _, _ = _scene(11, (130, 63, 0, 20), 4)
    rois[1, 1] = rois[1, 0]                                     # the first of two equal boxes wins
    pts = np.concatenate([pts, np.asarray([[-1, 0, 0, 0], [4, 0, 0, 0], [np.nan, 0, 0, 0]], F32)])
    got = sref.points_in_boxes_stack(pts, rois)
    want = np.full(pts.shape[0], -1, np.int32)
    for p in range(pts.shape[0]):
        f = pts[p, 0]
        if not (f >= 0 and f < 4):
            continue
        for k in range(4):
            if _inside_cell(rois[int(f), k], pts[p, 1:4], (1, 1, 1)) >= 0:
                want[p] = k
                break
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (got >= 0).sum() > 50 and (got[-3:] == -1).all() and not (got[130:193] == 1).any()
    perm = np.random.default_rng(0).permutation(pts.shape[0])
    assert np.array_equal(sref.points_in_boxes_stack(pts[perm], rois), want[perm])


def test_limits_are_refused_on_the_host():
    """The limits include/spx.h §30 states: refused with SPX_ERR_TOO_LARGE before any launch (no GPU needed)."""
    import ctypes
    from spx import _lib
    lib = _lib.load()
    buf = ctypes.addressof((ctypes.c_int64 * 8)())
    args = lambda b, n, pf, o: (buf,) * 4 + (b, n, 10, pf, o, o, o, 4) + (buf,) * 4 + (1 << 40, None)
    assert lib.spx_roiaware_sparse_collect(*args(257, 1, 10, 2)) == -5             # frames
    assert lib.spx_roiaware_sparse_collect(*args(2, (1 << 19) + 1, 10, 2)) == -5   # RoI rows of the one-launch scan
    assert lib.spx_roiaware_sparse_collect(*args(2, 1 << 10, 10, 255)) == -5       # cells
    assert lib.spx_roiaware_sparse_collect(*args(1, 1, 1 << 29, 2)) == -5          # points
    assert lib.spx_roiaware_sparse_collect(*args(1, 1, 10, 256)) == -1
    assert lib.spx_roiaware_sparse_ws_bytes(1, 1, 10, 256, 2, 2) == 0
    assert lib.spx_roiaware_sparse_ws_bytes(2, 5, 193, 2, 3, 4) >= 10 * (3 * 193 + 3 * 24 + 2) * 4
    assert lib.spx_points_in_boxes_stack(buf, buf, 70000, 10, 4, buf, None) == -5
    assert lib.spx_points_in_boxes_stack(None, buf, 2, 10, 4, buf, None) == -1
