"""Numpy restatement of the two static-capacity voxel-row ops (include/spx.h §19, csrc/voxel_rows.hip): what the GPU
tests compare the kernels with, bit for bit.  float32 throughout, one rounding per operation, sums in point order."""
import numpy as np

OUT_OF_GRID = -9          # SPX_ERR_OUT_OF_GRID


def table_build(indices, n_live, batch, shape3):
    """indices (cap, 4) int32 (b, z, y, x), n_live live rows (None: all) -> (table (batch, Z, Y, X) int32 with the row of
    every live row at its cell and -1 elsewhere, status: 0 or OUT_OF_GRID when a live row lies outside the table).
    Rows at or beyond n_live are not read."""
    cap = indices.shape[0]
    n_live = cap if n_live is None else min(int(n_live), cap)
    dims = np.array([batch] + [int(s) for s in shape3], dtype=np.int64)
    table = np.full(tuple(dims), -1, dtype=np.int32)
    live = indices[:n_live].astype(np.int64)
    ok = ((live >= 0) & (live < dims)).all(axis=1)
    rows = np.nonzero(ok)[0]
    table[tuple(live[rows].T)] = rows.astype(np.int32)
    return table, (0 if bool(ok.all()) else OUT_OF_GRID)


def point_cells(new_xyz, shape3, range_lo, voxel_size):
    """new_xyz (B, m, 3) -> (cells (B, m, 3) int64 as (z, y, x), inside (B, m) bool): trunc((p - lo) / vs) in float32."""
    lo = np.asarray(range_lo, dtype=np.float32)
    vs = np.asarray(voxel_size, dtype=np.float32)
    f = (new_xyz.astype(np.float32) - lo) / vs
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(f).all(-1)
        c = np.trunc(np.where(np.isfinite(f), f, -1.0)).astype(np.int64)            # (x, y, z)
    dims_xyz = np.array([shape3[2], shape3[1], shape3[0]], dtype=np.int64)
    inside &= (f > -1.0).all(-1) & (c < dims_xyz).all(-1)
    return c[..., ::-1], inside


def rows_mean(new_xyz, feats, table, range_lo, voxel_size, cap, n_live=None, out=None):
    """new_xyz (B, m, 3), feats (B, C, m), table (B, Z, Y, X) -> out (cap, C) float32.  Rows below n_live (None: cap):
    the mean of the cell's points (sum from 0 in ascending point order, times 1 / count) where table[cell] is the row,
    0 elsewhere.  Rows at or beyond n_live keep what `out` held (NaN when no `out` is given)."""
    b, c, m = feats.shape
    n_live = cap if n_live is None else min(int(n_live), cap)
    out = np.full((cap, c), np.nan, dtype=np.float32) if out is None else out.copy()
    out[:n_live] = 0.0
    cells, inside = point_cells(new_xyz, table.shape[1:], range_lo, voxel_size)
    f32 = feats.astype(np.float32)
    for f in range(b):
        sums, counts, order = {}, {}, []
        for i in range(m):
            if not inside[f, i]:
                continue
            key = tuple(cells[f, i])
            if key not in sums:
                sums[key] = np.zeros((c,), dtype=np.float32)
                counts[key] = 0
                order.append(key)
            sums[key] = sums[key] + f32[f, :, i]
            counts[key] += 1
        for key in order:
            row = int(table[(f,) + key])
            if 0 <= row < n_live:
                out[row] = sums[key] * (np.float32(1.0) / np.float32(counts[key]))
    return out


# ---------------------------------------------------------------------------------------------- the shared small case
B, SHAPE, CAP, C, M = 2, (4, 8, 8), 32, 5, 16
LO, VS = (0.0, -4.0, -1.0), (0.5, 1.0, 0.5)          # x in [0, 4), y in [-4, 4), z in [-1, 1)


def _centre(z, y, x, jitter=(0.0, 0.0, 0.0)):
    return [LO[0] + (x + 0.5 + jitter[0]) * VS[0], LO[1] + (y + 0.5 + jitter[1]) * VS[1], LO[2] + (z + 0.5 + jitter[2]) * VS[2]]


def make_case(n_live, seed=0):
    """indices (CAP, 4): every row a distinct in-grid cell (dead rows too: a kernel that reads them marks the table);
    frame 0 owns more live rows than frame 1.  Points: frame 0 has three points in the cell of row 0, two in the cell of
    row 1, one in a cell no row uses (a miss), one outside the grid, one in the cell of a DEAD row; frame 1 the rest."""
    rng = np.random.default_rng(seed)
    lin = rng.permutation(SHAPE[0] * SHAPE[1] * SHAPE[2])[:CAP]        # distinct (z, y, x) whatever the frame
    b = np.where(np.arange(CAP) < 20, 0, 1)                            # 20 rows of frame 0, 12 of frame 1
    idx = np.stack([b, lin // (SHAPE[1] * SHAPE[2]), (lin // SHAPE[2]) % SHAPE[1], lin % SHAPE[2]], 1).astype(np.int32)
    used0 = {tuple(r[1:]) for r in idx if r[0] == 0}
    miss = next((z, y, x) for z in range(SHAPE[0]) for y in range(SHAPE[1]) for x in range(SHAPE[2])
                if (z, y, x) not in used0)
    xyz = np.zeros((B, M, 3), dtype=np.float32)
    rows0 = [r for r in range(CAP) if idx[r, 0] == 0]
    rows1 = [r for r in range(CAP) if idx[r, 0] == 1]
    plan0 = [rows0[0], rows0[1], rows0[0], None, rows0[2], rows0[1], "out", rows0[0], rows0[-1], rows0[3], "neg"]
    for i in range(M):
        what = plan0[i] if i < len(plan0) else rows0[4 + i % 5]
        if what is None:
            xyz[0, i] = _centre(*miss)
        elif what == "out":
            xyz[0, i] = [LO[0] + SHAPE[2] * VS[0] + 0.25, 0.0, 0.0]   # beyond the last x cell
        elif what == "neg":
            xyz[0, i] = [LO[0] - 1.25 * VS[0], 0.0, 0.0]              # below the grid
        else:
            xyz[0, i] = _centre(*idx[what, 1:], jitter=tuple(rng.uniform(-0.4, 0.4, 3)))
        xyz[1, i] = _centre(*idx[rows1[i % 7], 1:], jitter=tuple(rng.uniform(-0.4, 0.4, 3)))
    feats = rng.standard_normal((B, C, M)).astype(np.float32)
    return idx, xyz, feats, n_live
