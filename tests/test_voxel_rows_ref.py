"""The numpy restatement of the voxel-row ops (tests/voxel_rows_ref.py) against a brute-force loop over every cell of
the grid, on cases built to hit: two and three points in one cell, a cell that is not active, a point outside the grid,
live count 0, live count equal to the capacity, frames with different live counts.  No GPU."""
import numpy as np
import pytest

import voxel_rows_ref as vr

B, SHAPE, CAP, C, M, LO, VS = vr.B, vr.SHAPE, vr.CAP, vr.C, vr.M, vr.LO, vr.VS
make_case = vr.make_case


def _brute(idx, xyz, feats, n_live):
    """Every cell of the grid in turn: its points, their mean, its row."""
    n_live = CAP if n_live is None else n_live
    table = np.full((B,) + SHAPE, -1, dtype=np.int32)
    for r in range(n_live):
        table[tuple(idx[r])] = r
    out = np.full((CAP, C), np.nan, dtype=np.float32)
    out[:n_live] = 0
    lo, vs = np.float32(LO), np.float32(VS)
    for b in range(B):
        for z in range(SHAPE[0]):
            for y in range(SHAPE[1]):
                for x in range(SHAPE[2]):
                    members = []
                    for i in range(M):
                        q = (xyz[b, i] - lo) / vs
                        if all(q > -1.0) and tuple(int(v) for v in q) == (x, y, z):
                            members.append(i)
                    row = table[b, z, y, x]
                    if not members or row < 0:
                        continue
                    s = np.zeros((C,), dtype=np.float32)
                    for i in members:
                        s = s + feats[b, :, i]
                    out[row] = s * (np.float32(1.0) / np.float32(len(members)))
    return table, out


@pytest.mark.parametrize("n_live", [0, CAP, 25, 20, 7, None])
def test_restatement_matches_brute_force(n_live):
    idx, xyz, feats, n_live = make_case(n_live)
    table, status = vr.table_build(idx, n_live, B, SHAPE)
    want_table, want = _brute(idx, xyz, feats, n_live)
    assert status == 0
    assert np.array_equal(table, want_table)
    got = vr.rows_mean(xyz, feats, table, LO, VS, CAP, n_live)
    assert np.array_equal(got, want, equal_nan=True)
    live = CAP if n_live is None else n_live
    assert np.isnan(got[live:]).all() and np.isfinite(got[:live]).all()


def test_case_hits_what_it_was_built_for():
    idx, xyz, feats, _ = make_case(7)
    cells, inside = vr.point_cells(xyz, SHAPE, LO, VS)
    assert not inside[0, 6] and not inside[0, 10] and inside[0, :6].all()          # the two outside points
    keys0 = [tuple(c) for c in cells[0]]
    assert keys0.count(keys0[0]) == 3 and keys0.count(keys0[1]) == 2                # three and two points in a cell
    table, _ = vr.table_build(idx, 7, B, SHAPE)
    assert table[(0,) + keys0[3]] == -1                                             # the miss: no row has this cell
    assert not any(tuple(r[1:]) == keys0[3] for r in idx if r[0] == 0)
    assert tuple(idx[19, 1:]) == keys0[8] and table[(0,) + keys0[8]] == -1          # the cell of a dead row
    assert (table[1] == -1).all()                                                   # frame 1 has no live row at 7
    assert vr.table_build(idx, CAP, B, SHAPE)[0][(0,) + keys0[8]] == 19


def test_out_of_grid_live_row_is_skipped_and_reported():
    idx, _, _, _ = make_case(CAP)
    bad = idx.copy()
    bad[3, 2] = SHAPE[1]                                                            # y one past the grid
    table, status = vr.table_build(bad, CAP, B, SHAPE)
    good, _ = vr.table_build(idx, CAP, B, SHAPE)
    assert status == vr.OUT_OF_GRID
    good[tuple(idx[3])] = -1
    assert np.array_equal(table, good)
    assert vr.table_build(bad, 3, B, SHAPE)[1] == 0                                 # dead: never read
