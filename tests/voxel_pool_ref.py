"""A numpy restatement of the voxel-grid pooling ops (include/spx.h §27), in any numpy dtype: float64 for comparisons with
a tolerance, int64 for bit-exact ones.  Not a test module.

Exact use: coordinates on a half-integer lattice are passed DOUBLED as int64 (xyz2 = 2 xyz, new_xyz2 = 2 new_xyz) with f2 =
2 f, b2 = 2 b and integer A; then max_fwd returns 2 out, max_bwd returns (df, 2 dA, db) and moments returns (2 sum d,
4 sum d d^T), every one an exact integer.

The association follows the header: v = f + (((A0 dx + A1 dy) + A2 dz) + b); the winner is the lowest slot that attains
the maximum; an empty query has d = 0 and f = 0 in every slot."""
import numpy as np


def offsets(xyz, new_xyz, idx, empty, dtype):
    """d (M, S, 3): xyz[idx] - new_xyz subtracted in the inputs' own dtype (float32 for the op's inputs), then promoted;
    0 for empty queries, whose idx is not used."""
    idx = np.where(empty[:, None], 0, idx)
    d = (xyz[idx] - new_xyz[:, None, :]).astype(dtype)
    d[empty] = 0
    return d


def moments(xyz, new_xyz, idx, empty, dtype=np.float64):
    d = offsets(xyz, new_xyz, idx, empty, dtype).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.array([x.sum(), y.sum(), z.sum(), (x * x).sum(), (x * y).sum(), (x * z).sum(), (y * y).sum(), (y * z).sum(),
                     (z * z).sum()], dtype=dtype)


def values(f, xyz, new_xyz, idx, empty, a, b, dtype=np.float64):
    """v (M, S, C)"""
    d = offsets(xyz, new_xyz, idx, empty, dtype)
    a, b = a.astype(dtype), b.astype(dtype)
    idx = np.where(empty[:, None], 0, idx)
    fv = f.astype(dtype)[idx]                                   # (M, S, C)
    fv[empty] = 0
    t = ((d[:, :, None, 0] * a[None, None, :, 0] + d[:, :, None, 1] * a[None, None, :, 1])
         + d[:, :, None, 2] * a[None, None, :, 2]) + b[None, None, :]
    return fv + t


def max_fwd(f, xyz, new_xyz, idx, empty, a, b, dtype=np.float64):
    v = values(f, xyz, new_xyz, idx, empty, a, b, dtype)
    arg = v.argmax(axis=1)                                      # first occurrence = lowest slot
    best = np.take_along_axis(v, arg[:, None, :], axis=1)[:, 0, :]
    pos = best > 0
    return np.where(pos, best, 0).astype(dtype), np.where(pos, arg, -1).astype(np.int32)


def top2_gap(f, xyz, new_xyz, idx, empty, a, b):
    """Per (m, c): the float64 maximum minus the largest value among slots that point at ANOTHER row (inf when there is
    none), and the largest |v|.  Empty queries: inf."""
    v = values(f, xyz, new_xyz, idx, empty, a, b, np.float64)
    arg = v.argmax(axis=1)
    best = np.take_along_axis(v, arg[:, None, :], axis=1)[:, 0, :]
    win_row = np.take_along_axis(idx, arg.reshape(arg.shape[0], -1), axis=1).reshape(arg.shape)   # (M, C)
    other = idx[:, :, None] != win_row[:, None, :]              # (M, S, C)
    second = np.where(other, v, -np.inf).max(axis=1)
    gap = best - second
    gap[empty] = np.inf
    return gap, np.abs(v).max()


def max_bwd(dout, arg, idx, empty, xyz, new_xyz, n_src, dtype=np.float64):
    m, c = dout.shape
    live = arg >= 0
    g = np.where(live, dout.astype(dtype), 0)
    slot = np.clip(arg, 0, None)
    d = offsets(xyz, new_xyz, idx, empty, dtype)                # (M, S, 3)
    d_win = d[np.arange(m)[:, None], slot]                      # (M, C, 3)
    da = np.einsum('mc,mcj->cj', g, d_win)
    db = g.sum(axis=0)
    df = np.zeros((n_src, c), dtype=dtype)
    rows = np.where(empty[:, None], 0, idx)[np.arange(m)[:, None], slot]            # (M, C)
    to_f = live & ~empty[:, None]
    mm, cc = np.nonzero(to_f)
    np.add.at(df, (rows[mm, cc], cc), g[mm, cc])
    return df, da, db


def random_lists(rng, m, nsample, n_src, p_empty=0.2):
    """idx (M, S) int32 and empty (M) bool shaped like voxel_query's output: k in [1, S] found rows, the rest of the list
    padded by repeating the first; empty queries hold zeros."""
    idx = rng.integers(0, n_src, size=(m, nsample)).astype(np.int32)
    k = rng.integers(1, nsample + 1, size=m)
    pad = np.arange(nsample)[None, :] >= k[:, None]
    idx = np.where(pad, idx[:, :1], idx)
    empty = rng.random(m) < p_empty
    idx[empty] = 0
    return idx, empty


def float_case(c, seed, m=2049, nsample=16, n_src=300):
    """float32 inputs shaped like one pooling level: voxel centres tens of metres from the origin, queries within a
    fraction of a metre of their first neighbour."""
    rng = np.random.default_rng(seed)
    idx, empty = random_lists(rng, m, nsample, n_src)
    xyz = (rng.normal(size=(n_src, 3)) * 2 + np.array([30.0, -5.0, 1.0])).astype(np.float32)
    new_xyz = (xyz[idx[:, 0]] + rng.normal(size=(m, 3)) * 0.4).astype(np.float32)
    return dict(idx=idx, empty=empty, xyz=xyz, new_xyz=new_xyz, f=rng.normal(size=(n_src, c)).astype(np.float32),
                a=(rng.normal(size=(c, 3)) * 0.5).astype(np.float32), b=(rng.normal(size=(c,)) * 0.2).astype(np.float32),
                dout=rng.normal(size=(m, c)).astype(np.float32))


FLOAT_CASES = ((32, 101), (64, 102))          # (channels, seed)
ARG_GAP = 1e-5                                # of the largest |v|: below it float32 may pick the other row


def decided_pairs(case):
    """(m, c) pairs whose winner float32 must reproduce: the float64 top-two gap between distinct rows, and the distance
    of the maximum from 0 (where arg flips to -1), both exceed ARG_GAP of the largest value."""
    gap, vmax = top2_gap(case["f"], case["xyz"], case["new_xyz"], case["idx"], case["empty"], case["a"], case["b"])
    v = values(case["f"], case["xyz"], case["new_xyz"], case["idx"], case["empty"], case["a"], case["b"])
    return (gap > ARG_GAP * vmax) & (np.abs(v.max(axis=1)) > ARG_GAP * vmax)


def voxel_query_bruteforce(max_range, radius, nsample, xyz, new_xyz, new_coords, table):
    """voxel_query_utils.voxel_query in numpy (csrc/voxel_query.hip): the cells within max_range = (z, y, x) of new_coords
    (b, z, y, x) are scanned in ascending z, y, x; a voxel whose centre is within radius (float32: (dx dx + dy dy) + dz dz
    <= r r) joins the list.  Lists are padded by cycling from their start; density = occupied cells scanned / cells in the
    range.  Valid only while no ball holds more than nsample voxels (asserted): the reservoir step never runs, so the
    lists are the scan order.  -> idx (M, nsample) int32, empty (M) bool, density (M, 1) float32."""
    xyz, new_xyz = np.asarray(xyz, np.float32), np.asarray(new_xyz, np.float32)
    table, new_coords = np.asarray(table), np.asarray(new_coords)
    zr, yr, xr = [int(v) for v in max_range]
    b_n, z_n, y_n, x_n = table.shape
    r2 = np.float32(radius) * np.float32(radius)
    m = new_xyz.shape[0]
    idx = np.zeros((m, nsample), np.int32)
    empty = np.zeros(m, bool)
    cnt = np.zeros((m, 1), np.float32)
    for p in range(m):
        b, z, y, x = [int(v) for v in new_coords[p]]
        found = []
        if 0 <= b < b_n:
            block = table[b, max(z - zr, 0):max(min(z + zr + 1, z_n), 0), max(y - yr, 0):max(min(y + yr + 1, y_n), 0),
                          max(x - xr, 0):max(min(x + xr + 1, x_n), 0)].reshape(-1)      # C order = ascending z, y, x
            rows = block[block >= 0]
            cnt[p, 0] = len(rows)
            d = xyz[rows] - new_xyz[p]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            found = list(rows[d2 <= r2])
        assert len(found) <= nsample, "a ball holds more than nsample voxels: the reservoir draw would run"
        if not found:
            empty[p] = True
            continue
        idx[p] = [found[l % len(found)] for l in range(nsample)]
    volume = (xr * 2 + 1) * (yr * 2 + 1) * (zr * 2 + 1)
    return idx, empty, cnt / np.float32(volume)
