"""Float64 numpy restatement of DynamicPillarVFE with one last-layer PFNLayerV2 (reference
pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:14-142): pillarisation, forward in both modes and parameter gradients,
plus the case generator of tests/test_gpu_dyn_pillar_vfe.py.  The [K, C_out] activations over the K kept points are built
densely here: the kernel's algebra (include/spx.h §24) is not restated, so the two check each other.

Cells are taken in float32 (the subtraction and the division rounded separately), pillars with np.unique.  A point is
kept iff its x / y cell is on the grid; z is not tested; a NaN coordinate or a batch index outside [0, batch) drops it.
Selection: arg[m, c] is the row in `points` of the first point of pillar m, in ascending row order, whose relu(z[:, c])
attains the pillar's maximum; active[m, c] = out[m, c] > 0.  backward() takes an optional (arg, active) override, so that
the gradient can be evaluated for the winners another implementation chose."""
import numpy as np

VOXEL = (0.16, 0.16, 4.0)
NX, NY, BATCH = 16, 12, 2
RANGE = (0.0, 0.0, -3.0, NX * VOXEL[0], NY * VOXEL[1], 1.0)
MOMENTUM, EPS = 0.01, 1e-3
C_OUT = 64


def offsets(voxel=VOXEL, range_lo=RANGE[:3]):
    return tuple(v / 2 + lo for v, lo in zip(voxel, range_lo))


def c_in_of(c, use_abs, with_dist):
    return (c + 6 if use_abs else c + 3) + (1 if with_dist else 0)


def grid_of(rng, voxel):
    return [int(round((rng[3 + j] - rng[j]) / voxel[j])) for j in range(2)]


def pillarize(points, rng=RANGE, voxel=VOXEL, batch=BATCH, cap=None):
    """points [N, 1 + C] float32 (batch, x, y, z, ...) -> dict(coords [M, 4] (b, 0, cy, cx), inverse [N] (-1 dropped),
    count [M], offset [M + 1], order [K], num_pillars (the true count, may exceed cap), num_points, cells [N, 2])."""
    points = np.asarray(points, np.float32)
    n = points.shape[0]
    gx, gy = grid_of(rng, voxel)
    with np.errstate(invalid="ignore"):
        fx = np.floor((points[:, 1] - np.float32(rng[0])) / np.float32(voxel[0]))
        fy = np.floor((points[:, 2] - np.float32(rng[1])) / np.float32(voxel[1]))
        keep = (fx >= 0) & (fx < gx) & (fy >= 0) & (fy < gy) & (points[:, 0] >= 0) & (points[:, 0] < batch)
    cx = np.where(keep, fx, 0).astype(np.int64)
    cy = np.where(keep, fy, 0).astype(np.int64)
    b = np.where(keep, points[:, 0], 0).astype(np.int64)
    key = (b * gx + cx) * gy + cy
    unq, inv_k = np.unique(key[keep], return_inverse=True)
    true_m = unq.shape[0]
    m = true_m if cap is None else min(true_m, int(cap))
    inverse = np.full(n, -1, np.int64)
    inverse[keep] = inv_k
    inverse[inverse >= m] = -1
    unq = unq[:m]
    coords = np.stack([unq // (gx * gy), np.zeros(m, np.int64), unq % gy, (unq // gy) % gx], 1).astype(np.int32)
    live = np.nonzero(inverse >= 0)[0]
    count = np.bincount(inverse[live], minlength=m).astype(np.int32)
    offset = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    order = live[np.argsort(inverse[live], kind="stable")].astype(np.int32)
    return dict(coords=coords, inverse=inverse.astype(np.int32), count=count, offset=offset, order=order,
                num_pillars=true_m, num_points=int(live.shape[0]), cells=np.stack([cx, cy], 1))


def features(case, pz, center_dtype=np.float64):
    """[K, C_in] float64 over the kept points in ascending row order, and their rows.  center_dtype=float32 forms the
    pillar centre as the float32 composition does (product and sum rounded to float32)."""
    pts = case["points"].astype(np.float64)
    rows = np.nonzero(pz["inverse"] >= 0)[0]
    inv = pz["inverse"][rows].astype(np.int64)
    m = pz["coords"].shape[0]
    voxel, offs = case.get("voxel", VOXEL), case.get("offs", None)
    offs = offsets(voxel, case.get("range", RANGE)[:3]) if offs is None else offs
    xyz = pts[rows, 1:4]
    mean = np.zeros((m, 3))
    np.add.at(mean, inv, xyz)
    mean /= np.maximum(pz["count"], 1)[:, None]
    cd = center_dtype
    cells = pz["coords"][inv][:, [3, 2]]
    ctr = np.stack([(cells[:, j].astype(cd) * cd(voxel[j]) + cd(offs[j])).astype(np.float64) for j in range(2)]
                   + [np.full(rows.shape[0], float(cd(offs[2])))], 1)
    parts = [pts[rows, 1:] if case["use_abs"] else pts[rows, 4:], xyz - mean[inv], xyz - ctr]
    if case["with_dist"]:
        parts.append(np.sqrt((xyz * xyz).sum(1, keepdims=True)))
    return np.concatenate(parts, 1), rows, inv


def forward(case, training=True, center_dtype=np.float64, pz=None):
    pz = pillarize(case["points"], case.get("range", RANGE), case.get("voxel", VOXEL), case.get("batch", BATCH)) \
        if pz is None else pz
    f, rows, inv = features(case, pz, center_dtype)
    k, m = f.shape[0], pz["coords"].shape[0]
    w, gamma, beta = (case[key].astype(np.float64) for key in ("weight", "gamma", "beta"))
    x = f @ w.T                                                  # [K, C_out]
    rm, rv = case["running_mean"].astype(np.float64), case["running_var"].astype(np.float64)
    out = dict(f=f, rows=rows, inv=inv, x=x, pz=pz)
    if training:
        mean = x.mean(0)
        var = x.var(0)                                           # biased
        out["running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
        out["running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * var * k / max(k - 1, 1)
        out["nbt"] = int(case["nbt"]) + 1
    else:
        mean, var = rm, rv
    invstd = 1.0 / np.sqrt(var + EPS)
    z = (x - mean) * invstd * gamma + beta
    y = np.maximum(z, 0.0)
    # rows is ascending and inv follows it, so a stable sort by pillar is `order`'s order
    perm = np.argsort(inv, kind="stable")
    starts = pz["offset"][:-1].astype(np.int64)
    ys = y[perm]
    best = np.maximum.reduceat(ys, starts, axis=0) if m else np.zeros((0, C_OUT))
    seg = inv[perm]
    pos = np.where(ys == best[seg], np.arange(k)[:, None], k)
    first = np.minimum.reduceat(pos, starts, axis=0) if m else np.zeros((0, C_OUT), np.int64)
    out.update(mean=mean, var=var, invstd=invstd, z=z, out=best, perm=perm)
    out["arg"] = rows[perm][first].astype(np.int64)              # rows in `points`
    out["active"] = best > 0
    return out


def ambiguous(fwd):
    """[M, C_out] bool: the float64 top-two gap over the pillar's points, or the top value's distance from 0, is below
    1e-5 max|z|.  A pillar of one point has no gap."""
    z, inv, perm, pz = fwd["z"], fwd["inv"], fwd["perm"], fwd["pz"]
    k = z.shape[0]
    starts = pz["offset"][:-1].astype(np.int64)
    thr = 1e-5 * np.abs(z).max()
    zs = z[perm]
    top = np.maximum.reduceat(zs, starts, axis=0)
    seg = inv[perm]
    pos = np.where(zs == top[seg], np.arange(k)[:, None], k)
    first = np.minimum.reduceat(pos, starts, axis=0)
    rest = zs.copy()
    rest[first, np.arange(z.shape[1])[None, :]] = -np.inf
    second = np.maximum.reduceat(rest, starts, axis=0)
    return ((top - second) < thr) | (np.abs(top) < thr)


def backward(case, fwd, d_out, arg=None, active=None, training=True):
    """(d_weight, d_gamma, d_beta) through the dense [K, C_out] BatchNorm backward."""
    arg = fwd["arg"] if arg is None else np.asarray(arg, np.int64)
    active = fwd["active"] if active is None else np.asarray(active, bool)
    f, x, rows = fwd["f"], fwd["x"], fwd["rows"]
    k = f.shape[0]
    gamma = case["gamma"].astype(np.float64)
    kept_row = np.full(case["points"].shape[0], -1, np.int64)
    kept_row[rows] = np.arange(k)
    g = np.zeros_like(x)
    mi, ci = np.nonzero(active)
    sel = kept_row[arg[mi, ci]]
    assert (sel >= 0).all()
    g[sel, ci] = d_out.astype(np.float64)[mi, ci]
    xhat = (x - fwd["mean"]) * fwd["invstd"]
    d_beta = g.sum(0)
    d_gamma = (g * xhat).sum(0)
    if training:
        dx = gamma * fwd["invstd"] * (g - d_beta / k - xhat * d_gamma / k)
    else:
        dx = gamma * fwd["invstd"] * g
    return dx.T @ f, d_gamma, d_beta


def scatter(pillar_features, coords, batch_size, nx, ny):
    """The reference's PointPillarScatter.forward: [B, C, ny, nx]."""
    c = pillar_features.shape[1]
    out = np.zeros((batch_size, c, ny * nx), pillar_features.dtype)
    for b in range(batch_size):
        sel = coords[:, 0] == b
        out[b][:, coords[sel, 1] + coords[sel, 2] * nx + coords[sel, 3]] = pillar_features[sel].T
    return out.reshape(batch_size, c, ny, nx)


def make_points(rng, n, c, heavy=0, dirty=True, cells=(NX, NY)):
    """n rows (batch, x, y, z, extras): `heavy` of them in one pillar next to the origin, the rest spread over the first
    `cells` cells of the two frames; with `dirty` about 6 % outside x / y (below the range: dropped, three rows beyond its
    far edge), 10 % outside z (kept), a few NaN and batch -1 rows."""
    pts = np.zeros((n, 1 + c), np.float32)
    pts[:, 0] = rng.integers(0, BATCH, n)
    lo, hi = np.asarray(RANGE[:3]), np.asarray(RANGE[3:])
    span = hi - lo
    span[:2] = np.asarray(cells) * np.asarray(VOXEL[:2])
    pad = np.array([0.03, 0.03, 0.1]) if dirty else np.array([-0.01, -0.01, -0.01])
    pts[:, 1:4] = lo - pad * span + rng.uniform(0, 1, (n, 3)) * (1 + 2 * pad) * span
    pts[:, 4:] = rng.uniform(0, 1, (n, c - 3))
    if heavy:
        rows = rng.choice(n, heavy, replace=False)
        cell = np.array([1, 2])
        pts[rows, 0] = 1
        pts[rows, 1:3] = (cell + rng.uniform(0.02, 0.98, (heavy, 2))) * np.asarray(VOXEL[:2]) + lo[:2]
    if dirty and n >= 100:
        bad = rng.choice(n, 9, replace=False)
        pts[bad[6:8], 1] = hi[0] + rng.uniform(0.0, 0.1, 2)
        pts[bad[8], 2] = hi[1] + 0.05
        pts[bad[:2], 1] = np.nan
        pts[bad[2:3], 2] = np.nan
        pts[bad[3:6], 0] = -1
    return pts


def make_case(seed, n, c, use_abs=True, with_dist=False, kind="skew", check=True):
    """One input set.  kind: 'skew' 60 % of the points in one pillar; 'spread' none; 'tiny' 3 points in 2 pillars."""
    rng = np.random.default_rng(seed)
    if kind == "tiny":
        pts = np.zeros((3, 1 + c), np.float32)
        pts[:, 0] = (0, 1, 0)
        pts[:, 1:4] = [(0.21, 0.5, -1.0), (1.0, 1.3, 0.2), (0.29, 0.55, 0.4)]
        pts[:, 4:] = rng.uniform(0, 1, (3, c - 3))
    else:
        pts = make_points(rng, n, c, heavy=(n * 3) // 5 if kind == "skew" else 0)
    m = pillarize(pts)["num_pillars"]
    k = c_in_of(c, use_abs, with_dist)
    case = dict(points=pts, use_abs=use_abs, with_dist=with_dist, kind=kind,
                weight=rng.uniform(-1, 1, (C_OUT, k)).astype(np.float32) / np.float32(np.sqrt(10.0)),
                gamma=rng.uniform(0.5, 1.5, C_OUT).astype(np.float32), beta=rng.normal(0, 0.3, C_OUT).astype(np.float32),
                running_mean=rng.normal(0, 0.5, C_OUT).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, C_OUT).astype(np.float32), nbt=np.int64(7),
                d_out=rng.normal(0, 1, (m, C_OUT)).astype(np.float32))
    if check:
        share = ambiguous(forward(case)).mean()
        assert share <= 0.01, (kind, n, share)
    return case


#: name -> make_case arguments: the forward / gradient cases of tests/test_gpu_dyn_pillar_vfe.py;
#: tests/test_dyn_pillar_vfe_ref.py builds each once so that the 1 % cap on ambiguous pairs is asserted without a GPU
GPU_CASES = {
    "abs_skew": (0, 5000, 4, True, False, "skew"),
    "rel_dist_skew": (10, 5000, 5, False, True, "skew"),
    "tiny": (20, 3, 4, True, False, "tiny"),
}


def gpu_case(name):
    return make_case(*GPU_CASES[name])
