"""Float64 numpy restatement of PillarVFE with one last-layer PFNLayer (reference
pcdet/models/backbones_3d/vfe/pillar_vfe.py:29-123), forward and parameter gradients, plus the case generator of
tests/test_gpu_pillar_vfe.py.  The [M, T, C_out] tensors are built densely here: the kernel's algebra (include/spx.h §23)
is not restated, so the two check each other.

Selection: arg[m, c] is the index of the first row of relu(z[m, :, c]) that attains the maximum, reported as T when that
row is a padding row; active[m, c] = out[m, c] > 0.  backward() takes an optional (arg, active) override, so that the
gradient can be evaluated for the winners another implementation chose."""
import numpy as np

VOXEL = (0.16, 0.16, 4.0)
RANGE_LO = (0.0, -39.68, -3.0)
GRID = (432, 496)                     # nx, ny
MOMENTUM, EPS = 0.01, 1e-3
C_OUT = 64


def offsets(voxel=VOXEL, range_lo=RANGE_LO):
    return tuple(v / 2 + lo for v, lo in zip(voxel, range_lo))


def c_in_of(c, use_abs, with_dist):
    return (c + 6 if use_abs else c + 3) + (1 if with_dist else 0)


def features(voxels, num, coords, use_abs, with_dist, voxel=VOXEL, offs=None, center_dtype=np.float64):
    """[M, T, C_in] float64, zero on the padding rows.  center_dtype=float32 forms the pillar centre as the float32
    composition does (product and sum rounded to float32)."""
    offs = offsets(voxel) if offs is None else offs
    v = voxels.astype(np.float64)
    m, t, _c = v.shape
    n = np.clip(num.astype(np.int64), 0, t)
    mask = np.arange(t)[None, :] < n[:, None]
    v = v * mask[:, :, None]
    xyz = v[:, :, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = xyz.sum(1, keepdims=True) / n.astype(np.float64)[:, None, None]
    cd = center_dtype
    ctr = np.stack([(coords[:, 3 - j].astype(cd) * cd(voxel[j]) + cd(offs[j])).astype(np.float64) for j in range(3)], 1)
    parts = [v if use_abs else v[:, :, 3:], xyz - mean, xyz - ctr[:, None, :]]
    if with_dist:
        parts.append(np.sqrt((xyz * xyz).sum(2, keepdims=True)))
    f = np.concatenate(parts, 2)
    return np.where(mask[:, :, None], f, 0.0), n


def forward(case, training=True, center_dtype=np.float64):
    f, n = features(case["voxels"], case["num"], case["coords"], case["use_abs"], case["with_dist"],
                    offs=case.get("offs", None), center_dtype=center_dtype)
    m, t, _k = f.shape
    w, gamma, beta = (case[k].astype(np.float64) for k in ("weight", "gamma", "beta"))
    x = f @ w.T                                                  # [M, T, C_out]
    rm, rv = case["running_mean"].astype(np.float64), case["running_var"].astype(np.float64)
    out = dict(f=f, n=n, x=x)
    if training:
        cnt = m * t
        mean = x.reshape(cnt, -1).mean(0)
        var = x.reshape(cnt, -1).var(0)                          # biased
        out["running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
        out["running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * var * cnt / max(cnt - 1, 1)
        out["nbt"] = int(case["nbt"]) + 1
    else:
        mean, var = rm, rv
    invstd = 1.0 / np.sqrt(var + EPS)
    z = (x - mean) * invstd * gamma + beta
    y = np.maximum(z, 0.0)
    idx = y.argmax(1)                                            # first maximum
    out.update(mean=mean, var=var, invstd=invstd, z=z, out=y.max(1))
    out["arg"] = np.where(idx >= n[:, None], t, idx).astype(np.int64)
    out["active"] = out["out"] > 0
    return out


def ambiguous(fwd):
    """[M, C_out] bool: the float64 top-two gap of the candidates (the real rows and, where the pillar has padding, ONE
    padding candidate), or the top value's distance from 0, is below 1e-5 max|z|."""
    z, n = fwd["z"], fwd["n"]
    m, t, c = z.shape
    thr = 1e-5 * np.abs(z).max()
    cand = np.where((np.arange(t)[None, :] <= n[:, None])[:, :, None], z, -np.inf)     # rows 0 .. n: n is the padding one
    top2 = -np.sort(-cand, axis=1)[:, :2]
    if t == 1 or top2.shape[1] < 2:
        gap = np.full((m, c), np.inf)
    else:
        gap = top2[:, 0] - top2[:, 1]
    return (gap < thr) | (np.abs(top2[:, 0]) < thr)


def backward(case, fwd, d_out, arg=None, active=None, training=True):
    """(d_weight, d_gamma, d_beta) through the dense [M, T, C_out] BatchNorm backward."""
    arg = fwd["arg"] if arg is None else np.asarray(arg, np.int64)
    active = fwd["active"] if active is None else np.asarray(active, bool)
    f, n, x = fwd["f"], fwd["n"], fwd["x"]
    m, t, _k = f.shape
    gamma = case["gamma"].astype(np.float64)
    row = np.where(arg >= t, np.minimum(n, t - 1)[:, None], arg)          # a padding winner: the first padding row
    g = np.zeros_like(x)
    mi, ci = np.nonzero(active)
    g[mi, row[mi, ci], ci] = d_out.astype(np.float64)[mi, ci]
    xhat = (x - fwd["mean"]) * fwd["invstd"]
    d_beta = g.sum((0, 1))
    d_gamma = (g * xhat).sum((0, 1))
    if training:
        cnt = m * t
        dx = gamma * fwd["invstd"] * (g - d_beta / cnt - xhat * d_gamma / cnt)
    else:
        dx = gamma * fwd["invstd"] * g
    d_weight = np.einsum("mtc,mtk->ck", dx, f)
    return d_weight, d_gamma, d_beta


def scatter(pillar_features, coords, batch_size, nx, ny):
    """The reference's PointPillarScatter.forward: [B, C, ny, nx]."""
    c = pillar_features.shape[1]
    out = np.zeros((batch_size, c, ny * nx), pillar_features.dtype)
    for b in range(batch_size):
        sel = coords[:, 0] == b
        out[b][:, coords[sel, 1] + coords[sel, 2] * nx + coords[sel, 3]] = pillar_features[sel].T
    return out.reshape(batch_size, c, ny, nx)


def make_case(seed, m, t, c, use_abs=True, with_dist=False, kind="mixed", check=True):
    """One input set.  kind: 'mixed' point counts from 1 to T with most pillars nearly empty; 'full' every pillar full;
    'neg_beta' some channels' beta so negative that their maxima are all 0; 'far' x near 70 m with millimetre spread
    inside a pillar; 'dup' a few pillars whose second point repeats the first."""
    rng = np.random.default_rng(seed)
    nx, ny = GRID
    x_lo = nx - 40 if kind == "far" else 0
    cells = rng.choice((nx - x_lo) * ny * 2, size=m, replace=False)
    coords = np.stack([cells % 2, np.zeros(m, np.int64), (cells // 2) % ny, x_lo + (cells // 2) // ny], 1).astype(np.int32)
    if kind == "full":
        num = np.full(m, t)
    else:
        num = np.minimum(1 + rng.geometric(0.25, m), t)                   # a KITTI-like skew
        if m >= 3:
            num[:3] = (1, t, max(t // 2, 1))
        elif m == 2:
            num[:2] = (1, t)
    offs = np.asarray(offsets())
    centre = coords[:, [3, 2, 1]] * np.asarray(VOXEL) + offs
    half = np.full(3, 3e-3) if kind == "far" else 0.5 * np.asarray(VOXEL)      # metres around the pillar centre
    u = rng.uniform(-1.0, 1.0, (m, t, 3)) * half
    voxels = np.zeros((m, t, c), np.float32)
    voxels[:, :, :3] = centre[:, None, :] + u
    voxels[:, :, 3:] = rng.uniform(0, 1, (m, t, c - 3))
    dup = np.zeros(m, bool)
    if kind == "dup":
        dup[np.argsort(-num, kind="stable")[:max(m // 50, 1)]] = True
        dup &= num >= 2
        voxels[dup, 1] = voxels[dup, 0]
    voxels *= (np.arange(t)[None, :] < num[:, None])[:, :, None]         # zero padding, as the voxeliser leaves it
    k = c_in_of(c, use_abs, with_dist)
    case = dict(voxels=voxels, num=num.astype(np.int32), coords=coords, use_abs=use_abs, with_dist=with_dist, dup=dup,
                weight=rng.uniform(-1, 1, (C_OUT, k)).astype(np.float32) / np.float32(np.sqrt(10.0)),
                gamma=rng.uniform(0.5, 1.5, C_OUT).astype(np.float32), beta=rng.normal(0, 0.3, C_OUT).astype(np.float32),
                running_mean=rng.normal(0, 0.5, C_OUT).astype(np.float32),
                running_var=rng.uniform(0.5, 2.0, C_OUT).astype(np.float32), nbt=np.int64(7),
                d_out=rng.normal(0, 1, (m, C_OUT)).astype(np.float32), t=t, kind=kind)
    if kind == "neg_beta":
        case["beta"][::4] = -15.0
    if check:
        share = ambiguous(forward(case)).mean()
        assert share <= 0.01, (kind, m, t, share)
    return case


#: name -> make_case arguments: the cases of tests/test_gpu_pillar_vfe.py (M in {1, 2, 257, 1000}, T in {32, 20, 1},
#: C in {4, 5}, both flags on and off); tests/test_pillar_vfe_ref.py builds each once so that the 1 % cap on ambiguous
#: pairs is asserted without a GPU
GPU_CASES = {
    "m1_t32": (0, 1, 32, 4, True, False, "mixed"),
    "m2_t20_rel_dist": (10, 2, 20, 5, False, True, "mixed"),
    "m257_t32": (20, 257, 32, 4, True, False, "mixed"),
    "m1000_t20_dist": (30, 1000, 20, 5, True, True, "mixed"),
    "m257_t1_rel": (41, 257, 1, 4, False, False, "mixed"),
    "full": (50, 257, 32, 5, True, False, "full"),
    "neg_beta": (61, 257, 20, 4, True, False, "neg_beta"),
    "far": (70, 257, 32, 5, True, True, "far"),
    "dup": (80, 257, 32, 4, True, False, "dup"),
}


def gpu_case(name):
    return make_case(*GPU_CASES[name])
