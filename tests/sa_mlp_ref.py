"""Plain restatements of spx_sa_mlp2_max (include/spx.h §28): the eval-mode tail of a two-layer stacked SA pointnet.

  sa_mlp2_max      numpy, float64 by default: the formula of the header, one line per step.
  composition      torch, any device and dtype: what the op replaces — the grouped (M, 3 + C, S) tensor with empty balls
                   zeroed, Conv2d, eval BatchNorm2d, ReLU, Conv2d, BatchNorm2d, ReLU, max over the slots.
  fold_bn          eval BatchNorm (gamma, beta, mean, var) -> the affine map (a, b) the op takes.
  exact_cases      small-integer data on which every product and every sum is an integer below 2^24, so float32 holds
                   them whatever the order of summation: the device result must equal the restatement bit for bit.
  float_case       random data at PV-RCNN's channel plans for the accuracy comparison."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
EXACT = float(1 << 24)
SHAPES = ((16, 16, 16), (16, 32, 16), (64, 16, 16), (32, 32, 32), (64, 64, 16), (64, 64, 32))   # (C1, C2, S)
MS = (1, 3, 65)
NS = (1, 40)


# ------------------------------------------------------------------------------------------------------- restatement
def sa_mlp2_max(P, xyz, new_xyz, idx, empty, Wx, a1, b1, W2, a2, b2, dtype=np.float64):
    """out (M, C2).  P (N, C1) or None, xyz (N, 3), new_xyz (M, 3), idx (M, S) global rows, empty (M) bool or None,
    Wx (C1, 3), a1 / b1 (C1), W2 (C2, C1), a2 / b2 (C2).  An empty ball, and a row outside [0, N), is a zero column."""
    xyz, new_xyz, Wx, a1, b1, W2, a2, b2 = [np.asarray(v, dtype) for v in (xyz, new_xyz, Wx, a1, b1, W2, a2, b2)]
    idx = np.asarray(idx, np.int64)
    m, s = idx.shape
    n, c1 = xyz.shape[0], Wx.shape[0]
    valid = (idx >= 0) & (idx < n)
    if empty is not None:
        valid &= ~np.asarray(empty, bool)[:, None]
    r = np.clip(idx, 0, max(n - 1, 0))
    d = np.where(valid[..., None], xyz[r] - new_xyz[:, None, :], 0)                       # (M, S, 3)
    p = np.zeros((m, s, c1), dtype) if P is None else np.where(valid[..., None], np.asarray(P, dtype)[r], 0)
    h = np.maximum(a1 * (p + d @ Wx.T) + b1, 0)                                           # (M, S, C1)
    z = np.maximum(a2 * (h @ W2.T) + b2, 0)                                               # (M, S, C2)
    return z.max(axis=1)


def fold_bn(gamma, beta, mean, var, eps=EPS):
    a = gamma / np.sqrt(var + eps)
    return a, beta - mean * a


# ------------------------------------------------------------------------------------------------------- composition
def composition(features, xyz, new_xyz, idx, empty, Wf, Wx, bn1, W2, bn2, eps=EPS):
    """torch tensors of one device and dtype; features (N, C) and Wf (C1, C), or both None; bn = (gamma, beta, running
    mean, running var).  idx (M, S) integer global rows, empty (M) bool.  -> (M, C2)."""
    n = xyz.shape[0]
    valid = ((idx >= 0) & (idx < n) & ~empty[:, None])[..., None]
    r = idx.long().clamp(0, max(n - 1, 0))
    zero = torch.zeros((), dtype=xyz.dtype, device=xyz.device)
    grouped = torch.where(valid, xyz[r] - new_xyz[:, None, :], zero)                      # (M, S, 3)
    w1 = Wx
    if features is not None:
        grouped = torch.cat([grouped, torch.where(valid, features[r], zero)], dim=-1)    # (M, S, 3 + C)
        w1 = torch.cat([Wx, Wf], dim=1)
    x = grouped.permute(2, 0, 1).unsqueeze(0)                                             # (1, 3 + C, M, S)
    for w, (gamma, beta, mean, var) in ((w1, bn1), (W2, bn2)):
        x = F.conv2d(x, w[:, :, None, None])
        x = F.relu(F.batch_norm(x, mean, var, gamma, beta, False, 0.0, eps))
    x = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)                           # (1, C2, M)
    return x.squeeze(0).permute(1, 0)


# ------------------------------------------------------------------------------------------------------- lists
def random_lists(rng, m, s, n, p_empty=0.25, specials=True):
    """Ball-query-shaped lists: k in [1, s] ascending hits, the unfilled slots repeat the first hit; an empty ball is all 0
    with its mask set.  specials: some slots point at row n - 1, some lie outside [0, n) (-1, n, n + 5)."""
    idx = np.zeros((m, s), np.int32)
    empty = rng.random(m) < p_empty
    for q in range(m):
        if empty[q]:
            continue
        k = int(rng.integers(1, s + 1))
        hits = np.sort(rng.integers(0, n, size=k))
        idx[q, :k] = hits
        idx[q, k:] = hits[0]
        if specials and rng.random() < 0.3:
            idx[q, int(rng.integers(0, s))] = n - 1
        if specials and rng.random() < 0.3:
            idx[q, int(rng.integers(0, s))] = (-1, n, n + 5)[int(rng.integers(0, 3))]
    return idx, empty


# ------------------------------------------------------------------------------------------------------- exact cases
KINDS = ("mixed", "distinct_w2", "winner_row", "negative_l1", "all_empty", "p_none")


def exact_case_names():
    """Every (shape, M, N) as `mixed`; the special kinds at the shapes that can hold them."""
    names = []
    for c1, c2, s in SHAPES:
        for m in MS:
            for n in NS:
                names.append(("mixed", c1, c2, s, m, n))
        names.append(("winner_row", c1, c2, s, 3, 40))
        names.append(("negative_l1", c1, c2, s, 65, 40))
        names.append(("all_empty", c1, c2, s, 65, 40))
        names.append(("p_none", c1, c2, s, 65, 40))
        if c1 != c2:
            names.append(("distinct_w2", c1, c2, s, 65, 40))
    return names


def case_id(key):
    return "%s-c%d-c%d-s%d-m%d-n%d" % key


@functools.lru_cache(maxsize=None)
def exact_case(key):
    """Integer inputs (float64 arrays holding integers) and the float64 restatement, computed once and shared; never
    written to.  Asserts that float32 holds every intermediate exactly."""
    kind, c1, c2, s, m, n = key
    rng = np.random.default_rng(sum(map(ord, case_id(key))))
    idx, empty = random_lists(rng, m, s, n)
    xyz = rng.integers(-8, 9, size=(n, 3)).astype(np.float64)
    new_xyz = rng.integers(-8, 9, size=(m, 3)).astype(np.float64)
    P = rng.integers(-8, 9, size=(n, c1)).astype(np.float64)
    Wx = rng.integers(-2, 3, size=(c1, 3)).astype(np.float64)
    a1 = rng.integers(-2, 3, size=(c1,)).astype(np.float64)
    b1 = rng.integers(-4, 5, size=(c1,)).astype(np.float64)
    W2 = rng.integers(-3, 4, size=(c2, c1)).astype(np.float64)
    a2 = rng.integers(-2, 3, size=(c2,)).astype(np.float64)
    b2 = rng.integers(-4, 5, size=(c2,)).astype(np.float64)
    if kind == "distinct_w2":                       # a transposed or mis-strided W2 cannot reproduce this
        W2 = (rng.permutation(c1 * c2) - (c1 * c2) // 2).reshape(c2, c1).astype(np.float64)
        a2 = np.where(a2 == 0, 1.0, a2)
    elif kind == "winner_row":                      # the maximum of channel o sits in row o % S, and only there
        assert n >= s and c1 >= s
        idx = np.tile(np.arange(s, dtype=np.int32), (m, 1))
        empty = np.zeros(m, bool)
        P = np.zeros((n, c1))
        P[np.arange(s), np.arange(s)] = 10.0        # source row r < S is one-hot in channel r
        Wx[:] = 0
        a1[:] = 1
        b1[:] = 0
        W2 = (-rng.integers(0, 3, size=(c2, c1))).astype(np.float64)
        W2[np.arange(c2), np.arange(c2) % s] = 3.0  # z[s, o] = 10 * W2[o, s]: 30 in row o % S, <= 0 elsewhere
        a2[:] = 1
        b2 = rng.integers(1, 5, size=(c2,)).astype(np.float64)
    elif kind == "negative_l1":                     # even channels: layer 1 below zero everywhere; odd: b1 > 0
        P[:, 0::2] = -200 - np.abs(P[:, 0::2])
        a1[0::2] = 1 + np.abs(a1[0::2])
        b1[0::2] = -np.abs(b1[0::2])
        b1[1::2] = 1 + np.abs(b1[1::2])
    elif kind == "all_empty":
        empty[:] = True
        idx[:] = 0
    elif kind == "p_none":
        P = None
    out = sa_mlp2_max(P, xyz, new_xyz, idx, empty, Wx, a1, b1, W2, a2, b2)
    # float32 exactness: the largest conceivable magnitude of any partial sum, from absolute values
    d_max = 16.0
    p_max = 0.0 if P is None else np.abs(P).max()
    h_max = np.abs(a1) * (p_max + np.abs(Wx).sum(axis=1) * d_max) + np.abs(b1)            # (C1)
    z_max = np.abs(a2) * (np.abs(W2) @ h_max) + np.abs(b2)
    assert z_max.max() < EXACT and h_max.max() < EXACT, (key, z_max.max())
    if kind == "winner_row":
        assert np.array_equal(out, np.tile(30.0 + b2, (m, 1)))
    if kind == "all_empty":
        assert np.array_equal(out, np.tile(np.maximum(a2 * (W2 @ np.maximum(b1, 0)) + b2, 0), (m, 1)))
    return dict(key=key, P=P, xyz=xyz, new_xyz=new_xyz, idx=idx, empty=empty, Wx=Wx, a1=a1, b1=b1, W2=W2, a2=a2, b2=b2,
                out=out)


def identity_bn(a, b, eps=EPS):
    """(gamma, beta, mean, var) whose eval fold is (a, b) to a rounding error: mean 0, var + eps = 1."""
    return a, b, np.zeros_like(a), np.full_like(a, 1.0 - eps)


# ------------------------------------------------------------------------------------------------------- float cases
#             name          C_in  C1  C2  S   M    N
FLOAT_CASES = (("roi_grid_0", 128, 64, 64, 16, 432, 600),
               ("roi_grid_1", 128, 64, 64, 16, 432, 600),
               ("roi_grid_2", 128, 64, 64, 16, 432, 600),
               ("vsa_0",      16,  16, 16, 32, 432, 600))


@functools.lru_cache(maxsize=None)
def float_case(name):
    """float64 arrays: features, geometry, lists, both convs and both BatchNorms at a PV-RCNN channel plan, and the
    float64 restatement of the result."""
    _, c_in, c1, c2, s, m, n = [k for k in FLOAT_CASES if k[0] == name][0]
    rng = np.random.default_rng(sum(map(ord, name)))
    idx, empty = random_lists(rng, m, s, n, p_empty=0.15, specials=False)
    xyz = rng.uniform(-3.0, 3.0, size=(n, 3))
    new_xyz = rng.uniform(-3.0, 3.0, size=(m, 3))
    features = rng.standard_normal((n, c_in))
    w1 = rng.standard_normal((c1, 3 + c_in)) * np.sqrt(2.0 / (3 + c_in))                  # kaiming, as init_weights
    W2 = rng.standard_normal((c2, c1)) * np.sqrt(2.0 / c1)

    def bn(c):
        return (rng.uniform(0.5, 1.5, c), rng.standard_normal(c) * 0.1, rng.standard_normal(c) * 0.1,
                rng.uniform(0.5, 1.5, c))
    bn1, bn2 = bn(c1), bn(c2)
    Wx, Wf = w1[:, :3].copy(), w1[:, 3:].copy()
    a1, b1 = fold_bn(*bn1)
    a2, b2 = fold_bn(*bn2)
    out = sa_mlp2_max(features @ Wf.T, xyz, new_xyz, idx, empty, Wx, a1, b1, W2, a2, b2)
    return dict(features=features, xyz=xyz, new_xyz=new_xyz, idx=idx, empty=empty, Wf=Wf, Wx=Wx, bn1=bn1, W2=W2, bn2=bn2,
                a1=a1, b1=b1, a2=a2, b2=b2, out=out)
