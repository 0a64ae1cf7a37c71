"""PillarVFE (include/spx.h §23) and DynamicPillarVFE (§24) are ONE PFN layer (csrc/pfn_layer.h): on inputs where the two
files' feature builders give the same doubles, the two ops must agree bit for bit in eval mode.

Why they must.  Points are (batch, x, y, z, intensity) with x, y, z multiples of 2^-6 in [0, 64), voxels of 0.5 from a
range that starts at 0, and every pillar holds a power-of-two number of points (1 .. 32).  A sum of at most 32 such
coordinates is exact in double and so is its division by a power of two, so slots 3-5 (xyz - pillar mean) are the same
doubles whether they are formed as `x - sum * (1 / n)` (§23, one fma) or as `x - stored mean` (§24).  The pillar centres
are dyadic, and the z cell is 0 on both sides, so §23's `centre32(0, vz, oz)` is §24's `oz`.  From equal features the shared
dot13 / fold give equal activations, and the max of equal candidates is the same whatever the order they are walked in.
§23's padding rows offer relu(shift); with running_mean = 0 and beta <= 0 the shift is <= 0, the offer is 0 and never
beats a best >= 0 under the strict `>`: the one place where the two ops legitimately differ is out of play.  Ties keep
the lowest slot in §23 and the lowest position in §24, which are the same point because the §23 voxels are filled in
`order`.

The patterns: one pillar of 32; (1, 32, 32), whose third pillar straddles a 64-position chunk edge (§24's head / tail
partial slots and k_fwd_combine); 70 pillars cycling 1, 2, 4, 8, 16, 32: several 256-position tiles in §24, a ragged
last 8-pillar tile in §23."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T = 32
VOXEL = (0.5, 0.5, 4.0)
RANGE = (0.0, 0.0, -1.0, 64.0, 64.0, 3.0)
OFFSETS = (0.25, 0.25, 1.0)                 # voxel / 2 + range_lo, all dyadic
EPS, MOMENTUM = 1e-3, 0.01
PATTERNS = {
    "one_pillar_of_32": (32,),
    "chunk_edge_1_32_32": (1, 32, 32),
    "seventy_pillars": tuple((1, 2, 4, 8, 16, 32)[i % 6] for i in range(70)),
}


def _points(counts, seed):
    """Pillar i sits in cell (cx = i, cy = (7 i) mod 128) of frame 0, so pillar rows come out in pattern order; the point
    rows are shuffled, so `order` is not the identity."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, n in enumerate(counts):
        cx, cy = i, (7 * i) % 128
        p = np.zeros((n, 5), np.float64)
        p[:, 1] = cx * 0.5 + rng.integers(0, 32, n) / 64.0
        p[:, 2] = cy * 0.5 + rng.integers(0, 32, n) / 64.0
        p[:, 3] = rng.integers(0, 64 * 64, n) / 64.0
        p[:, 4] = rng.integers(0, 256, n) / 256.0
        rows.append(p)
    pts = np.concatenate(rows).astype(np.float32)
    assert (pts[:, 1:4] * 64 == np.round(pts[:, 1:4] * 64)).all() and pts[:, 1:4].min() >= 0 and pts[:, 1:4].max() < 64
    return pts[rng.permutation(pts.shape[0])]


def _params(c_in, seed):
    g = torch.Generator().manual_seed(seed)
    weight = torch.randn((64, c_in), generator=g) * 0.3
    gamma = torch.randn((64,), generator=g)
    beta = -torch.rand((64,), generator=g)
    beta[::8] = 0.0                                               # the boundary of beta <= 0
    running_var = 0.5 + 1.5 * torch.rand((64,), generator=g)
    return [t.to(DEV) for t in (weight, gamma, beta, torch.zeros((64,)), running_var)]


@functools.lru_cache(maxsize=None)
def _both(pattern, use_abs):
    """Both ops on one cloud -> (out_pillar, arg_pillar, out_dyn, arg_dyn, order, offset, count), computed once."""
    from spx import ops
    counts = PATTERNS[pattern]
    pts = torch.from_numpy(_points(counts, len(counts))).to(DEV)
    pz = ops.dynamic_pillarize(pts, RANGE, VOXEL, batch_size=1, sync=True)
    assert pz["num_pillars"] == len(counts) and pz["count"].tolist() == list(counts)
    assert (pz["coords"][:, 1] == 0).all()                        # the z cell
    weight, gamma, beta, rm, rv = _params(ops.pillar_vfe_c_in(4, use_abs, False), 7)
    kw = dict(use_absolute_xyz=use_abs, with_distance=False, training=False)
    dyn = ops.dynamic_pillar_vfe_fwd(pts, pz, weight, gamma, beta, rm, rv, None, MOMENTUM, EPS, VOXEL[:2], OFFSETS, **kw)
    order, offset, count = pz["order"].long(), pz["offset"].long(), pz["count"]
    m = len(counts)
    voxels = torch.zeros((m, T, 4), dtype=torch.float32, device=DEV)
    for p in range(m):
        voxels[p, :counts[p]] = pts[order[offset[p]:offset[p] + counts[p]], 1:]
    pil = ops.pillar_vfe_fwd(voxels, count, pz["coords"], weight, gamma, beta, rm, rv, None, MOMENTUM, EPS, VOXEL, OFFSETS,
                             **kw)
    torch.cuda.synchronize()
    return pil["out"], pil["arg"].long(), dyn["out"], dyn["arg"].long(), order, offset, count


@pytest.mark.parametrize("use_abs", [True, False])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_pillar_and_dynamic_pillar_vfe_agree_bitwise_in_eval(pattern, use_abs):
    out_p, arg_p, out_d, arg_d, order, offset, count = _both(pattern, use_abs)
    assert out_p.shape == out_d.shape == (len(PATTERNS[pattern]), 64)
    assert torch.equal(out_p, out_d)
    pos = out_p > 0
    assert pos.any()
    assert (arg_p[pos] < count.long()[:, None].expand(-1, 64)[pos]).all()      # no padding row won
    row = order[(offset[:-1, None] + arg_p).clamp(max=order.shape[0] - 1)]
    assert torch.equal(row[pos], arg_d[pos])
