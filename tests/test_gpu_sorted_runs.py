"""The edges of the sorted-runs contract (csrc/sorted_runs.h) through the six Python entry points that rest on it:
ops.group_points_bwd, three_interpolate_bwd, stack_group_points_bwd, stack_three_interpolate_bwd, group_project_bwd
(dP^T only) and voxel_pool_max_bwd (df only).

One index pattern is a list of entries, each a target row or a dropped slot (index -1, index == n, an empty ball where the
op has one), laid out in each op's own geometry.  C = 3, gradients are integers with |v| <= 8 and weights are 1 or 2, so
every float32 sum (at most 300 terms of magnitude <= 16) is exact in any order: the result must EQUAL a float64
index_add_ on the CPU cast to float32, and two calls must be bit-equal.  No tolerance is involved."""
import functools

import numpy as np
import pytest
import torch

from spx import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
C = 3
NEG, EMPTY = -1, -2   # dropped slots; a value == n is the third kind


def _blocks(rng, pairs, count):
    """`count` aligned pairs drawn from `pairs`: an EMPTY pair then covers one whole ball of the ops with nsample 2"""
    return np.array([pairs[i] for i in rng.integers(0, len(pairs), count)], np.int64).reshape(-1)


@functools.lru_cache(maxsize=None)
def _pattern(name):
    """-> (n targets, entries (E,) int64, frames of the two batch ops); E is a multiple of 6"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("pow2_64", "pow2_65", "two_frames"):       # n == 2^6: the sentinel needs one bit more than n - 1
        n = 65 if name == "pow2_65" else 64
        pairs = [(0, n - 1), (n - 1, 0), (NEG, n), (n, 0), (n - 1, NEG), (EMPTY, EMPTY), (0, 0), (n - 1, n - 1)]
        return n, _blocks(rng, pairs, 48), 2 if name == "two_frames" else 1
    if name == "one_target":                               # sentinel 1, one key bit
        return 1, _blocks(rng, [(0, 0), (0, NEG), (1, 0), (EMPTY, EMPTY)], 48), 1
    if name == "all_dropped":
        return 64, _blocks(rng, [(NEG, 64), (64, NEG), (EMPTY, EMPTY), (NEG, NEG)], 48), 1
    if name == "one_long_run":                             # crosses the 128-position chunks and a 256-thread block
        return 64, np.full(300, 63, np.int64), 1
    raise KeyError(name)


PATTERNS = ("pow2_64", "pow2_65", "one_target", "all_dropped", "one_long_run")
OPS = ("group_points", "three_interpolate", "stack_group_points", "stack_three_interpolate", "group_project", "voxel_pool")
CASES = [(op, p) for op in OPS for p in PATTERNS] + [("group_points", "two_frames"), ("three_interpolate", "two_frames")]


def _ints(rng, shape, lo=-8, hi=8):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float32))


def _idx(entries, empty_as):
    return torch.from_numpy(np.where(entries == EMPTY, empty_as, entries).astype(np.int32))


def _poison(*shape):
    """A freed NaN block of the output's size: the op's torch.empty of that size takes it from the caching allocator."""
    torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _case(op, pattern):
    """-> run() -> (targets, C) device result, and the float32 cast of the float64 CPU index_add_; built once."""
    n, ent, frames = _pattern(pattern)
    rng = np.random.default_rng(sum(map(ord, op + pattern)))
    e = ent.shape[0]
    has_empty = op in ("group_project", "voxel_pool")
    live = (ent >= 0) & (ent < n)
    tgt = torch.from_numpy(np.concatenate([np.where(live, ent + f * n, -1) for f in range(frames)]))
    if op == "group_points":
        idx = _idx(ent, NEG).view(1, e // 2, 2).repeat(frames, 1, 1)
        g = _ints(rng, (frames, C, e // 2, 2))
        contrib = g.reshape(frames, C, e).permute(0, 2, 1).reshape(-1, C)
        gd, id_ = g.to(DEV), idx.to(DEV)
        run = lambda: ops.group_points_bwd(gd, id_, n).permute(0, 2, 1).reshape(frames * n, C)
        shape = (frames, C, n)
    elif op == "three_interpolate":
        idx = _idx(ent, NEG).view(1, e // 3, 3).repeat(frames, 1, 1)
        g, w = _ints(rng, (frames, C, e // 3)), _ints(rng, (frames, e // 3, 3), 1, 2)
        contrib = (g.permute(0, 2, 1)[:, :, None, :] * w[:, :, :, None]).reshape(-1, C)
        gd, id_, wd = g.to(DEV), idx.to(DEV), w.to(DEV)
        run = lambda: ops.three_interpolate_bwd(gd, id_, wd, n).permute(0, 2, 1).reshape(frames * n, C)
        shape = (frames, C, n)
    elif op == "stack_group_points":
        idx, g = _idx(ent, NEG).view(e // 2, 2), _ints(rng, (e // 2, C, 2))
        contrib = g.permute(0, 2, 1).reshape(-1, C)
        gd, id_ = g.to(DEV), idx.to(DEV)
        nc, mc = (torch.tensor([v], dtype=torch.int32, device=DEV) for v in (n, e // 2))
        run = lambda: ops.stack_group_points_bwd(gd, nc, id_, mc, n)
        shape = (n, C)
    elif op == "stack_three_interpolate":
        idx, g, w = _idx(ent, NEG).view(e // 3, 3), _ints(rng, (e // 3, C)), _ints(rng, (e // 3, 3), 1, 2)
        contrib = (g[:, None, :] * w[:, :, None]).reshape(-1, C)
        gd, id_, wd = g.to(DEV), idx.to(DEV), w.to(DEV)
        run = lambda: ops.stack_three_interpolate_bwd(gd, id_, wd, n)
        shape = (n, C)
    elif op == "group_project":
        idx, g = _idx(ent, 0).view(e // 2, 2), _ints(rng, (1, C, e // 2, 2))     # an empty ball points at the live row 0
        empty = torch.from_numpy((ent.reshape(-1, 2) == EMPTY).any(1))
        contrib = g.reshape(C, e).t()
        gd, id_, ed = g.to(DEV), idx.to(DEV), empty.to(DEV)
        run = lambda: ops.group_project_bwd(gd, None, None, id_, ed, n, need_dwx=False)[0].t()
        shape = (C, n)
    else:
        # nsample 1 and arg 0: the one slot of every query wins in every channel, so every entry counts
        idx, g = _idx(ent, 0).view(e, 1), _ints(rng, (e, C))
        empty = torch.from_numpy(ent == EMPTY)
        contrib = g
        gd, id_, ed = g.to(DEV), idx.to(DEV), empty.to(DEV)
        arg = torch.zeros((e, C), dtype=torch.int32, device=DEV)
        xyz, new_xyz = torch.zeros((n, 3), device=DEV), torch.zeros((e, 3), device=DEV)
        run = lambda: ops.voxel_pool_max_bwd(gd, arg, xyz, new_xyz, id_, ed, n)[0]
        shape = (n, C)
    keep = tgt >= 0
    ref = torch.zeros((frames * n, C), dtype=torch.float64).index_add_(0, tgt[keep], contrib.double()[keep])
    assert float(ref.abs().max()) < 2 ** 24
    return run, ref.float(), shape


@pytest.mark.parametrize("op,pattern", CASES, ids=["%s-%s" % c for c in CASES])
def test_sorted_runs_edges(op, pattern):
    run, ref, shape = _case(op, pattern)
    _poison(*shape)
    a = run().contiguous().cpu()
    _poison(*shape)
    b = run().contiguous().cpu()
    assert torch.equal(a, ref), (a - ref).abs().max()
    assert torch.equal(a, b)
    if pattern == "all_dropped":
        assert not ref.any()
    if pattern == "one_long_run":
        assert not a[:-1].any() and ref[-1].any()
