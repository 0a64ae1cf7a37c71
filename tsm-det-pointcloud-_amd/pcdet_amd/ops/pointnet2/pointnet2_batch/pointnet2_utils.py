"""pointnet2_batch on libspx (include/spx.h §11; reference pcdet/ops/pointnet2/pointnet2_batch/pointnet2_utils.py).

Same public names, call signatures and return values as the reference module; every op runs the HIP kernels of
csrc/pointnet2.hip.  Sampling, ball query and three-NN return integer tensors and carry no gradient; gather, grouping
and three-point interpolation are autograd Functions whose backward sums duplicate indices in a fixed order
(deterministic, unlike the reference's atomicAdd)."""
import torch
import torch.nn as nn
from torch.autograd import Function

from spx import ops

__all__ = [
    "calc_dist_matrix_for_sampling", "furthest_point_sample", "farthest_point_sample", "furthest_point_sample_matrix",
    "furthest_point_sample_weights", "furthest_point_sample_with_dist", "furthest_point_sample_with_weighted_dist",
    "gather_operation", "grouping_operation", "three_nn", "three_interpolate", "ball_query", "ball_query_dilated",
    "QueryAndGroup", "QueryAndGroupDilated", "GroupAll", "group_project",
]


@torch.no_grad()
def calc_dist_matrix_for_sampling(xyz, features=None, gamma=1.0):
    """(B, N, 3) [+ (B, N, C) features] -> (B, N, N) pairwise distance matrix for the matrix FPS forms."""
    dist = torch.cdist(xyz, xyz)
    if features is not None:
        dist += torch.cdist(features, features) * gamma
    return dist


@torch.no_grad()
def furthest_point_sample(xyz, npoint):
    """xyz (B, N, 3) -> (B, npoint) int32 indices of iterative furthest point sampling (the first pick is point 0)."""
    return ops.furthest_point_sample(xyz, npoint)


farthest_point_sample = furthest_point_sample


@torch.no_grad()
def furthest_point_sample_matrix(matrix, npoint):
    """matrix (B, N, N) pairwise distances -> (B, npoint) int32."""
    return ops.furthest_point_sample_matrix(matrix, npoint)


@torch.no_grad()
def furthest_point_sample_weights(xyz, weights, npoint):
    """xyz (B, N, 3), weights (B, N) -> (B, npoint) int32; the first pick is the heaviest point, later picks rank the
    minimum distance times max(weight, 1e-12)."""
    return ops.furthest_point_sample(xyz, npoint, weights=weights)


@torch.no_grad()
def furthest_point_sample_with_dist(dist, npoint):
    """dist (B, N, N) pairwise distances -> (B, npoint) int32 (the reference's matrix kernel under its other name)."""
    return ops.furthest_point_sample_matrix(dist, npoint)


@torch.no_grad()
def furthest_point_sample_with_weighted_dist(dist, weights, npoint):
    """dist (B, N, N), weights (B, N) -> (B, npoint) int32."""
    return ops.furthest_point_sample_matrix(dist, npoint, weights=weights)


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B, C, N), idx (B, npoint) -> (B, C, npoint)."""
        ctx.for_backwards = (idx, features.shape[2])
        return ops.group_points(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        idx, n = ctx.for_backwards
        return ops.group_points_bwd(grad_out, idx, n), None


gather_operation = GatherOperation.apply


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        """features (B, C, N), idx (B, npoint, nsample) -> (B, C, npoint, nsample)."""
        ctx.for_backwards = (idx, features.shape[2])
        return ops.group_points(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        idx, n = ctx.for_backwards
        return ops.group_points_bwd(grad_out, idx, n), None


grouping_operation = GroupingOperation.apply


class ThreeNN(Function):
    @staticmethod
    def forward(ctx, unknown, known):
        """unknown (B, N, 3), known (B, M, 3) -> dist (B, N, 3) L2 distances, idx (B, N, 3) int32."""
        dist2, idx = ops.three_nn(unknown, known)
        return torch.sqrt(dist2), idx

    @staticmethod
    def backward(ctx, a=None, b=None):
        return None, None


three_nn = ThreeNN.apply


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        """features (B, C, M), idx / weight (B, n, 3) -> (B, C, n)."""
        ctx.three_interpolate_for_backward = (idx, weight, features.shape[2])
        return ops.three_interpolate(features, idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight, m = ctx.three_interpolate_for_backward
        return ops.three_interpolate_bwd(grad_out, idx, weight, m), None, None


three_interpolate = ThreeInterpolate.apply


@torch.no_grad()
def ball_query(radius, nsample, xyz, new_xyz):
    """-> idx_cnt (B, npoint) hits kept, idx (B, npoint, nsample) int32 of the points with d^2 < radius^2."""
    return ops.ball_query(xyz, new_xyz, nsample, radius)


@torch.no_grad()
def ball_query_dilated(radius_in, radius_out, nsample, xyz, new_xyz):
    """-> idx_cnt, idx of the points with radius_in^2 <= d^2 < radius_out^2."""
    return ops.ball_query(xyz, new_xyz, nsample, radius_out, r_in=radius_in)


def _group(idx, xyz, new_xyz, features, use_xyz):
    grouped_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx)      # (B, 3, npoint, nsample)
    grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
    if features is not None:
        grouped_features = grouping_operation(features, idx)
        new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if use_xyz else grouped_features
    else:
        assert use_xyz, "Cannot have not features and not use xyz as a feature!"
        new_features = grouped_xyz
    return new_features, grouped_xyz


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """xyz (B, N, 3), new_xyz (B, npoint, 3), features (B, C, N) -> idx_cnt (B, npoint),
        new_features (B, 3 + C, npoint, nsample), grouped_xyz (B, 3, npoint, nsample)."""
        idx_cnt, idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        new_features, grouped_xyz = _group(idx, xyz, new_xyz, features, self.use_xyz)
        return idx_cnt, new_features, grouped_xyz


class QueryAndGroupDilated(nn.Module):
    def __init__(self, radius_in, radius_out, nsample, use_xyz=True):
        super().__init__()
        self.radius_in, self.radius_out, self.nsample, self.use_xyz = radius_in, radius_out, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """As QueryAndGroup, over the shell radius_in <= d < radius_out."""
        idx_cnt, idx = ball_query_dilated(self.radius_in, self.radius_out, self.nsample, xyz, new_xyz)
        new_features, grouped_xyz = _group(idx, xyz, new_xyz, features, self.use_xyz)
        return idx_cnt, new_features, grouped_xyz


class GroupAll(nn.Module):
    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """xyz (B, N, 3), new_xyz ignored, features (B, C, N) -> (B, 3 + C, 1, N)."""
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped_features = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features


class GroupProject(Function):
    @staticmethod
    def forward(ctx, features, wf, wx, xyz, ctr, idx, empty, batch):
        """The first 1x1 conv of a grouper on the grouped tensor, without building it (spx.h §13):
        features (N, C) source rows or None, wf (Cout, C) or None, wx (Cout, 3) or None, xyz (N, 3), ctr (B * npoint, 3),
        idx (B * npoint, S) global rows, empty (B * npoint) bool or None -> (B, Cout, npoint, S)
        = wf · features[idx] + wx · (xyz[idx] - ctr), 0 in empty balls."""
        if (xyz is not None and xyz.requires_grad) or (ctr is not None and ctr.requires_grad):
            raise RuntimeError("group_project: coordinates carry no gradient (they come from sampling); detach them")
        p = torch.mm(features, wf.t()) if wf is not None else None
        ctx.save_for_backward(features, wf, xyz, ctr, idx, empty)
        ctx.has_wx = wx is not None
        ctx.n_src = features.shape[0] if features is not None else xyz.shape[0]
        return ops.group_project(p, wx, xyz, ctr, idx, empty, batch)

    @staticmethod
    def backward(ctx, grad_out):
        features, wf, xyz, ctr, idx, empty = ctx.saved_tensors
        need_f, need_wf, need_wx = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_dp = wf is not None and (need_f or need_wf)
        need_dwx = ctx.has_wx and need_wx
        if not (need_dp or need_dwx):
            return (None,) * 8
        dpt, dwx = ops.group_project_bwd(grad_out, xyz if need_dwx else None, ctr if need_dwx else None, idx, empty,
                                         ctx.n_src, need_dp=need_dp, need_dwx=need_dwx)
        d_f = torch.mm(dpt.t(), wf) if need_dp and need_f else None
        d_wf = torch.mm(dpt, features) if need_dp and need_wf else None
        return d_f, d_wf, dwx, None, None, None, None, None


def group_project(features, wf, wx, xyz, ctr, idx, empty, batch):
    """GroupProject.apply; see there."""
    return GroupProject.apply(features, wf, wx, xyz, ctr, idx, empty, batch)
