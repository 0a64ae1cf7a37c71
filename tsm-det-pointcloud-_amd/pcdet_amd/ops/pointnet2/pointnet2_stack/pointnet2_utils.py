"""pointnet2_stack on libspx (include/spx.h §18; reference pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py).

Same public names, call signatures and return values as the reference module; every op runs the HIP kernels of
csrc/pointnet2_stack.hip on stacked (N1 + N2 + ..., C) tensors with per-frame counts.  Sampling, ball query and three-NN
return integer tensors and carry no gradient; grouping and three-point interpolation are autograd Functions whose
backward sums duplicate indices in a fixed order (deterministic, unlike the reference's atomicAdd).

The reference asserts `x.shape[0] == x_batch_cnt.sum()` in several places, one host read each.  Those asserts are gone:
the counts stay on the device, and a tensor may have MORE rows than its counts sum to (static capacity, so that a step
can be captured in a graph and replayed with other counts).  Such rows are dead: a dead query row gets idx 0 and an
empty-ball mask of True (three_nn: idx 0, distance inf), a dead output row of grouping or interpolation is 0, a dead
source row gets a zero gradient.  Counts that sum to more than the rows are clamped by the kernels."""
import torch
import torch.nn as nn
from torch.autograd import Function

from spx import ops

from ..pointnet2_batch import pointnet2_utils as _batch_utils

__all__ = [
    "ball_query", "grouping_operation", "QueryAndGroup", "farthest_point_sample", "furthest_point_sample",
    "stack_farthest_point_sample", "three_nn", "three_interpolate", "three_nn_for_vector_pool_by_two_step",
    "vector_pool_with_voxel_query_op",
]


@torch.no_grad()
def ball_query(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), counts (batch_size,) int32 -> idx (M1 + M2 ..., nsample) int32
    frame-local rows (the first nsample points closer than radius in ascending order, unfilled slots = the first of
    them, an empty ball all 0) and empty_ball_mask (M1 + M2 ...) bool.  Dead rows: idx 0, mask True."""
    return ops.stack_ball_query(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, radius, nsample)


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, features_batch_cnt, idx, idx_batch_cnt):
        """features (N1 + N2 ..., C), idx (M1 + M2 ..., nsample) frame-local -> (M1 + M2 ..., C, nsample).  Dead rows of
        idx give 0; dead rows of features are not read and get a zero gradient."""
        ctx.for_backwards = (features.shape[0], idx, features_batch_cnt, idx_batch_cnt)
        return ops.stack_group_points(features, features_batch_cnt, idx, idx_batch_cnt)

    @staticmethod
    def backward(ctx, grad_out):
        n, idx, features_batch_cnt, idx_batch_cnt = ctx.for_backwards
        return ops.stack_group_points_bwd(grad_out, features_batch_cnt, idx, idx_batch_cnt, n), None, None, None


grouping_operation = GroupingOperation.apply


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None):
        """-> new_features (M1 + M2 ..., [3 +] C, nsample): the grouped xyz relative to the centre, then the grouped
        features, both 0 for empty balls (and dead rows); idx (M1 + M2 ..., nsample).  No host read."""
        idx, empty_ball_mask = ball_query(self.radius, self.nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        empty = empty_ball_mask[:, None, None]
        grouped_xyz = grouping_operation(xyz, xyz_batch_cnt, idx, new_xyz_batch_cnt)   # (M1 + M2, 3, nsample)
        grouped_xyz = (grouped_xyz - new_xyz.unsqueeze(-1)).masked_fill(empty, 0)
        if features is not None:
            grouped_features = grouping_operation(features, xyz_batch_cnt, idx, new_xyz_batch_cnt).masked_fill(empty, 0)
            new_features = torch.cat([grouped_xyz, grouped_features], dim=1) if self.use_xyz else grouped_features
        else:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
            new_features = grouped_xyz
        return new_features, idx


# the batch-shaped (B, N, 3) sampler of the stack module is the pointnet2_batch kernel (spx_furthest_point_sample)
farthest_point_sample = furthest_point_sample = _batch_utils.furthest_point_sample


@torch.no_grad()
def stack_farthest_point_sample(xyz, xyz_batch_cnt, npoint, total=None):
    """xyz (N1 + N2 ..., 3), counts (batch_size,), npoint an int (per frame), a list or an int tensor (batch_size,) ->
    (sum of npoint,) int32 GLOBAL rows, frame after frame; the first pick of a frame is its first row.  An int or a list
    costs no host read; a tensor costs the one read of its sum that sizes the output, as in the reference, unless the
    caller passes that sum as `total` (a device tensor with its sum known on the host: no read, no host-to-device copy,
    so the call can be captured in a graph)."""
    batch_size = xyz_batch_cnt.shape[0]
    if isinstance(npoint, torch.Tensor):
        total = int(npoint.sum().item()) if total is None else int(total)
        npoint = npoint.to(device=xyz.device, dtype=torch.int32)
    else:
        if not isinstance(npoint, (list, tuple)):
            npoint = [npoint] * batch_size
        total = int(sum(npoint))
        npoint = torch.tensor(list(npoint), dtype=torch.int32).to(xyz.device, non_blocking=True)
    return ops.stack_furthest_point_sample(xyz, xyz_batch_cnt, npoint, total)


@torch.no_grad()
def three_nn(unknown, unknown_batch_cnt, known, known_batch_cnt):
    """unknown (N1 + N2 ..., 3), known (M1 + M2 ..., 3) -> dist (N1 + N2 ..., 3) L2 distances and idx (N1 + N2 ..., 3)
    int32 GLOBAL known rows of the three nearest known points of the same frame.  A frame with fewer than three known
    points leaves inf and its first known row in the unfilled slots; dead rows hold inf and 0."""
    assert unknown.dim() == 2 and unknown.shape[1] == 3 and known.dim() == 2 and known.shape[1] == 3
    dist2, idx = ops.stack_three_nn(unknown, unknown_batch_cnt, known, known_batch_cnt)
    return torch.sqrt(dist2), idx


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight, batch_cnt=None):
        """features (M1 + M2 ..., C), idx / weight (N1 + N2 ..., 3) -> (N1 + N2 ..., C).  batch_cnt (optional, not in the
        reference): the counts of the N side; with it the rows past their sum are 0 whatever their weights hold."""
        assert idx.shape[0] == weight.shape[0] and idx.shape[1] == weight.shape[1] == 3
        ctx.three_interpolate_for_backward = (idx, weight, features.shape[0], batch_cnt)
        return ops.stack_three_interpolate(features, idx, weight, batch_cnt)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight, m, batch_cnt = ctx.three_interpolate_for_backward
        return ops.stack_three_interpolate_bwd(grad_out, idx, weight, m, batch_cnt), None, None, None


three_interpolate = ThreeInterpolate.apply


def three_nn_for_vector_pool_by_two_step(*args, **kwargs):
    raise NotImplementedError("three_nn_for_vector_pool_by_two_step: vector pooling (vector_pool_gpu.cu, PV-RCNN++) is not "
                              "ported")


def vector_pool_with_voxel_query_op(*args, **kwargs):
    raise NotImplementedError("vector_pool_with_voxel_query_op: vector pooling (vector_pool_gpu.cu, PV-RCNN++) is not "
                              "ported")
