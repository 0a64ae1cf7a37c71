"""roiaware_pool3d on libspx (include/spx.h §12; reference pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py).

Same public names, argument order, shapes, dtypes and return values as the reference module.  points_in_boxes_gpu and
RoI-aware pooling run the HIP kernels of csrc/roiaware_pool3d.hip; the pooling backward sums over RoIs in a fixed
ascending order (deterministic, unlike the reference's atomicAdd).  points_in_boxes_cpu is the reference's host op
(dataset side, margin 1e-2), restated in vectorised numpy: it is not a fallback of the GPU op."""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from spx import ops

from ...utils import common_utils

__all__ = ["points_in_boxes_cpu", "points_in_boxes_gpu", "points_in_boxes_stack", "RoIAwarePool3d",
           "RoIAwarePool3dFunction"]

_CPU_MARGIN = np.float64(np.float32(1e-2))   # the reference's `const float MARGIN = 1e-2` widened for the double compare
_CPU_CHUNK = 1 << 22                          # (box, point) pairs evaluated at once


def _in_boxes_cpu(pts, boxes):
    """(P, 3), (N, 7) float32 -> (N, P) bool, the reference's check_pt_in_box3d_cpu in float32 / float64 as written."""
    x, y, z = (pts[None, :, k] for k in range(3))
    cx, cy, cz, dx, dy, dz, rz = (boxes[:, k, None] for k in range(7))
    cosa = np.cos(-rz.astype(np.float64)).astype(np.float32)
    sina = np.sin(-rz.astype(np.float64)).astype(np.float32)
    sx, sy = x - cx, y - cy
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    with np.errstate(invalid="ignore"):
        zin = ~(np.abs(z - cz).astype(np.float64) > dz.astype(np.float64) / 2.0)
        return zin & (np.abs(lx).astype(np.float64) < dx.astype(np.float64) / 2.0 + _CPU_MARGIN) \
            & (np.abs(ly).astype(np.float64) < dy.astype(np.float64) / 2.0 + _CPU_MARGIN)


def points_in_boxes_cpu(points, boxes):
    """
    Args:
        points: (num_points, 3)
        boxes: [x, y, z, dx, dy, dz, heading], (x, y, z) is the box center, each box DO NOT overlaps
    Returns:
        point_indices: (N, num_points) int32, 1 where the point lies in the box
    """
    assert boxes.shape[1] == 7
    assert points.shape[1] == 3
    points, is_numpy = common_utils.check_numpy_to_torch(points)
    boxes, is_numpy = common_utils.check_numpy_to_torch(boxes)
    pts = points.detach().float().contiguous().numpy()
    bxs = boxes.detach().float().contiguous().numpy()
    out = np.zeros((bxs.shape[0], pts.shape[0]), dtype=np.int32)
    step = max(1, _CPU_CHUNK // max(1, bxs.shape[0]))
    for s in range(0, pts.shape[0], step):
        out[:, s:s + step] = _in_boxes_cpu(pts[s:s + step], bxs)
    point_indices = torch.from_numpy(out)
    return point_indices.numpy() if is_numpy else point_indices


def points_in_boxes_gpu(points, boxes):
    """
    :param points: (B, M, 3)
    :param boxes: (B, T, 7), num_valid_boxes <= T
    :return box_idxs_of_pts: (B, M), default background = -1
    """
    assert boxes.shape[0] == points.shape[0]
    assert boxes.shape[2] == 7 and points.shape[2] == 3
    return ops.points_in_boxes(points, boxes)


def points_in_boxes_stack(points_bxyz, boxes):
    """
    :param points_bxyz: (N1 + N2 + ..., 4) [bs_idx, x, y, z], frames of any length
    :param boxes: (B, T, 7), num_valid_boxes <= T
    :return box_idxs_of_pts: (N1 + N2 + ...), the first box of the point's own frame holding it, background = -1
    """
    assert boxes.shape[2] == 7 and points_bxyz.shape[1] == 4
    return ops.points_in_boxes_stack(points_bxyz, boxes)


class RoIAwarePool3d(nn.Module):
    def __init__(self, out_size, max_pts_each_voxel=128):
        super().__init__()
        self.out_size = out_size
        self.max_pts_each_voxel = max_pts_each_voxel

    def forward(self, rois, pts, pts_feature, pool_method='max'):
        assert pool_method in ['max', 'avg']
        return RoIAwarePool3dFunction.apply(rois, pts, pts_feature, self.out_size, self.max_pts_each_voxel, pool_method)


class RoIAwarePool3dFunction(Function):
    @staticmethod
    def forward(ctx, rois, pts, pts_feature, out_size, max_pts_each_voxel, pool_method):
        """
        Args:
            rois: (N, 7) [x, y, z, dx, dy, dz, heading] (x, y, z) is the box center
            pts: (npoints, 3)
            pts_feature: (npoints, C)
            out_size: int or tuple, like 7 or (7, 7, 7)
            max_pts_each_voxel: each voxel keeps the first max_pts_each_voxel - 1 points
            pool_method: 'max' or 'avg'

        Returns:
            pooled_features: (N, out_x, out_y, out_z, C)
        """
        assert rois.shape[1] == 7 and pts.shape[1] == 3
        if isinstance(out_size, int):
            out_x = out_y = out_z = out_size
        else:
            assert len(out_size) == 3
            for k in range(3):
                assert isinstance(out_size[k], int)
            out_x, out_y, out_z = out_size

        pool_method = {'max': 0, 'avg': 1}[pool_method]
        pooled, argmax, pt_cell, vox_cnt = ops.roiaware_pool3d_fwd(rois, pts, pts_feature, (out_x, out_y, out_z),
                                                                   max_pts_each_voxel, pool_method)
        ctx.roiaware_pool3d_for_backward = (argmax, pt_cell, vox_cnt, pool_method)
        return pooled

    @staticmethod
    def backward(ctx, grad_out):
        """
        :param grad_out: (N, out_x, out_y, out_z, C)
        :return:
            grad_in: (npoints, C)
        """
        argmax, pt_cell, vox_cnt, pool_method = ctx.roiaware_pool3d_for_backward
        grad_in = ops.roiaware_pool3d_bwd(grad_out.contiguous(), argmax, pt_cell, vox_cnt, pool_method)
        return None, None, grad_in, None, None, None
