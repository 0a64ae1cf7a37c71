"""roipoint_pool3d, host side (reference pcdet/ops/roipoint_pool3d/roipoint_pool3d_utils.py).

RoIPointPool3d has the reference's constructor and returns (pooled_features, pooled_empty_flag) like it.
roipoint_pool3d_torch is the op as a torch composition with no host read, pinned bit for bit to the numpy restatement
tests/roipoint_pool3d_ref.py; RoIPointPool3d runs it for CPU tensors.  There is no HIP kernel for this op yet, and the
composition is not a stand-in for one: RoIPointPool3d raises NotImplementedError for device tensors.

Semantics: the box grows by float32 adds of the extra width; a point is inside by the test of csrc/box_inside.h; per
(frame, box) the first min(cnt, S) inside points in ascending index fill the first slots, slot k >= cnt repeats slot
k % cnt, an empty box gives flag 1 and a block of zeros.

Deliberate differences: pool_extra_width may be a scalar or three values (the reference's scalar default cannot run
through its own enlarge_box3d); boxes may have more than seven columns; the op is forward only and no input receives a
gradient (the reference's backward raises)."""
import numpy as np
import torch
import torch.nn as nn

__all__ = ["RoIPointPool3d", "roipoint_pool3d_torch"]

_MARGIN = float(np.float32(1e-5))      # the reference's `const float MARGIN = 1e-5`, widened for the double compare


def _three(extra_width):
    w = [float(v) for v in extra_width] if isinstance(extra_width, (list, tuple)) else [float(extra_width)] * 3
    if len(w) != 3 or not all(v >= 0.0 for v in w):
        raise ValueError("pool_extra_width must be a non-negative scalar or three non-negative values, got %r"
                         % (extra_width,))
    return w


def inside_mask(points, boxes3d, extra_width):
    """points (B, N, 3), boxes3d (B, M, >= 7) -> (B, M, N) bool: the inside test of csrc/box_inside.h in its own
    arithmetic (float32 local coordinates, one rounding per operation; limits compared in float64)."""
    w = _three(extra_width)
    p, b = points.float(), boxes3d.float()
    x, y, z = (p[:, None, :, k] for k in range(3))
    cx, cy, cz, dx, dy, dz, rz = (b[:, :, k, None] for k in range(7))
    dx, dy, dz = dx + w[0], dy + w[1], dz + w[2]                      # float32 adds
    cosa, sina = torch.cos(-rz.double()).float(), torch.sin(-rz.double()).float()
    sx, sy = x - cx, y - cy
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    zin = ~((z - cz).abs().double() > dz.double() / 2.0)
    return zin & (lx.abs().double() < dx.double() / 2.0 + _MARGIN) & (ly.abs().double() < dy.double() / 2.0 + _MARGIN)


def roipoint_pool3d_torch(points, point_features, boxes3d, pool_extra_width, num_sampled_points):
    """-> pooled_features (B, M, S, 3 + C), pooled_empty_flag (B, M) int32, equal to the restatement bit for bit on
    float32 inputs: a (B, M, N) inside mask, a cumulative count for the slots (slot k is the first point whose count reaches
    k + 1), slot k >= cnt taken from slot k % cnt, empty RoIs zeroed.  The inside test always runs on the float32
    values; the rows are gathered in the inputs' dtype (float64 in, float64 out)."""
    s = int(num_sampled_points)
    p, f = points.detach(), point_features.detach()
    bsz, n = p.shape[:2]
    m, c = boxes3d.shape[1], f.shape[2]
    if n == 0 or m == 0 or bsz == 0:
        return f.new_zeros((bsz, m, s, 3 + c)), torch.ones((bsz, m), dtype=torch.int32, device=p.device)
    inside = inside_mask(p, boxes3d.detach(), pool_extra_width)
    count = inside.cumsum(dim=-1, dtype=torch.int32)                   # (B, M, N), non-decreasing
    cnt = count[:, :, -1]                                              # (B, M)
    slots = torch.arange(s, device=p.device, dtype=torch.int32)
    src = slots[None, None, :] % torch.clamp(torch.clamp(cnt, max=s), min=1)[:, :, None]
    idx = torch.searchsorted(count, (src + 1).contiguous()).clamp(max=n - 1)      # (B, M, S) point indices
    frame = torch.arange(bsz, device=p.device)[:, None, None]
    pooled = torch.cat((p[frame, idx].to(f.dtype), f[frame, idx]), dim=-1)
    live = cnt > 0
    pooled = torch.where(live[:, :, None, None], pooled, torch.zeros_like(pooled))
    return pooled, (~live).int()


class RoIPointPool3d(nn.Module):
    def __init__(self, num_sampled_points=64, pool_extra_width=1.0):
        super().__init__()
        self.num_sampled_points = num_sampled_points
        self.pool_extra_width = pool_extra_width

    def forward(self, points, point_features, boxes3d):
        """
        Args:
            points: (B, N, 3)
            point_features: (B, N, C)
            boxes3d: (B, M, 7 + ...), [x, y, z, dx, dy, dz, heading]

        Returns:
            pooled_features: (B, M, num_sampled_points, 3 + C)
            pooled_empty_flag: (B, M) int32
        """
        assert points.dim() == 3 and points.shape[2] == 3
        if points.is_cuda:
            raise NotImplementedError("RoIPointPool3d: roipoint_pool3d has no HIP kernel yet; only CPU tensors are served")
        return roipoint_pool3d_torch(points, point_features, boxes3d, self.pool_extra_width, self.num_sampled_points)
