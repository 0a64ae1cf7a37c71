"""Losses of the anchor head (semantics of reference pcdet/utils/loss_utils.py:9-77,140-209,310-338) and of the
fast_cpc point head (WeightedBinaryCrossEntropyLoss, PointSASALoss: :339-362, :545-753).
Device-agnostic: nothing is moved with .cuda() at construction."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import common_utils


class SigmoidFocalClassificationLoss(nn.Module):
    def __init__(self, gamma=2.0, alpha=0.25):
        super().__init__()
        self.alpha, self.gamma = alpha, gamma

    @staticmethod
    def sigmoid_cross_entropy_with_logits(input, target):
        # max(x,0) - x*z + log(1 + exp(-|x|))
        return torch.clamp(input, min=0) - input * target + torch.log1p(torch.exp(-torch.abs(input)))

    def forward(self, input, target, weights):
        p = torch.sigmoid(input)
        alpha_w = target * self.alpha + (1 - target) * (1 - self.alpha)
        pt = target * (1.0 - p) + (1.0 - target) * p
        loss = alpha_w * torch.pow(pt, self.gamma) * self.sigmoid_cross_entropy_with_logits(input, target)
        if weights.dim() == 2 or (weights.dim() == 1 and target.dim() == 2):
            weights = weights.unsqueeze(-1)
        assert weights.dim() == loss.dim()
        return loss * weights


class WeightedSmoothL1Loss(nn.Module):
    def __init__(self, beta=1.0 / 9.0, code_weights=None):
        super().__init__()
        self.beta = beta
        if code_weights is not None:
            self.register_buffer("code_weights", torch.from_numpy(np.array(code_weights, dtype=np.float32)),
                                 persistent=False)
        else:
            self.code_weights = None

    @staticmethod
    def smooth_l1_loss(diff, beta):
        if beta < 1e-5:
            return torch.abs(diff)
        n = torch.abs(diff)
        return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)

    def forward(self, input, target, weights=None):
        target = torch.where(torch.isnan(target), input, target)
        diff = input - target
        if self.code_weights is not None:
            diff = diff * self.code_weights.to(diff.device).view(1, 1, -1)
        loss = self.smooth_l1_loss(diff, self.beta)
        if weights is not None:
            assert weights.shape[0] == loss.shape[0] and weights.shape[1] == loss.shape[1]
            loss = loss * weights.unsqueeze(-1)
        return loss


class WeightedCrossEntropyLoss(nn.Module):
    def forward(self, input, target, weights):
        return F.cross_entropy(input.permute(0, 2, 1), target.argmax(dim=-1), reduction="none") * weights


class WeightedBinaryCrossEntropyLoss(nn.Module):
    """Binary cross entropy with logits, mean over the classes, times the row weights (reference loss_utils.py:339-362).
    input, target (..., #classes), weights (...) -> (...).  No parameters or buffers."""

    def forward(self, input, target, weights):
        return F.binary_cross_entropy_with_logits(input, target, reduction='none').mean(dim=-1) * weights


class _FusedPointSegLoss(torch.autograd.Function):
    """One layer's 0-d loss with d(loss)/d(scores) from one libspx launch group (csrc/point_loss.hip); backward scales
    the saved gradient."""

    @staticmethod
    def forward(ctx, scores, labels, num_class, func, layer_weight):
        from spx import ops
        loss, d_scores = ops.point_seg_loss(scores, labels, num_class, func, layer_weight)
        ctx.save_for_backward(d_scores)
        ctx.shape = scores.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_scores, = ctx.saved_tensors
        return (d_scores * g).view(ctx.shape), None, None, None, None


class _FusedCenterHeadLoss(torch.autograd.Function):
    """One centre head's two 0-d losses (hm_loss * cls_weight, loc_loss * loc_weight) with their gradients w.r.t. the
    heatmap logits and the regression maps from one libspx launch group (csrc/center_loss.hip, no host read, no float
    atomics); backward scales the saved gradients.  The normalisers are applied inside the op (count first), so the
    saved gradients are final.  apply(heatmap, target_boxes, inds, masks, code_weights, cls_weight, loc_weight, hm,
    *regs) -> (hm_loss, loc_loss); code_weights: host floats."""

    @staticmethod
    def forward(ctx, heatmap, target_boxes, inds, masks, code_weights, cls_weight, loc_weight, hm, *regs):
        from spx import ops
        losses, _reg_loss, d_hm, d_regs = ops.center_head_loss(hm, heatmap, regs, target_boxes, inds, masks,
                                                               code_weights, cls_weight, loc_weight)
        ctx.save_for_backward(d_hm, *d_regs)
        ctx.dtypes = [hm.dtype] + [t.dtype for t in regs]
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_hm, g_loc):
        d_hm, *d_regs = ctx.saved_tensors
        grads = [(d_hm * g_hm).to(ctx.dtypes[0])] + [(d * g_loc).to(t) for d, t in zip(d_regs, ctx.dtypes[1:])]
        return (None,) * 7 + tuple(grads)


class PointSASALoss(nn.Module):
    """The reference's layer-wise SASA segmentation loss (loss_utils.py:545-704) up to its targets: the constructor
    (no parameters or buffers), assign_target and forward, which assigns the targets of every weighted layer, one HIP
    launch per layer for the whole batch and no host read, and loss_forward, the loss of every layer that has scores and
    labels: fused (forward and gradient from csrc/point_loss.hip, no host read) or as the reference's torch composition."""

    def __init__(self, func='BCE', layer_weights=None, extra_width=None, set_ignore_flag=False, num_class=None):
        super().__init__()
        self.layer_weights = layer_weights
        if func == 'BCE':
            self.loss_func = WeightedBinaryCrossEntropyLoss()
        elif func == 'Focal':
            self.loss_func = SigmoidFocalClassificationLoss()
        else:
            raise NotImplementedError
        assert not set_ignore_flag or (set_ignore_flag and extra_width is not None)
        self.extra_width = extra_width
        self.set_ignore_flag = set_ignore_flag
        self.num_class = num_class

    def assign_target(self, points, gt_boxes):
        """points (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> point_cls_labels (.) long (0 background,
        -1 ignored), point_box_labels (., 7), point_part_labels (., 3)."""
        from ..models.dense_heads import point_targets
        return point_targets.sasa_assign_target(points, gt_boxes, extra_width=self.extra_width,
                                                set_ignore_flag=self.set_ignore_flag, num_class=self.num_class)

    def forward(self, l_points, l_scores, gt_boxes):
        """l_points: per layer (N, 4) [bs_idx, x, y, z]; l_scores: per layer (N, 1) or None; gt_boxes (B, M, 8) ->
        l_labels, l_boxes, l_parts.  As in the reference, a layer without scores or with weight 0 appends None to
        l_labels only."""
        l_labels, l_boxes, l_parts = [], [], []
        for i in range(len(self.layer_weights)):
            if l_scores[i] is None or self.layer_weights[i] == 0:
                l_labels.append(None)
                continue
            li_labels, li_boxes, li_parts = self.assign_target(l_points[i], gt_boxes)
            l_labels.append(li_labels)
            l_boxes.append(li_boxes)
            l_parts.append(li_parts)
        return l_labels, l_boxes, l_parts

    def loss_forward(self, l_scores, l_labels, l_points, l_boxes, l_parts, fused=True):
        """l_scores: per layer (N, 1) or (N, num_class) logits or None; l_labels: per layer (N) long (> 0 the class, 0
        background, -1 ignored) or None -> per layer the 0-d layer_weight * sum / clamp(#labels >= 0, 1), or None.
        The target is the one-hot of the class without its background column; a one-column score meets every one of
        the num_class target columns (with 3 classes a foreground row is one positive and two negative terms).
        l_points, l_boxes and l_parts are not read, as in the reference.  fused needs GPU tensors."""
        focal = isinstance(self.loss_func, SigmoidFocalClassificationLoss)
        if fused and focal and (self.loss_func.alpha != 0.25 or self.loss_func.gamma != 2.0):
            raise NotImplementedError('fused SASA loss: focal alpha 0.25, gamma 2 only')
        l_loss = []
        for i in range(len(self.layer_weights)):
            li_scores, li_labels = l_scores[i], l_labels[i]
            if li_scores is None or li_labels is None:
                l_loss.append(None)
                continue
            if fused:
                l_loss.append(_FusedPointSegLoss.apply(li_scores, li_labels, self.num_class, int(focal),
                                                       float(self.layer_weights[i])))
                continue
            cls_weights = (li_labels >= 0).to(li_scores.dtype)
            one_hot = li_scores.new_zeros(*li_labels.shape, self.num_class + 1)
            one_hot.scatter_(-1, (li_labels * (li_labels > 0).long()).unsqueeze(-1), 1.0)
            one_hot = one_hot[:, 1:]
            li_loss = self.loss_func(li_scores.expand_as(one_hot)[None], one_hot[None], cls_weights.reshape(1, -1))
            l_loss.append(self.layer_weights[i] * li_loss.sum() / torch.clamp(cls_weights.sum(dim=0), min=1.0))
        return l_loss


# ------------------------------------------------------------------ centre head (reference loss_utils.py:420-542)

def neg_loss_cornernet(pred, gt, mask=None):
    """CornerNet's penalty-reduced focal loss: pred, gt (B, C, H, W), pred a probability, gt 1 exactly at the centres;
    mask (B, H, W) or None -> 0-d.  The value of the reference, which branches on `num_pos == 0` on the host; here the
    two branches are selected on the device, so the loss can be captured in a graph."""
    pos_inds = gt.eq(1).float()
    neg_inds = gt.lt(1).float()
    neg_weights = torch.pow(1 - gt, 4)
    pos_loss = torch.log(pred) * torch.pow(1 - pred, 2) * pos_inds
    neg_loss = torch.log(1 - pred) * torch.pow(pred, 2) * neg_weights * neg_inds
    if mask is not None:
        mask = mask[:, None, :, :].float()
        pos_loss = pos_loss * mask
        neg_loss = neg_loss * mask
        num_pos = (pos_inds.float() * mask).sum()
    else:
        num_pos = pos_inds.float().sum()
    pos_loss = pos_loss.sum()
    neg_loss = neg_loss.sum()
    return torch.where(num_pos == 0, -neg_loss, -(pos_loss + neg_loss) / num_pos.clamp_min(1.0))


class FocalLossCenterNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.neg_loss = neg_loss_cornernet

    def forward(self, out, target, mask=None):
        return self.neg_loss(out, target, mask=mask)


def _reg_loss(regr, gt_regr, mask):
    """L1 over the live slots: regr, gt_regr (B, K, D), mask (B, K) -> (D), each column's sum / max(#live, 1), with the
    reference's NaN mask (a NaN target zeroes the prediction's side only, so it still surfaces in the loss)."""
    num = mask.float().sum()
    mask = mask.unsqueeze(2).expand_as(gt_regr).float()
    isnotnan = (~torch.isnan(gt_regr)).float()
    mask = mask * isnotnan
    regr = regr * mask
    gt_regr = gt_regr * mask
    loss = torch.abs(regr - gt_regr)
    loss = loss.transpose(2, 0)
    loss = torch.sum(loss, dim=2)
    loss = torch.sum(loss, dim=1)
    return loss / torch.clamp_min(num, min=1.0)


class RegLossCenterNet(nn.Module):
    def forward(self, output, mask, ind=None, target=None):
        """output (B, D, H, W) with ind (B, K) flat cells, or (B, K, D) without; mask (B, K); target (B, K, D) -> (D)."""
        if ind is None:
            pred = output
        else:
            from ..models.model_utils.centernet_utils import _transpose_and_gather_feat
            pred = _transpose_and_gather_feat(output, ind)
        return _reg_loss(pred, target, mask)


_CORNER_TEMPLATE = {}


def _corners_3d(boxes3d):
    """(N, 7) -> (N, 8, 3) corners in the boxes' own dtype, the reference's boxes_to_corners_3d (box_utils.py:28-53)."""
    key = (boxes3d.device, boxes3d.dtype)
    template = _CORNER_TEMPLATE.get(key)
    if template is None:      # built once per device and dtype: a host-to-device copy cannot be part of a captured graph
        template = _CORNER_TEMPLATE[key] = boxes3d.new_tensor([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1],
                                                               [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]]) / 2
    corners = boxes3d[:, None, 3:6] * template[None]
    corners = common_utils.rotate_points_along_z(corners, boxes3d[:, 6])
    return corners + boxes3d[:, None, 0:3]


def get_corner_loss_lidar(pred_bbox3d, gt_bbox3d):
    """(N, 7), (N, 7) -> (N): smooth-L1 (beta 1) of the eight corner distances, the smaller of the distance to the ground
    truth and to the ground truth turned by pi, averaged over the corners (reference loss_utils.py:365-388)."""
    assert pred_bbox3d.shape[0] == gt_bbox3d.shape[0]
    pred_corners = _corners_3d(pred_bbox3d)
    gt_corners = _corners_3d(gt_bbox3d)
    gt_flip = torch.cat([gt_bbox3d[:, :6], gt_bbox3d[:, 6:7] + np.pi, gt_bbox3d[:, 7:]], dim=1)
    gt_corners_flip = _corners_3d(gt_flip)
    dist = torch.min(torch.norm(pred_corners - gt_corners, dim=2), torch.norm(pred_corners - gt_corners_flip, dim=2))
    return WeightedSmoothL1Loss.smooth_l1_loss(dist, beta=1.0).mean(dim=1)


def sigmoid_focal_cls_loss(input, target, gamma=2.0, alpha=0.25):
    """Element-wise sigmoid focal loss on logits with soft targets in [0, 1].  SECONDHead's IOU_LOSS 'focalbce' calls this
    name (reference second_head.py:169), but neither the fork nor upstream OpenPCDet defines it; this is
    SigmoidFocalClassificationLoss (:9-77) with unit weights, its defaults gamma 2 and alpha 0.25."""
    p = torch.sigmoid(input)
    alpha_w = target * alpha + (1 - target) * (1 - alpha)
    pt = target * (1.0 - p) + (1.0 - target) * p
    return alpha_w * torch.pow(pt, gamma) * SigmoidFocalClassificationLoss.sigmoid_cross_entropy_with_logits(input, target)
