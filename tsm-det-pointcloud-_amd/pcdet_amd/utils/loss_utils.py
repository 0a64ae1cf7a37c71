"""Losses of the anchor head (semantics of reference pcdet/utils/loss_utils.py:9-77,140-209,310-338).
Device-agnostic: nothing is moved with .cuda() at construction."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


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
    """Constructed by the fast_cpc point head (reference loss_utils.py:339).  Holds no parameters or buffers; its
    forward belongs to the point head's training path, which is not ported yet."""

    def forward(self, input, target, weights):
        raise NotImplementedError('WeightedBinaryCrossEntropyLoss.forward: point-head training is not ported')


class PointSASALoss(nn.Module):
    """The reference's layer-wise SASA segmentation loss (loss_utils.py:545-704) up to its targets: the constructor
    (no parameters or buffers), assign_target and forward, which assigns the targets of every weighted layer, one HIP
    launch per layer for the whole batch and no host read.  loss_forward, the loss itself, is not ported yet."""

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
