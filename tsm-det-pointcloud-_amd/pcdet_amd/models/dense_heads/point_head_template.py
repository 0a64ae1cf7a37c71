"""PointHeadTemplate (reference pcdet/models/dense_heads/point_head_template.py): loss-module construction,
make_fc_layers and generate_predicted_boxes of the point heads; assign_stack_targets and get_cls_layer_loss for the
case PointHeadSimple uses (ignore flag, no ball constraint, no box or part labels), for the whole batch with no per-frame
loop and no host read.  The other target options and loss terms are not ported and raise by name."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...ops.roiaware_pool3d import roiaware_pool3d_utils
from ...utils import loss_utils


class PointHeadTemplate(nn.Module):
    def __init__(self, model_cfg, num_class):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class

        self.build_losses(self.model_cfg.LOSS_CONFIG)
        self.forward_ret_dict = None

    def build_losses(self, losses_cfg):
        self.add_module('fg_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        self.add_module('corner_loss_func', loss_utils.WeightedSmoothL1Loss(code_weights=[1] * 24))
        self.add_module('center_loss_func', loss_utils.WeightedSmoothL1Loss(code_weights=[1, 1, 1]))
        reg_loss_type = losses_cfg.get('LOSS_REG', None)
        if reg_loss_type == 'l1':
            self.reg_loss_func = F.l1_loss
        elif reg_loss_type == 'WeightedSmoothL1Loss':
            self.reg_loss_func = loss_utils.WeightedSmoothL1Loss(
                code_weights=losses_cfg.LOSS_WEIGHTS.get('code_weights', None))
        else:
            self.reg_loss_func = F.smooth_l1_loss

    @staticmethod
    def make_fc_layers(fc_cfg, input_channels, output_channels):
        fc_layers = []
        c_in = input_channels
        for k in range(0, fc_cfg.__len__()):
            fc_layers.extend([
                nn.Linear(c_in, fc_cfg[k], bias=False),
                nn.BatchNorm1d(fc_cfg[k]),
                nn.ReLU(),
            ])
            c_in = fc_cfg[k]
        fc_layers.append(nn.Linear(c_in, output_channels, bias=True))
        return nn.Sequential(*fc_layers)

    def assign_stack_targets(self, points, gt_boxes, extend_gt_boxes=None,
                             ret_box_labels=False, ret_part_labels=False,
                             set_ignore_flag=True, use_ball_constraint=False, central_radius=2.0):
        """points (B * K, 4) [bs_idx, x, y, z] in B equal, contiguous frames; gt_boxes, extend_gt_boxes (B, M, 8 | 10) ->
        point_cls_labels (B * K) long: the class of the first GT box holding the point (1 when class agnostic), -1 for a
        point inside the enlarged box only, 0 elsewhere.  Two points_in_boxes_gpu calls on the (B, K, 3) view."""
        assert len(points.shape) == 2 and points.shape[1] == 4, 'points.shape=%s' % str(points.shape)
        assert len(gt_boxes.shape) == 3 and gt_boxes.shape[2] in (8, 10), 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        if ret_box_labels:
            raise NotImplementedError('assign_stack_targets: ret_box_labels is not ported')
        if ret_part_labels:
            raise NotImplementedError('assign_stack_targets: ret_part_labels is not ported')
        if use_ball_constraint or not set_ignore_flag:
            raise NotImplementedError('assign_stack_targets: use_ball_constraint is not ported (set_ignore_flag only)')
        assert extend_gt_boxes is not None and extend_gt_boxes.shape == gt_boxes.shape, 'extend_gt_boxes'
        batch_size = gt_boxes.shape[0]
        assert points.shape[0] % batch_size == 0, 'points: %d rows in %d frames' % (points.shape[0], batch_size)
        pts = points[:, 1:4].reshape(batch_size, -1, 3).contiguous()
        box_idxs_of_pts = roiaware_pool3d_utils.points_in_boxes_gpu(pts, gt_boxes[:, :, 0:7].contiguous()).long()
        extend_box_idxs_of_pts = roiaware_pool3d_utils.points_in_boxes_gpu(
            pts, extend_gt_boxes[:, :, 0:7].contiguous()).long()
        fg_flag = box_idxs_of_pts >= 0
        ignore_flag = fg_flag ^ (extend_box_idxs_of_pts >= 0)
        labels = torch.where(ignore_flag, -torch.ones_like(box_idxs_of_pts), torch.zeros_like(box_idxs_of_pts))
        if self.num_class == 1:
            fg_labels = torch.ones_like(box_idxs_of_pts)
        else:
            fg_labels = torch.gather(gt_boxes[:, :, -1].long(), 1, box_idxs_of_pts.clamp(min=0))
        labels = torch.where(fg_flag, fg_labels, labels)
        return {'point_cls_labels': labels.view(-1), 'point_box_labels': None, 'point_part_labels': None}

    def get_cls_layer_loss(self, tb_dict=None):
        """The focal class loss over the points that are not ignored, normalised by the number of positives; tb_dict
        holds 0-dim tensors (no host read)."""
        point_cls_labels = self.forward_ret_dict['point_cls_labels'].view(-1)
        point_cls_preds = self.forward_ret_dict['point_cls_preds'].view(-1, self.num_class)

        positives = (point_cls_labels > 0)
        negative_cls_weights = (point_cls_labels == 0) * 1.0
        cls_weights = (negative_cls_weights + 1.0 * positives).to(point_cls_preds.dtype)
        pos_normalizer = positives.sum(dim=0).to(point_cls_preds.dtype)
        cls_weights = cls_weights / torch.clamp(pos_normalizer, min=1.0)

        one_hot_targets = point_cls_preds.new_zeros(*list(point_cls_labels.shape), self.num_class + 1)
        one_hot_targets.scatter_(-1, (point_cls_labels * (point_cls_labels >= 0).long()).unsqueeze(dim=-1).long(), 1.0)
        one_hot_targets = one_hot_targets[..., 1:]
        cls_loss_src = self.cls_loss_func(point_cls_preds, one_hot_targets, weights=cls_weights)
        point_loss_cls = cls_loss_src.sum()

        loss_weights_dict = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        point_loss_cls = point_loss_cls * loss_weights_dict['point_cls_weight']
        if tb_dict is None:
            tb_dict = {}
        tb_dict.update({
            'point_loss_cls': point_loss_cls.detach(),
            'point_pos_num': pos_normalizer.detach()
        })
        return point_loss_cls, tb_dict

    def generate_predicted_boxes(self, points, point_cls_preds, point_box_preds):
        """points (N, 3), point_cls_preds (N, num_class), point_box_preds (N, code_size) ->
        point_cls_preds (N, num_class), point_box_preds (N, 7 + C) decoded at the points."""
        _, pred_classes = point_cls_preds.max(dim=-1)
        point_box_preds = self.box_coder.decode_torch(point_box_preds, points, pred_classes + 1)
        return point_cls_preds, point_box_preds

    def forward(self, **kwargs):
        raise NotImplementedError
