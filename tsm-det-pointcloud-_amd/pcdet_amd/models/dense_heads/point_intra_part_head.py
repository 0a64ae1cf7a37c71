"""PointIntraPartOffsetHead (reference pcdet/models/dense_heads/point_intra_part_head.py:7-140, the fork's version with
its part labels of point_head_template.py:161-175): per point a foreground score and the intra-object part location.
Reference constructor signature and state_dict keys.

Departures, recorded in DESIGN.md §6l:
  * the fork hard-codes point_feature_layers as 64 -> FEATURES_FC -> 256 (make_fc_layers_v1) and always rewrites
    multi_scale_3d_features['x_points_mean' / 'x_points_max'].  With FEATURES_FC in the config that tree is built with 64
    generalised to input_channels; without it the FC stacks sit directly on input_channels (upstream OpenPCDet, the
    form UNetV2's 16 channels need).  x_points_* are rewritten only when present;
  * assign_targets is the head's own: two points_in_boxes_stack calls (GT and enlarged GT) over the ragged frames and a
    torch composition of the class and part labels for the whole batch, no per-frame loop, no host read
    (PointHeadTemplate.assign_stack_targets keeps refusing ret_part_labels);
  * get_part_layer_loss keeps 0-dim tensors in tb_dict (no .item());
  * TARGET_CONFIG.BOX_CODER (the box_layers branch) raises NotImplementedError."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...ops.roiaware_pool3d import roiaware_pool3d_utils
from ...utils import box_utils
from .point_head_template import PointHeadTemplate


class PointIntraPartOffsetHead(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        if self.model_cfg.TARGET_CONFIG.get('BOX_CODER', None) is not None:
            raise NotImplementedError('PointIntraPartOffsetHead: TARGET_CONFIG.BOX_CODER (box_layers) is not ported')
        self.box_layers = None
        features_fc = self.model_cfg.get('FEATURES_FC', None)
        head_channels = 256 if features_fc is not None else input_channels
        self.cls_layers = self.make_fc_layers(
            fc_cfg=self.model_cfg.CLS_FC,
            input_channels=head_channels,
            output_channels=num_class
        )
        self.part_reg_layers = self.make_fc_layers(
            fc_cfg=self.model_cfg.PART_FC,
            input_channels=head_channels,
            output_channels=3
        )
        if features_fc is not None:
            self.point_feature_layers = self.make_fc_layers_v1(
                fc_cfg=features_fc,
                input_channels=input_channels,
                output_channels=256,
                end_bn_active=True,
            )
        else:
            self.point_feature_layers = None

    @staticmethod
    def make_fc_layers_v1(fc_cfg, input_channels, output_channels, end_bn_active=False):
        fc_layers = []
        c_in = input_channels
        for k in range(0, fc_cfg.__len__()):
            fc_layers.extend([
                nn.Linear(c_in, fc_cfg[k], bias=False),
                nn.BatchNorm1d(fc_cfg[k]),
                nn.ReLU(),
            ])
            c_in = fc_cfg[k]
        if end_bn_active:
            fc_layers.append(nn.Linear(c_in, output_channels, bias=False))
            fc_layers.append(nn.BatchNorm1d(output_channels, eps=1e-5, momentum=0.01))
            fc_layers.append(nn.ReLU())
        else:
            fc_layers.append(nn.Linear(c_in, output_channels, bias=True))
        return nn.Sequential(*fc_layers)

    def assign_targets(self, input_dict):
        """point_coords (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> point_cls_labels (N) long (the class
        of the first GT box holding the point, 1 when class agnostic; -1 inside the enlarged box only; 0 elsewhere) and
        point_part_labels (N, 3): |(|local / dims| * 2 - 0.5) * 2| snapped to 1 above 0.75, to 0 below 0.25 and
        stretched by * 2 - 0.5 between, zero for a point outside every box."""
        point_coords = input_dict['point_coords']
        gt_boxes = input_dict['gt_boxes']
        assert gt_boxes.shape.__len__() == 3, 'gt_boxes.shape=%s' % str(gt_boxes.shape)
        assert point_coords.shape.__len__() in [2], 'points.shape=%s' % str(point_coords.shape)

        batch_size, num_boxes = gt_boxes.shape[0], gt_boxes.shape[1]
        extend_gt_boxes = box_utils.enlarge_box3d(
            gt_boxes.view(-1, gt_boxes.shape[-1]), extra_width=self.model_cfg.TARGET_CONFIG.GT_EXTRA_WIDTH
        ).view(batch_size, -1, gt_boxes.shape[-1])
        box_idxs_of_pts = roiaware_pool3d_utils.points_in_boxes_stack(
            point_coords, gt_boxes[:, :, 0:7].contiguous()).long()
        extend_box_idxs_of_pts = roiaware_pool3d_utils.points_in_boxes_stack(
            point_coords, extend_gt_boxes[:, :, 0:7].contiguous()).long()
        fg_flag = box_idxs_of_pts >= 0
        ignore_flag = fg_flag ^ (extend_box_idxs_of_pts >= 0)
        labels = torch.where(ignore_flag, -torch.ones_like(box_idxs_of_pts), torch.zeros_like(box_idxs_of_pts))

        # the box of every point (row 0 of its frame for a background point: masked below)
        frame = point_coords[:, 0].long().clamp(0, batch_size - 1)
        rows = frame * num_boxes + box_idxs_of_pts.clamp(min=0)
        gt_box_of_points = gt_boxes.view(-1, gt_boxes.shape[-1])[rows]
        if self.num_class == 1:
            fg_labels = torch.ones_like(box_idxs_of_pts)
        else:
            fg_labels = gt_box_of_points[:, -1].long()
        labels = torch.where(fg_flag, fg_labels, labels)

        shifted = point_coords[:, 1:4] - gt_box_of_points[:, 0:3]
        # common_utils.rotate_points_along_z by -heading
        cosa, sina = torch.cos(-gt_box_of_points[:, 6]), torch.sin(-gt_box_of_points[:, 6])
        local = torch.stack((shifted[:, 0] * cosa - shifted[:, 1] * sina,
                             shifted[:, 0] * sina + shifted[:, 1] * cosa, shifted[:, 2]), dim=1)
        dims = torch.where(fg_flag.unsqueeze(1), gt_box_of_points[:, 3:6], torch.ones_like(shifted))
        temp = torch.abs(((torch.abs(local / dims) * 2) - 0.5) * 2)
        part = torch.where(temp > 0.75, torch.ones_like(temp),
                           torch.where(temp < 0.25, torch.zeros_like(temp), temp * 2 - 0.5))
        part = torch.where(fg_flag.unsqueeze(1), part, torch.zeros_like(part))
        return {'point_cls_labels': labels, 'point_box_labels': None, 'point_part_labels': part}

    def get_part_layer_loss(self, tb_dict=None):
        pos_mask = self.forward_ret_dict['point_cls_labels'] > 0
        point_part_labels = self.forward_ret_dict['point_part_labels']
        point_part_preds = self.forward_ret_dict['point_part_preds']
        pos_normalizer = torch.clamp(pos_mask.sum().to(point_part_preds.dtype), min=1.0)
        point_loss_part = F.binary_cross_entropy(torch.sigmoid(point_part_preds), point_part_labels, reduction='none')
        point_loss_part = (point_loss_part.sum(dim=-1) * pos_mask.to(point_part_preds.dtype)).sum() / (3 * pos_normalizer)

        loss_weights_dict = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        point_loss_part = point_loss_part * loss_weights_dict['point_part_weight']
        if tb_dict is None:
            tb_dict = {}
        tb_dict.update({'point_loss_part': point_loss_part.detach()})
        return point_loss_part, tb_dict

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        point_loss_cls, tb_dict = self.get_cls_layer_loss(tb_dict)
        point_loss_part, tb_dict = self.get_part_layer_loss(tb_dict)
        point_loss = point_loss_cls + point_loss_part
        return point_loss, tb_dict

    def forward(self, batch_dict):
        """point_features (N1 + N2 + ..., C), point_coords (N1 + N2 + ..., 4) -> point_cls_scores (N),
        point_part_offset (N, 3), both sigmoid outputs."""
        point_features = batch_dict['point_features']
        if self.point_feature_layers is not None:
            point_features = self.point_feature_layers(point_features)
        point_cls_preds = self.cls_layers(point_features)  # (total_points, num_class)
        point_part_preds = self.part_reg_layers(point_features)

        ret_dict = {
            'point_cls_preds': point_cls_preds,
            'point_part_preds': point_part_preds,
        }

        point_cls_scores = torch.sigmoid(point_cls_preds)
        point_part_offset = torch.sigmoid(point_part_preds)
        batch_dict['point_cls_scores'], _ = point_cls_scores.max(dim=-1)
        batch_dict['point_part_offset'] = point_part_offset
        multi_scale = batch_dict.get('multi_scale_3d_features', None)
        if multi_scale is not None and self.point_feature_layers is not None:
            for key in ('x_points_mean', 'x_points_max'):
                if key in multi_scale:
                    multi_scale[key] = multi_scale[key].replace_feature(point_features)

        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            ret_dict['point_cls_labels'] = targets_dict['point_cls_labels']
            ret_dict['point_part_labels'] = targets_dict.get('point_part_labels')
            ret_dict['point_box_labels'] = targets_dict.get('point_box_labels')

        self.forward_ret_dict = ret_dict
        return batch_dict
