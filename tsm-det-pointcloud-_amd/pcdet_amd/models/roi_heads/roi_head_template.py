"""RoIHeadTemplate (reference pcdet/models/roi_heads/roi_head_template.py:11-278): what every second-stage head shares --
the proposal layer, target assignment with the canonical transform, the box / class losses and the box decoding.

Differences from the reference, all so that a training step needs no host read and captures under torch.cuda.graph:
  * proposal_layer takes one batched torch.topk, one spx.ops.nms_bev per frame and a masked gather of the first
    NMS_POST_MAXSIZE kept positions against the device-side count; the reference reads the kept count back per frame.
    With NMS_CONFIG.FUSED: True one spx.ops.dense_post_process call replaces the topk and the per-frame loop.
  * proposal scores: the fork multiplies sigmoid(max class logit) by sigmoid(batch_dict['candidate_score']), a key only
    its own neck writes.  That score is used when the key is present; without it the score is upstream OpenPCDet's raw
    maximum class logit.
  * the losses keep fg_sum and every tb_dict entry on the device (0-dim tensors); the corner loss runs over all rows with
    the non-fg rows masked instead of over a boolean-indexed subset.
MULTI_CLASSES_NMS and a list-valued NMS_POST_MAXSIZE (the fork's class_agnostic_nms_v2) are refused by name."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...utils import box_coder_utils, common_utils, loss_utils
from .target_assigner.proposal_target_layer import ProposalTargetLayer

_AXIS_ALIGNED = {'nms_gpu': False, 'nms_normal_gpu': True}


class RoIHeadTemplate(nn.Module):
    def __init__(self, num_class, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.box_coder = getattr(box_coder_utils, self.model_cfg.TARGET_CONFIG.BOX_CODER)(
            **self.model_cfg.TARGET_CONFIG.get('BOX_CODER_CONFIG', {}))
        self.proposal_target_layer = ProposalTargetLayer(roi_sampler_cfg=self.model_cfg.TARGET_CONFIG)
        self.build_losses(self.model_cfg.LOSS_CONFIG)
        self.forward_ret_dict = None

    def build_losses(self, losses_cfg):
        self.add_module('reg_loss_func',
                        loss_utils.WeightedSmoothL1Loss(code_weights=losses_cfg.LOSS_WEIGHTS['code_weights']))

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        fc_layers = []
        pre_channel = input_channels
        for k in range(0, fc_list.__len__()):
            fc_layers.extend([nn.Conv1d(pre_channel, fc_list[k], kernel_size=1, bias=False), nn.BatchNorm1d(fc_list[k]),
                              nn.ReLU()])
            pre_channel = fc_list[k]
            if self.model_cfg.DP_RATIO >= 0 and k == 0:
                fc_layers.append(nn.Dropout(self.model_cfg.DP_RATIO))
        fc_layers.append(nn.Conv1d(pre_channel, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*fc_layers)

    @torch.no_grad()
    def proposal_layer(self, batch_dict, nms_config):
        """batch_cls_preds (B, N, classes | 1), batch_box_preds (B, N, 7 + C) (or flat with batch_index, equal frames) ->
        rois (B, P, 7 + C), roi_scores (B, P), roi_labels (B, P) in 1 .. classes, P = NMS_POST_MAXSIZE; rows past a
        frame's kept count are zero boxes with score 0 and label 1, as in the reference."""
        if batch_dict.get('rois', None) is not None:
            return batch_dict
        from spx import ops
        if nms_config.MULTI_CLASSES_NMS:
            raise NotImplementedError('MULTI_CLASSES_NMS is not supported by the proposal layer')
        if not isinstance(nms_config.NMS_POST_MAXSIZE, int):
            raise NotImplementedError('a list-valued NMS_POST_MAXSIZE (class_agnostic_nms_v2) is not supported')
        if nms_config.NMS_TYPE not in _AXIS_ALIGNED:
            raise NotImplementedError('NMS_TYPE %s' % nms_config.NMS_TYPE)
        batch_size = batch_dict['batch_size']
        box_preds, cls_preds = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        candidate = batch_dict.get('candidate_score', None)
        if batch_dict.get('batch_index', None) is not None:      # a point head's flat rows: frames of equal length
            assert cls_preds.dim() == 2 and box_preds.shape[0] % batch_size == 0
            box_preds = box_preds.view(batch_size, -1, box_preds.shape[-1])
            cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        assert cls_preds.dim() == 3
        n, post = box_preds.shape[1], int(nms_config.NMS_POST_MAXSIZE)
        scores, labels = torch.max(cls_preds, dim=2)
        if candidate is not None:
            scores = torch.sigmoid(scores) * torch.sigmoid(candidate.reshape(batch_size, n))
        k = min(int(nms_config.NMS_PRE_MAXSIZE), n)
        if nms_config.get('FUSED', False) and batch_size * n > 0:
            return self._proposal_layer_fused(batch_dict, nms_config, box_preds, scores, labels, k, post,
                                              cls_preds.shape[-1] > 1)
        top_scores, order = torch.topk(scores, k=k, dim=1)
        top_boxes = torch.gather(box_preds, 1, order.unsqueeze(-1).expand(-1, -1, box_preds.shape[-1]))
        top_labels = torch.gather(labels, 1, order)
        keep, count = [], []
        for index in range(batch_size):
            kept, cnt = ops.nms_bev(top_boxes[index, :, 0:7], nms_config.NMS_THRESH,
                                    axis_aligned=_AXIS_ALIGNED[nms_config.NMS_TYPE])
            keep.append(F.pad(kept[:post], (0, max(post - kept.shape[0], 0))))
            count.append(cnt)
        keep, count = torch.stack(keep), torch.stack(count)                      # (B, P), (B, 1)
        valid = torch.arange(post, device=keep.device).view(1, -1) < count
        keep = torch.where(valid, keep, torch.zeros_like(keep))                  # positions past the count are undefined
        rois = torch.gather(top_boxes, 1, keep.unsqueeze(-1).expand(-1, -1, box_preds.shape[-1])) * valid.unsqueeze(-1)
        roi_scores = torch.gather(top_scores, 1, keep) * valid
        roi_labels = torch.gather(top_labels, 1, keep) * valid
        batch_dict['rois'] = rois
        batch_dict['roi_scores'] = roi_scores
        batch_dict['roi_labels'] = roi_labels + 1
        batch_dict['has_class_labels'] = True if cls_preds.shape[-1] > 1 else False
        batch_dict.pop('batch_index', None)
        return batch_dict

    def _proposal_layer_fused(self, batch_dict, nms_config, box_preds, scores, labels, pre, post, has_class_labels):
        """NMS_CONFIG.FUSED: the selection, the NMS and the cut of every frame in one spx.ops.dense_post_process call
        (class agnostic, no threshold), then the gathers.  Same outputs as the loop above for scores without NaN (the op
        never selects a NaN, torch.topk ranks it first) and without ties at the cut (torch.topk's order of equal scores is
        unspecified; the op takes the lower row)."""
        from spx import ops
        batch_size, n = scores.shape
        flat_boxes = box_preds.reshape(batch_size * n, box_preds.shape[-1])
        flat_scores, flat_labels = scores.reshape(-1), labels.reshape(-1)
        res = ops.dense_post_process(flat_scores, flat_labels + 1, flat_boxes, batch_size, None, nms_config.NMS_THRESH,
                                     pre, post, axis_aligned=_AXIS_ALIGNED[nms_config.NMS_TYPE], per_class=False)
        sel = F.pad(res['sel'], (0, post - res['sel'].shape[1]), value=-1)         # (B, P); K = min(n, P) columns come back
        valid = sel >= 0
        # positions past the count read the frame's best row, as the loop's keep = 0 does, and are zeroed the same way
        # (a frame that selected nothing, all scores NaN, reads its own first row)
        first = torch.arange(batch_size, device=sel.device, dtype=sel.dtype).view(-1, 1) * n
        sel = torch.where(valid, sel, torch.where(valid[:, :1], sel[:, :1], first))
        batch_dict['rois'] = flat_boxes[sel] * valid.unsqueeze(-1)
        batch_dict['roi_scores'] = flat_scores[sel] * valid
        batch_dict['roi_labels'] = flat_labels[sel] * valid + 1
        batch_dict['has_class_labels'] = has_class_labels
        batch_dict.pop('batch_index', None)
        return batch_dict

    def assign_targets(self, batch_dict):
        batch_size = batch_dict['batch_size']
        with torch.no_grad():
            targets_dict = self.proposal_target_layer.forward(batch_dict)
        rois = targets_dict['rois']                    # (B, M, 7 + C)
        gt_of_rois = targets_dict['gt_of_rois']        # (B, M, 7 + C + 1)
        targets_dict['gt_of_rois_src'] = gt_of_rois.clone().detach()

        # canonical transformation
        roi_center = rois[:, :, 0:3]
        roi_ry = rois[:, :, 6] % (2 * np.pi)
        gt_of_rois = torch.cat([gt_of_rois[:, :, 0:3] - roi_center, gt_of_rois[:, :, 3:6],
                                (gt_of_rois[:, :, 6] - roi_ry).unsqueeze(-1), gt_of_rois[:, :, 7:]], dim=-1)
        # LiDAR coordinates -> the RoI's local coordinates
        gt_of_rois = common_utils.rotate_points_along_z(
            points=gt_of_rois.view(-1, 1, gt_of_rois.shape[-1]), angle=-roi_ry.view(-1)
        ).view(batch_size, -1, gt_of_rois.shape[-1])
        # flip the orientation where the RoI points the opposite way
        heading_label = gt_of_rois[:, :, 6] % (2 * np.pi)                                          # 0 .. 2 pi
        opposite_flag = (heading_label > np.pi * 0.5) & (heading_label < np.pi * 1.5)
        heading_label = torch.where(opposite_flag, (heading_label + np.pi) % (2 * np.pi), heading_label)
        heading_label = torch.where(heading_label > np.pi, heading_label - np.pi * 2, heading_label)  # (-pi / 2, pi / 2)
        heading_label = torch.clamp(heading_label, min=-np.pi / 2, max=np.pi / 2)
        gt_of_rois = torch.cat([gt_of_rois[:, :, :6], heading_label.unsqueeze(-1), gt_of_rois[:, :, 7:]], dim=-1)
        targets_dict['gt_of_rois'] = gt_of_rois
        return targets_dict

    def get_box_reg_layer_loss(self, forward_ret_dict):
        loss_cfgs = self.model_cfg.LOSS_CONFIG
        code_size = self.box_coder.code_size
        reg_valid_mask = forward_ret_dict['reg_valid_mask'].view(-1)
        gt_boxes3d_ct = forward_ret_dict['gt_of_rois'][..., 0:code_size]
        gt_of_rois_src = forward_ret_dict['gt_of_rois_src'][..., 0:code_size].view(-1, code_size)
        rcnn_reg = forward_ret_dict['rcnn_reg']        # (rcnn_batch_size, C)
        roi_boxes3d = forward_ret_dict['rois']
        rcnn_batch_size = gt_boxes3d_ct.view(-1, code_size).shape[0]
        fg_mask = (reg_valid_mask > 0)
        fg_sum = fg_mask.sum().to(rcnn_reg.dtype)      # stays on the device
        tb_dict = {}
        if loss_cfgs.REG_LOSS != 'smooth-l1':
            raise NotImplementedError('REG_LOSS %s' % loss_cfgs.REG_LOSS)
        rois_anchor = roi_boxes3d.clone().detach().view(-1, code_size)
        rois_anchor[:, 0:3] = 0
        rois_anchor[:, 6] = 0
        reg_targets = self.box_coder.encode_torch(gt_boxes3d_ct.view(rcnn_batch_size, code_size), rois_anchor)
        rcnn_loss_reg = self.reg_loss_func(rcnn_reg.view(rcnn_batch_size, -1).unsqueeze(dim=0), reg_targets.unsqueeze(dim=0))
        rcnn_loss_reg = (rcnn_loss_reg.view(rcnn_batch_size, -1) * fg_mask.unsqueeze(dim=-1).to(rcnn_reg.dtype)).sum() \
            / torch.clamp(fg_sum, min=1.0)
        rcnn_loss_reg = rcnn_loss_reg * loss_cfgs.LOSS_WEIGHTS['rcnn_reg_weight']
        tb_dict['rcnn_loss_reg'] = rcnn_loss_reg.detach()
        if loss_cfgs.CORNER_LOSS_REGULARIZATION:
            # every row, the non-fg rows with a zero regression so that nothing in them overflows; masked in the mean
            fg_rcnn_reg = torch.where(fg_mask.unsqueeze(-1), rcnn_reg.view(rcnn_batch_size, -1),
                                      torch.zeros_like(rcnn_reg.view(rcnn_batch_size, -1)))
            fg_roi_boxes3d = roi_boxes3d.detach().view(1, -1, code_size)
            batch_anchors = fg_roi_boxes3d.clone()
            roi_ry = fg_roi_boxes3d[:, :, 6].view(-1)
            roi_xyz = fg_roi_boxes3d[:, :, 0:3].view(-1, 3)
            batch_anchors[:, :, 0:3] = 0
            rcnn_boxes3d = self.box_coder.decode_torch(fg_rcnn_reg.view(1, -1, code_size), batch_anchors).view(-1, code_size)
            rcnn_boxes3d = common_utils.rotate_points_along_z(rcnn_boxes3d.unsqueeze(dim=1), roi_ry).squeeze(dim=1)
            rcnn_boxes3d = torch.cat([rcnn_boxes3d[:, 0:3] + roi_xyz, rcnn_boxes3d[:, 3:]], dim=1)
            loss_corner = loss_utils.get_corner_loss_lidar(rcnn_boxes3d[:, 0:7], gt_of_rois_src[:, 0:7])
            loss_corner = torch.where(fg_mask, loss_corner, torch.zeros_like(loss_corner)).sum() / torch.clamp(fg_sum, min=1.0)
            loss_corner = loss_corner * loss_cfgs.LOSS_WEIGHTS['rcnn_corner_weight']
            rcnn_loss_reg = rcnn_loss_reg + loss_corner
            tb_dict['rcnn_loss_corner'] = loss_corner.detach()
        return rcnn_loss_reg, tb_dict

    def get_box_cls_layer_loss(self, forward_ret_dict):
        loss_cfgs = self.model_cfg.LOSS_CONFIG
        rcnn_cls = forward_ret_dict['rcnn_cls']
        rcnn_cls_labels = forward_ret_dict['rcnn_cls_labels'].view(-1)
        if loss_cfgs.CLS_LOSS == 'BinaryCrossEntropy':
            rcnn_cls_flat = rcnn_cls.view(-1)
            batch_loss_cls = F.binary_cross_entropy(torch.sigmoid(rcnn_cls_flat), rcnn_cls_labels.to(rcnn_cls.dtype),
                                                    reduction='none')
        elif loss_cfgs.CLS_LOSS == 'CrossEntropy':
            batch_loss_cls = F.cross_entropy(rcnn_cls, rcnn_cls_labels, reduction='none', ignore_index=-1)
        else:
            raise NotImplementedError('CLS_LOSS %s' % loss_cfgs.CLS_LOSS)
        cls_valid_mask = (rcnn_cls_labels >= 0).to(batch_loss_cls.dtype)
        rcnn_loss_cls = (batch_loss_cls * cls_valid_mask).sum() / torch.clamp(cls_valid_mask.sum(), min=1.0)
        rcnn_loss_cls = rcnn_loss_cls * loss_cfgs.LOSS_WEIGHTS['rcnn_cls_weight']
        return rcnn_loss_cls, {'rcnn_loss_cls': rcnn_loss_cls.detach()}

    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        rcnn_loss_cls, cls_tb_dict = self.get_box_cls_layer_loss(self.forward_ret_dict)
        tb_dict.update(cls_tb_dict)
        rcnn_loss_reg, reg_tb_dict = self.get_box_reg_layer_loss(self.forward_ret_dict)
        tb_dict.update(reg_tb_dict)
        rcnn_loss = rcnn_loss_cls + rcnn_loss_reg
        tb_dict['rcnn_loss'] = rcnn_loss.detach()
        return rcnn_loss, tb_dict

    def generate_predicted_boxes(self, batch_size, rois, cls_preds, box_preds):
        """rois (B, N, 7), cls_preds (BN, num_class), box_preds (BN, code_size) -> (B, N, num_class), (B, N, code_size)."""
        code_size = self.box_coder.code_size
        batch_cls_preds = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        batch_box_preds = box_preds.view(batch_size, -1, code_size)
        roi_ry = rois[:, :, 6].view(-1)
        roi_xyz = rois[:, :, 0:3].view(-1, 3)
        local_rois = rois.clone().detach()
        local_rois[:, :, 0:3] = 0
        batch_box_preds = self.box_coder.decode_torch(batch_box_preds, local_rois).view(-1, code_size)
        batch_box_preds = common_utils.rotate_points_along_z(batch_box_preds.unsqueeze(dim=1), roi_ry).squeeze(dim=1)
        batch_box_preds = torch.cat([batch_box_preds[:, 0:3] + roi_xyz, batch_box_preds[:, 3:]], dim=1)
        return batch_cls_preds, batch_box_preds.view(batch_size, -1, code_size)
