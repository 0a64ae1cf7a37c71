"""CenterHead and SeparateHead (reference pcdet/models/dense_heads/center_head.py:11-355): a shared 3x3 conv, then per
head a small conv stack per regression target and one for the class heatmap; constructor signature, state_dict keys and
initialisation are the reference's.

What differs, on purpose:
  * assign_targets is ONE call of the HIP op spx.ops.center_assign_targets (csrc/center_targets.hip) for the whole batch
    and every head, with no host read, where the reference loops in Python over heads x frames x boxes, copies every
    frame's boxes to the host, reads radius[k].item() per box and draws each Gaussian in numpy.  GPU tensors only
    (SpxError otherwise), as for the point head.
  * The reference rewrites the class column of gt_boxes IN PLACE while it filters the boxes per head (center_head.py:
    194-195, an assignment through a view).  With one head that writes the value already there; with several heads the
    later heads, and every later module, read labels an earlier head has overwritten.  Here gt_boxes is never written
    and every head sees the original labels.
  * Nothing is moved with .cuda() at construction; the per-head class-id maps, the class-to-head table of the op and the
    code weights are non-persistent buffers (state_dict keys stay the reference's) that follow the module's device.
  * get_loss keeps 0-d tensors in tb_dict instead of .item() floats (the project's convention, anchor_head_template.py)
    and does not overwrite pred_dict['hm'] with its sigmoid; with the device-side branch of neg_loss_cornernet the whole
    of assign_targets + get_loss captures under torch.cuda.graph.
  * forward also takes the fork's `encoded_bev_features` list, as AnchorHeadSingle does.
  * Opt-in (POST_PROCESSING.FUSED: True, or static mode: `static_caps` in the batch dict): the boxes come from
    generate_predicted_boxes_static — spx.ops.center_decode (csrc/center_decode.hip) and spx.ops.point_post_process per
    head, static capacity, no host read — instead of the reference's sigmoid / exp / two topk / six gathers and its
    per-frame mask, NMS and cat.  Without the key the reference's eager composition runs, unchanged.
  * Opt-in (LOSS_CONFIG.FUSED: True): get_loss dispatches to get_loss_fused — spx.ops.center_head_loss
    (csrc/center_loss.hip) per head, losses and gradients in three launches, deterministic.  Without the key the torch
    composition runs, unchanged."""
import copy

import numpy as np
import torch
import torch.nn as nn
from torch.nn.init import kaiming_normal_

from ...utils import loss_utils
from ..model_utils import centernet_utils, model_nms_utils


class SeparateHead(nn.Module):
    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for cur_name in self.sep_head_dict:
            output_channels = self.sep_head_dict[cur_name]['out_channels']
            num_conv = self.sep_head_dict[cur_name]['num_conv']
            fc_list = []
            for _ in range(num_conv - 1):
                fc_list.append(nn.Sequential(
                    nn.Conv2d(input_channels, input_channels, kernel_size=3, stride=1, padding=1, bias=use_bias),
                    nn.BatchNorm2d(input_channels),
                    nn.ReLU()))
            fc_list.append(nn.Conv2d(input_channels, output_channels, kernel_size=3, stride=1, padding=1, bias=True))
            fc = nn.Sequential(*fc_list)
            if 'hm' in cur_name:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        kaiming_normal_(m.weight.data)
                        if m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            self.__setattr__(cur_name, fc)

    def forward(self, x):
        return {cur_name: self.__getattr__(cur_name)(x) for cur_name in self.sep_head_dict}


class CenterHead(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size = grid_size
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        self.feature_map_stride = self.model_cfg.TARGET_ASSIGNER_CONFIG.get('FEATURE_MAP_STRIDE', None)

        self.class_names = class_names
        self.class_names_each_head = []
        table = np.full((len(class_names) + 1, 2), -1, dtype=np.int32)      # global class id -> (head, class in head)
        for idx, cur_class_names in enumerate(self.model_cfg.CLASS_NAMES_EACH_HEAD):
            names = [x for x in cur_class_names if x in class_names]
            self.class_names_each_head.append(names)
            mapping = np.array([self.class_names.index(x) for x in names], dtype=np.int64)
            self.register_buffer('class_id_mapping_head_%d' % idx, torch.from_numpy(mapping), persistent=False)
            for slot, gid in enumerate(mapping.tolist()):
                table[gid + 1] = (idx, slot + 1)
        self.register_buffer('class_to_head_slot', torch.from_numpy(table), persistent=False)

        total_classes = sum([len(x) for x in self.class_names_each_head])
        assert total_classes == len(self.class_names), f'class_names_each_head={self.class_names_each_head}'

        self.shared_conv = nn.Sequential(
            nn.Conv2d(input_channels, self.model_cfg.SHARED_CONV_CHANNEL, 3, stride=1, padding=1,
                      bias=self.model_cfg.get('USE_BIAS_BEFORE_NORM', False)),
            nn.BatchNorm2d(self.model_cfg.SHARED_CONV_CHANNEL),
            nn.ReLU(),
        )

        self.heads_list = nn.ModuleList()
        self.separate_head_cfg = self.model_cfg.SEPARATE_HEAD_CFG
        for cur_class_names in self.class_names_each_head:
            cur_head_dict = copy.deepcopy(self.separate_head_cfg.HEAD_DICT)
            cur_head_dict['hm'] = dict(out_channels=len(cur_class_names), num_conv=self.model_cfg.NUM_HM_CONV)
            self.heads_list.append(SeparateHead(
                input_channels=self.model_cfg.SHARED_CONV_CHANNEL, sep_head_dict=cur_head_dict, init_bias=-2.19,
                use_bias=self.model_cfg.get('USE_BIAS_BEFORE_NORM', False)))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        self.build_losses()

    @property
    def class_id_mapping_each_head(self):
        return [getattr(self, 'class_id_mapping_head_%d' % i) for i in range(len(self.class_names_each_head))]

    def build_losses(self):
        self.add_module('hm_loss_func', loss_utils.FocalLossCenterNet())
        self.add_module('reg_loss_func', loss_utils.RegLossCenterNet())
        weights = self.model_cfg.get('LOSS_CONFIG', None)
        if weights is not None:
            self.register_buffer('code_weights', torch.tensor(list(weights.LOSS_WEIGHTS['code_weights']),
                                                              dtype=torch.float32), persistent=False)

    def assign_targets(self, gt_boxes, feature_map_size=None, **kwargs):
        """gt_boxes (B, M, C >= 8) on the GPU, the class in the last column; feature_map_size (H, W) -> dict of per-head
        lists: heatmaps (B, C_h, H, W), target_boxes (B, NUM_MAX_OBJS, C), inds and masks (B, NUM_MAX_OBJS) int64, and an
        empty heatmap_masks.  One HIP op call, no host read; gt_boxes is not written (see the module docstring)."""
        from spx import ops
        cfg = self.model_cfg.TARGET_ASSIGNER_CONFIG
        feature_map_size = feature_map_size[::-1]       # [H, W] ==> [x, y]
        ret = ops.center_assign_targets(
            gt_boxes, self.class_to_head_slot, [len(x) for x in self.class_names_each_head], self.point_cloud_range,
            self.voxel_size, cfg.FEATURE_MAP_STRIDE, feature_map_size, num_max_objs=cfg.NUM_MAX_OBJS,
            gaussian_overlap=cfg.GAUSSIAN_OVERLAP, min_radius=cfg.MIN_RADIUS)
        ret['heatmap_masks'] = []
        return ret

    def sigmoid(self, x):
        return torch.clamp(x.sigmoid(), min=1e-4, max=1 - 1e-4)

    def get_loss(self):
        if self.model_cfg.LOSS_CONFIG.get('FUSED', False):      # opt-in: spx.ops.center_head_loss per head
            return self.get_loss_fused()
        pred_dicts = self.forward_ret_dict['pred_dicts']
        target_dicts = self.forward_ret_dict['target_dicts']
        weights = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        tb_dict = {}
        loss = 0
        for idx, pred_dict in enumerate(pred_dicts):
            hm_loss = self.hm_loss_func(self.sigmoid(pred_dict['hm']), target_dicts['heatmaps'][idx])
            hm_loss = hm_loss * weights['cls_weight']

            target_boxes = target_dicts['target_boxes'][idx]
            pred_boxes = torch.cat([pred_dict[head_name] for head_name in self.separate_head_cfg.HEAD_ORDER], dim=1)
            reg_loss = self.reg_loss_func(pred_boxes, target_dicts['masks'][idx], target_dicts['inds'][idx], target_boxes)
            loc_loss = (reg_loss * self.code_weights.to(reg_loss.dtype)).sum()
            loc_loss = loc_loss * weights['loc_weight']

            loss = loss + hm_loss + loc_loss
            tb_dict['hm_loss_head_%d' % idx] = hm_loss.detach()
            tb_dict['loc_loss_head_%d' % idx] = loc_loss.detach()
        tb_dict['rpn_loss'] = loss.detach()
        return loss, tb_dict

    def get_loss_fused(self):
        """get_loss with each head's two losses and their gradients from spx.ops.center_head_loss (csrc/center_loss.hip):
        three launches per head forward, one multiplication per head output backward, no host read, no float atomics, so
        the gradients are bitwise reproducible also where two boxes share a cell.  Same return value as get_loss: (loss,
        tb_dict) with the same keys and 0-d tensors.  The regression maps are passed one by one in HEAD_ORDER, not
        concatenated.  A slot with mask 0 is never read (see the op's docstring)."""
        pred_dicts = self.forward_ret_dict['pred_dicts']
        target_dicts = self.forward_ret_dict['target_dicts']
        weights = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        if len(target_dicts.get('heatmap_masks', [])) > 0:
            raise NotImplementedError('get_loss_fused: a focal mask (heatmap_masks) is not supported; '
                                      'set LOSS_CONFIG.FUSED False')
        order = list(self.separate_head_cfg.HEAD_ORDER)
        code_weights = [float(v) for v in weights['code_weights']]
        num_cols = sum(int(self.separate_head_cfg.HEAD_DICT[name]['out_channels']) for name in order)
        if num_cols not in (8, 10) or len(code_weights) != num_cols:
            raise NotImplementedError('get_loss_fused: HEAD_ORDER %s has %d regression columns and %d code_weights '
                                      '(8, or 10 with vel, only)' % (order, num_cols, len(code_weights)))
        tb_dict = {}
        loss = 0
        for idx, pred_dict in enumerate(pred_dicts):
            hm_loss, loc_loss = loss_utils._FusedCenterHeadLoss.apply(
                target_dicts['heatmaps'][idx], target_dicts['target_boxes'][idx], target_dicts['inds'][idx],
                target_dicts['masks'][idx], code_weights, float(weights['cls_weight']), float(weights['loc_weight']),
                pred_dict['hm'], *[pred_dict[name] for name in order])
            loss = loss + hm_loss + loc_loss
            tb_dict['hm_loss_head_%d' % idx] = hm_loss.detach()
            tb_dict['loc_loss_head_%d' % idx] = loc_loss.detach()
        tb_dict['rpn_loss'] = loss.detach()
        return loss, tb_dict

    _FUSED_NMS_TYPES = {'nms_gpu': False, 'nms_normal_gpu': True}       # NMS_TYPE -> axis-aligned pair test

    def generate_predicted_boxes_static(self, batch_size, pred_dicts):
        """The boxes of the whole batch at static capacity with no host read (usable under torch.cuda.graph): per head
        spx.ops.center_decode (top-K over the logits, gathers and decode in one op) and spx.ops.point_post_process
        (class-agnostic NMS with NMS_PRE_MAXSIZE / NMS_POST_MAXSIZE), then each frame's survivors packed head after head.
        Returns pred_boxes (B, cap, 7 | 9), pred_scores (B, cap), pred_labels (B, cap) int64 (1-based), count (B) int32,
        zeros past count; cap = the heads' min(MAX_OBJ_PER_SAMPLE, NMS_POST_MAXSIZE) added up.  The K candidates are
        the K largest LOGITS with equal values in flat-index order: the eager path's topk over the sigmoids agrees
        wherever those are distinct and leaves the order among equal ones unspecified."""
        from spx import ops
        cfg = self.model_cfg.POST_PROCESSING
        nms = cfg.NMS_CONFIG
        if nms.NMS_TYPE == 'circle_nms':
            raise NotImplementedError('circle_nms is not implemented (the reference asserts it away as not checked); '
                                      'use NMS_TYPE nms_gpu')
        if nms.NMS_TYPE not in self._FUSED_NMS_TYPES:
            raise NotImplementedError('generate_predicted_boxes_static: NMS_TYPE %s (nms_gpu and nms_normal_gpu only)'
                                      % nms.NMS_TYPE)
        with_vel = 'vel' in self.separate_head_cfg.HEAD_ORDER
        parts = []
        for idx, pred_dict in enumerate(pred_dicts):
            dec = ops.center_decode(pred_dict['hm'], pred_dict['center'], pred_dict['center_z'], pred_dict['dim'],
                                    pred_dict['rot'], pred_dict['vel'] if with_vel else None, cfg.MAX_OBJ_PER_SAMPLE,
                                    self.feature_map_stride, self.voxel_size, self.point_cloud_range,
                                    cfg.POST_CENTER_LIMIT_RANGE, cfg.SCORE_THRESH, raw=True)
            boxes = dec['boxes'].flatten(0, 1)
            scores = dec['scores'].masked_fill(dec['keep'] == 0, -1.0)      # dropped rows: below the threshold of 0
            labels = self.class_id_mapping_each_head[idx][dec['labels'].long()] + 1
            res = ops.point_post_process(scores.flatten(), labels.flatten(), boxes, batch_size, [0.0], nms.NMS_THRESH,
                                         nms.NMS_PRE_MAXSIZE, nms.NMS_POST_MAXSIZE,
                                         axis_aligned=self._FUSED_NMS_TYPES[nms.NMS_TYPE], per_class=False)
            out_boxes = res['boxes']
            if with_vel:
                live = (res['sel'] >= 0).unsqueeze(-1).to(boxes.dtype)
                out_boxes = torch.cat([out_boxes, boxes[res['sel'].clamp_min(0)][..., 7:9] * live], dim=-1)
            parts.append((out_boxes, res['scores'], res['labels'], res['count']))
        if len(parts) == 1:
            boxes, scores, labels, count = parts[0]
        else:       # a stable partition: every frame's live rows first, head after head
            boxes, scores, labels = (torch.cat([p[i] for p in parts], dim=1) for i in range(3))
            live = torch.cat([torch.arange(p[1].shape[1], device=p[3].device).unsqueeze(0) < p[3].unsqueeze(1)
                              for p in parts], dim=1)
            order = torch.argsort((~live).to(torch.uint8), dim=1, stable=True)
            boxes = boxes.gather(1, order.unsqueeze(-1).expand(-1, -1, boxes.shape[-1]))
            scores, labels = scores.gather(1, order), labels.gather(1, order)
            count = torch.stack([p[3] for p in parts]).sum(0).to(torch.int32)
        return {'pred_boxes': boxes, 'pred_scores': scores, 'pred_labels': labels, 'count': count}

    @staticmethod
    def _slice_static(static):
        """The list of per-frame dicts from the static outputs: ONE host read (the counts)."""
        counts = static['count'].tolist()
        return [{'pred_boxes': static['pred_boxes'][i, :n], 'pred_scores': static['pred_scores'][i, :n],
                 'pred_labels': static['pred_labels'][i, :n]} for i, n in enumerate(counts)]

    def generate_predicted_boxes(self, batch_size, pred_dicts):
        post_process_cfg = self.model_cfg.POST_PROCESSING
        if post_process_cfg.get('FUSED', False):     # opt-in: the fused decode + NMS, one host read for the batch
            return self._slice_static(self.generate_predicted_boxes_static(batch_size, pred_dicts))
        device = pred_dicts[0]['hm'].device
        post_center_limit_range = torch.tensor(post_process_cfg.POST_CENTER_LIMIT_RANGE, dtype=torch.float32,
                                               device=device)
        ret_dict = [{'pred_boxes': [], 'pred_scores': [], 'pred_labels': []} for _ in range(batch_size)]
        for idx, pred_dict in enumerate(pred_dicts):
            batch_hm = pred_dict['hm'].sigmoid()
            batch_center = pred_dict['center']
            batch_center_z = pred_dict['center_z']
            batch_dim = pred_dict['dim'].exp()
            batch_rot_cos = pred_dict['rot'][:, 0].unsqueeze(dim=1)
            batch_rot_sin = pred_dict['rot'][:, 1].unsqueeze(dim=1)
            batch_vel = pred_dict['vel'] if 'vel' in self.separate_head_cfg.HEAD_ORDER else None

            final_pred_dicts = centernet_utils.decode_bbox_from_heatmap(
                heatmap=batch_hm, rot_cos=batch_rot_cos, rot_sin=batch_rot_sin, center=batch_center,
                center_z=batch_center_z, dim=batch_dim, vel=batch_vel, point_cloud_range=self.point_cloud_range,
                voxel_size=self.voxel_size, feature_map_stride=self.feature_map_stride,
                K=post_process_cfg.MAX_OBJ_PER_SAMPLE,
                circle_nms=(post_process_cfg.NMS_CONFIG.NMS_TYPE == 'circle_nms'),
                score_thresh=post_process_cfg.SCORE_THRESH, post_center_limit_range=post_center_limit_range)

            for k, final_dict in enumerate(final_pred_dicts):
                final_dict['pred_labels'] = self.class_id_mapping_each_head[idx][final_dict['pred_labels'].long()]
                selected, selected_scores = model_nms_utils.class_agnostic_nms(
                    box_scores=final_dict['pred_scores'], box_preds=final_dict['pred_boxes'],
                    nms_config=post_process_cfg.NMS_CONFIG, score_thresh=None)
                final_dict['pred_boxes'] = final_dict['pred_boxes'][selected]
                final_dict['pred_scores'] = selected_scores
                final_dict['pred_labels'] = final_dict['pred_labels'][selected]

                ret_dict[k]['pred_boxes'].append(final_dict['pred_boxes'])
                ret_dict[k]['pred_scores'].append(final_dict['pred_scores'])
                ret_dict[k]['pred_labels'].append(final_dict['pred_labels'])

        for k in range(batch_size):
            ret_dict[k]['pred_boxes'] = torch.cat(ret_dict[k]['pred_boxes'], dim=0)
            ret_dict[k]['pred_scores'] = torch.cat(ret_dict[k]['pred_scores'], dim=0)
            ret_dict[k]['pred_labels'] = torch.cat(ret_dict[k]['pred_labels'], dim=0) + 1
        return ret_dict

    @staticmethod
    def reorder_rois_for_refining(batch_size, pred_dicts):
        num_max_rois = max([len(cur_dict['pred_boxes']) for cur_dict in pred_dicts])
        num_max_rois = max(1, num_max_rois)     # at least one faked roi
        pred_boxes = pred_dicts[0]['pred_boxes']

        rois = pred_boxes.new_zeros((batch_size, num_max_rois, pred_boxes.shape[-1]))
        roi_scores = pred_boxes.new_zeros((batch_size, num_max_rois))
        roi_labels = pred_boxes.new_zeros((batch_size, num_max_rois)).long()
        for bs_idx in range(batch_size):
            num_boxes = len(pred_dicts[bs_idx]['pred_boxes'])
            rois[bs_idx, :num_boxes, :] = pred_dicts[bs_idx]['pred_boxes']
            roi_scores[bs_idx, :num_boxes] = pred_dicts[bs_idx]['pred_scores']
            roi_labels[bs_idx, :num_boxes] = pred_dicts[bs_idx]['pred_labels']
        return rois, roi_scores, roi_labels

    def forward(self, data_dict):
        if data_dict.get('encoded_bev_features', None) is not None:
            feats = data_dict['encoded_bev_features']
            spatial_features_2d = feats[0] if len(feats) == 1 else torch.cat(feats, dim=1)
        else:
            spatial_features_2d = data_dict['spatial_features_2d']
        x = self.shared_conv(spatial_features_2d.float())

        pred_dicts = [head(x) for head in self.heads_list]

        if self.training:
            self.forward_ret_dict['target_dicts'] = self.assign_targets(
                data_dict['gt_boxes'], feature_map_size=spatial_features_2d.size()[2:],
                feature_map_stride=data_dict.get('spatial_features_2d_strides', None))
        self.forward_ret_dict['pred_dicts'] = pred_dicts

        static = not self.training and data_dict.get('static_caps', None) is not None
        fused = static or bool(self.model_cfg.POST_PROCESSING.get('FUSED', False))
        if fused and (not self.training or self.predict_boxes_when_training):
            final = self.generate_predicted_boxes_static(data_dict['batch_size'], pred_dicts)
            if static:
                data_dict['final_box_static'] = final
            if self.predict_boxes_when_training:        # already zero-padded to one shape: no reorder_rois_for_refining
                data_dict['rois'] = final['pred_boxes']
                data_dict['roi_scores'] = final['pred_scores']
                data_dict['roi_labels'] = final['pred_labels']
                data_dict['has_class_labels'] = True
            elif not static:
                data_dict['final_box_dicts'] = self._slice_static(final)
        elif not self.training or self.predict_boxes_when_training:
            pred_dicts = self.generate_predicted_boxes(data_dict['batch_size'], pred_dicts)
            if self.predict_boxes_when_training:
                rois, roi_scores, roi_labels = self.reorder_rois_for_refining(data_dict['batch_size'], pred_dicts)
                data_dict['rois'] = rois
                data_dict['roi_scores'] = roi_scores
                data_dict['roi_labels'] = roi_labels
                data_dict['has_class_labels'] = True
            else:
                data_dict['final_box_dicts'] = pred_dicts
        return data_dict
