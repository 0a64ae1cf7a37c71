"""Detector3DTemplate — module assembly, checkpoint IO and post-processing with the reference's API
(pcdet/models/detectors/detector3d_template.py:17-205 build_*, :207-349 post_processing, :544-625 checkpoints).

Differences forced by the fork's drift, all backwards compatible:
  * build_backbone_2d keeps `num_bev_features` from the module's own attribute (falls back to the fork's
    num_voxel_neck_features) and never overwrites num_point_features with None;
  * POST_PROCESSING.SCORE_THRESH may be a scalar (upstream) or a per-class list (fork's multi_thresh).
The module slots of the SECOND, SECOND-IoU, Voxel R-CNN, PV-RCNN (pfe: VoxelSetAbstraction, point_head, roi_head) and
3DSSD paths are populated; `neck` stays None.  A RoI head that reads keypoint features (PVRCNNHead) is refused by name
when the model has built no PFE.
"""
import os

import torch
import torch.nn as nn

from ...utils.spconv_utils import find_all_spconv_keys
from .. import backbones_2d, backbones_3d, dense_heads, roi_heads
from ..backbones_2d import map_to_bev
from ..backbones_3d import pfe, vfe
from ..model_utils import model_nms_utils


class Detector3DTemplate(nn.Module):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.dataset = dataset
        self.class_names = dataset.class_names
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        self.module_topology = ['vfe', 'backbone_3d', 'map_to_bev_module', 'pfe', 'backbone_2d', 'neck', 'dense_head',
                                'point_head', 'roi_head']

    @property
    def mode(self):
        return 'TRAIN' if self.training else 'TEST'

    def update_global_step(self):
        self.global_step += 1

    def build_networks(self):
        info = {
            'module_list': [],
            'num_rawpoint_features': self.dataset.point_feature_encoder.num_point_features,
            'num_point_features': self.dataset.point_feature_encoder.num_point_features,
            'grid_size': self.dataset.grid_size,
            'point_cloud_range': self.dataset.point_cloud_range,
            'voxel_size': self.dataset.voxel_size,
            'depth_downsample_factor': getattr(self.dataset, 'depth_downsample_factor', None),
        }
        for module_name in self.module_topology:
            module, info = getattr(self, 'build_%s' % module_name)(model_info_dict=info)
            self.add_module(module_name, module)
        return info['module_list']

    def build_vfe(self, model_info_dict):
        if self.model_cfg.get('VFE', None) is None:
            return None, model_info_dict
        m = vfe.__all__[self.model_cfg.VFE.NAME](
            model_cfg=self.model_cfg.VFE, num_point_features=model_info_dict['num_rawpoint_features'],
            point_cloud_range=model_info_dict['point_cloud_range'], voxel_size=model_info_dict['voxel_size'],
            grid_size=model_info_dict['grid_size'], depth_downsample_factor=model_info_dict['depth_downsample_factor'])
        model_info_dict['num_point_features'] = m.get_output_feature_dim()
        model_info_dict['module_list'].append(m)
        return m, model_info_dict

    def build_backbone_3d(self, model_info_dict):
        if self.model_cfg.get('BACKBONE_3D', None) is None:
            return None, model_info_dict
        m = backbones_3d.get_backbone_3d(self.model_cfg.BACKBONE_3D.NAME)(
            model_cfg=self.model_cfg.BACKBONE_3D, input_channels=model_info_dict['num_point_features'],
            grid_size=model_info_dict['grid_size'], voxel_size=model_info_dict['voxel_size'],
            point_cloud_range=model_info_dict['point_cloud_range'])
        model_info_dict['module_list'].append(m)
        model_info_dict['num_point_features'] = m.num_point_features
        model_info_dict['backbone_channels'] = getattr(m, 'backbone_channels', None)
        model_info_dict['num_bev_features'] = getattr(m, 'num_bev_features', None)
        return m, model_info_dict

    def build_map_to_bev_module(self, model_info_dict):
        if self.model_cfg.get('MAP_TO_BEV', None) is None:
            return None, model_info_dict
        m = map_to_bev.__all__[self.model_cfg.MAP_TO_BEV.NAME](model_cfg=self.model_cfg.MAP_TO_BEV,
                                                               grid_size=model_info_dict['grid_size'])
        model_info_dict['module_list'].append(m)
        model_info_dict['num_bev_features'] = m.num_bev_features
        return m, model_info_dict

    def build_backbone_2d(self, model_info_dict):
        if self.model_cfg.get('BACKBONE_2D', None) is None:
            return None, model_info_dict
        m = backbones_2d.__all__[self.model_cfg.BACKBONE_2D.NAME](
            model_cfg=self.model_cfg.BACKBONE_2D, input_channels=model_info_dict['num_bev_features'],
            voxel_size=model_info_dict['voxel_size'], point_cloud_range=model_info_dict['point_cloud_range'],
            backbone_channels=model_info_dict.get('backbone_channels', None))
        model_info_dict['module_list'].append(m)
        nbev = getattr(m, 'num_bev_features', None)
        model_info_dict['num_bev_features'] = nbev if nbev is not None else m.num_voxel_neck_features
        if getattr(m, 'num_point_features', None) is not None:
            model_info_dict['num_point_features'] = m.num_point_features
        return m, model_info_dict

    def build_dense_head(self, model_info_dict):
        if self.model_cfg.get('DENSE_HEAD', None) is None:
            return None, model_info_dict
        m = dense_heads.__all__[self.model_cfg.DENSE_HEAD.NAME](
            model_cfg=self.model_cfg.DENSE_HEAD, input_channels=model_info_dict['num_bev_features'],
            num_class=self.num_class if not self.model_cfg.DENSE_HEAD.CLASS_AGNOSTIC else 1,
            class_names=self.class_names, grid_size=model_info_dict['grid_size'],
            point_cloud_range=model_info_dict['point_cloud_range'],
            predict_boxes_when_training=self.model_cfg.get('ROI_HEAD', False),
            voxel_size=model_info_dict.get('voxel_size', False))
        model_info_dict['module_list'].append(m)
        return m, model_info_dict

    def _absent(self, key, model_info_dict):
        if self.model_cfg.get(key, None) is not None:
            raise NotImplementedError('%s modules are outside the SECOND hot path (SURVEY.md §2)' % key)
        return None, model_info_dict

    def build_pfe(self, model_info_dict):
        if self.model_cfg.get('PFE', None) is None:
            return None, model_info_dict
        name = self.model_cfg.PFE.NAME
        if name not in pfe.__all__:
            raise NotImplementedError('PFE %s is not supported (%s)' % (name, ', '.join(pfe.__all__)))
        m = pfe.__all__[name](
            model_cfg=self.model_cfg.PFE, voxel_size=model_info_dict['voxel_size'],
            point_cloud_range=model_info_dict['point_cloud_range'], num_bev_features=model_info_dict['num_bev_features'],
            num_rawpoint_features=model_info_dict['num_rawpoint_features'])
        model_info_dict['module_list'].append(m)
        model_info_dict['num_point_features'] = m.num_point_features
        model_info_dict['num_point_features_before_fusion'] = m.num_point_features_before_fusion
        return m, model_info_dict

    def build_neck(self, model_info_dict):
        return self._absent('NECK', model_info_dict)

    def build_point_head(self, model_info_dict):
        if self.model_cfg.get('POINT_HEAD', None) is None:
            return None, model_info_dict
        if self.model_cfg.POINT_HEAD.get('USE_POINT_FEATURES_BEFORE_FUSION', False):
            num_point_features = model_info_dict['num_point_features_before_fusion']
        else:
            num_point_features = model_info_dict['num_point_features']
        m = dense_heads.__all__[self.model_cfg.POINT_HEAD.NAME](
            model_cfg=self.model_cfg.POINT_HEAD, input_channels=num_point_features,
            num_class=self.num_class if not self.model_cfg.POINT_HEAD.CLASS_AGNOSTIC else 1,
            predict_boxes_when_training=self.model_cfg.get('ROI_HEAD', False),
            voxel_size=model_info_dict.get('voxel_size', False), point_cloud_range=model_info_dict['point_cloud_range'])
        model_info_dict['module_list'].append(m)
        return m, model_info_dict

    def build_roi_head(self, model_info_dict):
        if self.model_cfg.get('ROI_HEAD', None) is None:
            return None, model_info_dict
        name = self.model_cfg.ROI_HEAD.NAME
        if name not in roi_heads.__all__ or name == 'RoIHeadTemplate':
            raise NotImplementedError('ROI_HEAD %s is not supported (second-stage heads: %s)'
                                      % (name, ', '.join(k for k in roi_heads.__all__ if k != 'RoIHeadTemplate')))
        if name in roi_heads.KEYPOINT_HEADS and getattr(self, 'pfe', None) is None:
            raise NotImplementedError('ROI_HEAD %s pools keypoint features and MODEL.PFE is missing: the model has no '
                                      'point-feature encoder (VoxelSetAbstraction) to read them from' % name)
        m = roi_heads.__all__[name](
            model_cfg=self.model_cfg.ROI_HEAD, input_channels=model_info_dict['num_point_features'],
            backbone_channels=model_info_dict.get('backbone_channels', None),
            point_cloud_range=model_info_dict['point_cloud_range'], voxel_size=model_info_dict['voxel_size'],
            grid_size=model_info_dict['grid_size'],
            num_class=self.num_class if not self.model_cfg.ROI_HEAD.CLASS_AGNOSTIC else 1)
        model_info_dict['module_list'].append(m)
        return m, model_info_dict

    def forward(self, **kwargs):
        raise NotImplementedError

    # ------------------------------------------------------------------ post-processing (reference :207-349)
    _FUSED_NMS_TYPES = {'nms_gpu': False, 'nms_normal_gpu': True}      # NMS_TYPE -> axis aligned
    # Candidates per frame up to which post_processing takes the fused path unless POST_PROCESSING.FUSED says otherwise:
    # measured 3.6x (batch 4) and 15.3x (batch 16) faster than the eager code at 512 (KITTI), 0.8x at 3 072 (Waymo, 4
    # frames, ~1 500 kept boxes each) -- profiles/post_process_bench.log.  Nothing in between was measured.
    FUSED_DEFAULT_MAX_N = 512

    def _dense_post_plan(self, batch_dict):
        """_fused_post_plan for dense (B, N, .) predictions of an anchor head or a second stage (no batch_index), served by
        spx.ops.dense_post_process: any N, NMS_PRE_MAXSIZE up to ops.DENSE_POST_PROCESS_MAX_PRE, at most
        ops.POST_PROCESS_MAX_N kept boxes per frame over the classes."""
        from spx import ops
        cfg = self.model_cfg.POST_PROCESSING
        nms = cfg.NMS_CONFIG
        boxes, cls = batch_dict.get('batch_box_preds', None), batch_dict.get('batch_cls_preds', None)
        batch_size = int(batch_dict['batch_size'])
        if not isinstance(boxes, torch.Tensor) or not isinstance(cls, torch.Tensor) or not boxes.is_cuda:
            return None
        if boxes.dim() != 3 or cls.dim() != 3 or cls.shape[-1] not in (1, self.num_class) or boxes.shape[-1] < 7:
            return None
        if nms.MULTI_CLASSES_NMS or nms.NMS_TYPE not in self._FUSED_NMS_TYPES:
            return None
        n = boxes.shape[1]
        if batch_size < 1 or n == 0 or boxes.shape[0] != batch_size or tuple(cls.shape[:2]) != (batch_size, n):
            return None
        thresh = cfg.SCORE_THRESH
        per_class = isinstance(thresh, (list, tuple))
        thresh = [float(t) for t in thresh] if per_class else [float(thresh)]
        if not isinstance(nms.NMS_PRE_MAXSIZE, int) or not isinstance(nms.NMS_POST_MAXSIZE, int):
            return None
        pre_max, post_max = int(nms.NMS_PRE_MAXSIZE), int(nms.NMS_POST_MAXSIZE)
        if not 1 <= len(thresh) <= 8 or not 1 <= pre_max <= ops.DENSE_POST_PROCESS_MAX_PRE or post_max < 1 \
                or len(thresh) * min(post_max, pre_max, n) > ops.POST_PROCESS_MAX_N:
            return None
        return dict(batch_size=batch_size, n=n, thresholds=thresh, per_class=per_class, nms_thresh=float(nms.NMS_THRESH),
                    pre_max=pre_max, post_max=post_max, axis_aligned=self._FUSED_NMS_TYPES[nms.NMS_TYPE], dense=True)

    def _fused_post_plan(self, batch_dict, dense=None):
        """The settings of the fused post-processing (spx.ops.point_post_process) for this batch, or None where it does
        not apply: flat point-head predictions with batch_index, a row count that divides into batch_size frames of at
        most ops.POST_PROCESS_MAX_N candidates, NMS_TYPE nms_gpu / nms_normal_gpu, no MULTI_CLASSES_NMS.  Host values
        only, no device read; that the frames really are contiguous and equally long is the device flag layout_ok of
        post_processing_static.
        Dense (B, N, .) predictions without batch_index (_dense_post_plan) give a plan only when asked for: dense=True, or
        dense=None and POST_PROCESSING.FUSED is True."""
        from spx import ops
        cfg = self.model_cfg.POST_PROCESSING
        nms = cfg.NMS_CONFIG
        index, boxes, cls = (batch_dict.get(k, None) for k in ('batch_index', 'batch_box_preds', 'batch_cls_preds'))
        if index is None and isinstance(boxes, torch.Tensor) and boxes.dim() == 3:
            want = cfg.get('FUSED', None) is True if dense is None else bool(dense)
            return self._dense_post_plan(batch_dict) if want else None
        batch_size = int(batch_dict['batch_size'])
        if not all(isinstance(t, torch.Tensor) for t in (index, boxes, cls)):
            return None
        if not boxes.is_cuda or boxes.dim() != 2 or cls.dim() != 2:
            return None
        if nms.MULTI_CLASSES_NMS or nms.NMS_TYPE not in self._FUSED_NMS_TYPES or cls.shape[1] not in (1, self.num_class):
            return None
        rows = boxes.shape[0]
        if batch_size < 1 or rows == 0 or rows % batch_size or rows // batch_size > ops.POST_PROCESS_MAX_N \
                or index.numel() != rows or cls.shape[0] != rows or boxes.shape[1] < 7:
            return None
        thresh = cfg.SCORE_THRESH
        per_class = isinstance(thresh, (list, tuple))
        thresh = [float(t) for t in thresh] if per_class else [float(thresh)]
        if not 1 <= len(thresh) <= 8 or int(nms.NMS_PRE_MAXSIZE) < 1 or int(nms.NMS_POST_MAXSIZE) < 1:
            return None
        return dict(batch_size=batch_size, n=rows // batch_size, thresholds=thresh, per_class=per_class,
                    nms_thresh=float(nms.NMS_THRESH), pre_max=int(nms.NMS_PRE_MAXSIZE), post_max=int(nms.NMS_POST_MAXSIZE),
                    axis_aligned=self._FUSED_NMS_TYPES[nms.NMS_TYPE])

    def post_processing_static(self, batch_dict, plan=None):
        """Post-processing of the whole batch with no host read (usable under torch.cuda.graph): K rows per frame,
        K = min(n, num_thresholds * NMS_POST_MAXSIZE) with per-class thresholds, min(n, NMS_POST_MAXSIZE) with one.
          sel (B, K) int64 rows of batch_box_preds or -1, count (B) int32, pred_boxes (B, K, 7), pred_scores (B, K),
          pred_labels (B, K) int64 (zeros past count); layout_ok: 0-dim bool, False when batch_index is not B equal,
          contiguous frames (the results are then meaningless); with gt_boxes and RECALL_THRESH_LIST also recalled
          (B, T) int32 and num_gt (B) int32 (spx.ops.recall_count).
        Dense (B, N, .) predictions (a plan of _dense_post_plan) go through spx.ops.dense_post_process: sel then counts
        rows of the flattened (B * N, .) predictions, the labels are roi_labels / batch_pred_labels when has_class_labels
        is set, and layout_ok is constantly True.
        Raises where the fused path does not apply (_fused_post_plan)."""
        from spx import ops
        plan = plan or self._fused_post_plan(batch_dict)
        if plan is None:
            raise NotImplementedError('post_processing_static needs flat point-head predictions of equal frames of at '
                                      'most %d candidates, or dense (B, N, .) predictions with POST_PROCESSING.FUSED: '
                                      'True, and NMS_TYPE nms_gpu / nms_normal_gpu' % ops.POST_PROCESS_MAX_N)
        cfg = self.model_cfg.POST_PROCESSING
        b, n = plan['batch_size'], plan['n']
        dense = plan.get('dense', False)
        box_preds, src_cls_preds = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        cls_preds = src_cls_preds if batch_dict['cls_preds_normalized'] else torch.sigmoid(src_cls_preds)
        scores, labels = torch.max(cls_preds, dim=-1)
        if dense:
            if batch_dict.get('has_class_labels', False):   # a second stage keeps the first stage's class
                labels = batch_dict['roi_labels' if 'roi_labels' in batch_dict else 'batch_pred_labels']
            else:
                labels = labels + 1
            box_preds = box_preds.reshape(b * n, box_preds.shape[-1])
            src_cls_preds = src_cls_preds.reshape(b * n, src_cls_preds.shape[-1])
            res = ops.dense_post_process(scores.reshape(-1), labels.reshape(-1), box_preds, b, plan['thresholds'],
                                         plan['nms_thresh'], plan['pre_max'], plan['post_max'],
                                         axis_aligned=plan['axis_aligned'], per_class=plan['per_class'])
        else:
            res = ops.point_post_process(scores, labels + 1, box_preds, b, plan['thresholds'], plan['nms_thresh'],
                                         plan['pre_max'], plan['post_max'], axis_aligned=plan['axis_aligned'],
                                         per_class=plan['per_class'])
        out = {'sel': res['sel'], 'count': res['count'], 'pred_boxes': res['boxes'], 'pred_scores': res['scores'],
               'pred_labels': res['labels']}
        if box_preds.shape[1] != 7 or box_preds.dtype != torch.float32:     # keep the caller's columns and dtype
            live = (res['sel'] >= 0).unsqueeze(-1)
            out['pred_boxes'] = box_preds[res['sel'].clamp_min(0)] * live.to(box_preds.dtype)
        if cfg.get('OUTPUT_RAW_SCORE', False):
            raw = torch.max(src_cls_preds, dim=-1)[0]
            out['pred_scores'] = raw[res['sel'].clamp_min(0)] * (res['sel'] >= 0).to(raw.dtype)
        if dense:
            out['layout_ok'] = torch.ones((), dtype=torch.bool, device=box_preds.device)
        else:
            frame = torch.arange(b, device=box_preds.device, dtype=batch_dict['batch_index'].dtype).view(b, 1)
            out['layout_ok'] = (batch_dict['batch_index'].reshape(b, n) == frame).all()
        thresh_list = cfg.get('RECALL_THRESH_LIST', None)
        if batch_dict.get('gt_boxes', None) is not None and thresh_list:
            out['recalled'], out['num_gt'] = ops.recall_count(res['boxes'], res['count'], batch_dict['gt_boxes'],
                                                              list(thresh_list))
        return out

    @staticmethod
    def _recall_dict(thresh_list, recalled, num_gt):
        """The reference's record (generate_recall_record :501-542) from per-frame counts already on the host; there is no
        roi head on these paths, so the roi_* entries stay 0."""
        recall_dict = {'gt': int(sum(num_gt))}
        for i, t in enumerate(thresh_list):
            recall_dict['roi_%s' % str(t)] = 0
            recall_dict['rcnn_%s' % str(t)] = int(sum(row[i] for row in recalled))
        return recall_dict

    def _post_processing_fused(self, batch_dict, plan):
        """pred_dicts from post_processing_static with ONE host read for the whole batch (counts, layout flag, recall);
        None when the layout flag says that the batch was not eligible after all."""
        st = self.post_processing_static(batch_dict, plan)
        b = plan['batch_size']
        parts = [st['count'].to(torch.int64), st['layout_ok'].to(torch.int64).view(1)]
        thresh_list = list(self.model_cfg.POST_PROCESSING.get('RECALL_THRESH_LIST', None) or [])
        if 'recalled' in st:
            parts += [st['num_gt'].to(torch.int64), st['recalled'].to(torch.int64).view(-1)]
        host = torch.cat(parts).tolist()
        if not host[b]:
            return None
        pred_dicts = [{'pred_boxes': st['pred_boxes'][i, :host[i]], 'pred_scores': st['pred_scores'][i, :host[i]],
                       'pred_labels': st['pred_labels'][i, :host[i]]} for i in range(b)]
        recall_dict = {}
        if 'recalled' in st:
            t = len(thresh_list)
            rec = host[2 * b + 1:]
            recall_dict = self._recall_dict(thresh_list, [rec[i * t:(i + 1) * t] for i in range(b)], host[b + 1:2 * b + 1])
        return pred_dicts, recall_dict

    def post_processing(self, batch_dict):
        cfg = self.model_cfg.POST_PROCESSING
        batch_size = batch_dict['batch_size']
        fused = cfg.get('FUSED', None)      # None: where it was measured faster; True / False force one path
        if fused is None or fused:
            plan = self._fused_post_plan(batch_dict)
            if plan is not None and fused is None and plan['n'] > self.FUSED_DEFAULT_MAX_N:
                plan = None
            done = self._post_processing_fused(batch_dict, plan) if plan is not None else None
            if done is not None:
                return done
        recall_dict, pred_dicts = {}, []
        for index in range(batch_size):
            if batch_dict.get('batch_index', None) is not None:    # flat (N, .) predictions of a point head
                assert batch_dict['batch_box_preds'].dim() == 2
                batch_mask = (batch_dict['batch_index'] == index)
            else:
                batch_mask = index
            box_preds = batch_dict['batch_box_preds'][batch_mask]
            cls_preds = batch_dict['batch_cls_preds'][batch_mask]
            src_cls_preds = cls_preds
            assert cls_preds.shape[1] in [1, self.num_class]
            if not batch_dict['cls_preds_normalized']:
                cls_preds = torch.sigmoid(cls_preds)
            if cfg.NMS_CONFIG.MULTI_CLASSES_NMS:
                raise NotImplementedError('MULTI_CLASSES_NMS is not used by the SECOND configuration')
            cls_preds, label_preds = torch.max(cls_preds, dim=-1)
            if batch_dict.get('has_class_labels', False):      # a second stage keeps the first stage's class (reference :281-283)
                label_key = 'roi_labels' if 'roi_labels' in batch_dict else 'batch_pred_labels'
                label_preds = batch_dict[label_key][index]
            else:
                label_preds = label_preds + 1
            thresh = cfg.SCORE_THRESH
            if isinstance(thresh, (list, tuple)):   # fork: per-class thresholds + a final cross-class NMS
                selected, selected_scores = model_nms_utils.multi_thresh(
                    box_scores=cls_preds, box_labels=label_preds, box_preds=box_preds, nms_config=cfg.NMS_CONFIG,
                    score_thresh=thresh)
            else:                                   # upstream: one class-agnostic NMS
                selected, selected_scores = model_nms_utils.class_agnostic_nms(
                    box_scores=cls_preds, box_preds=box_preds, nms_config=cfg.NMS_CONFIG, score_thresh=thresh)
            if cfg.get('OUTPUT_RAW_SCORE', False):
                selected_scores = torch.max(src_cls_preds, dim=-1)[0][selected]
            pred_dicts.append({'pred_boxes': box_preds[selected], 'pred_scores': selected_scores,
                               'pred_labels': label_preds[selected]})
        thresh_list = list(cfg.get('RECALL_THRESH_LIST', None) or [])
        if batch_dict.get('gt_boxes', None) is not None and thresh_list and batch_size > 0:
            recall_dict = self._eager_recall(pred_dicts, batch_dict['gt_boxes'], thresh_list)
        return pred_dicts, recall_dict

    def _eager_recall(self, pred_dicts, gt_boxes, thresh_list):
        """The recall record of per-frame pred_dicts: the kept boxes padded to one (B, K, 7) tensor, spx.ops.recall_count,
        one host read."""
        from spx import ops
        counts = [int(p['pred_boxes'].shape[0]) for p in pred_dicts]
        padded = gt_boxes.new_zeros((len(pred_dicts), max(max(counts), 1), 7), dtype=torch.float32)
        for i, p in enumerate(pred_dicts):
            padded[i, :counts[i]] = p['pred_boxes'][:, :7]
        count = torch.tensor(counts, dtype=torch.int32).to(gt_boxes.device)
        recalled, num_gt = ops.recall_count(padded, count, gt_boxes, thresh_list)
        return self._recall_dict(thresh_list, recalled.tolist(), num_gt.tolist())

    # ------------------------------------------------------------------ checkpoints (reference :544-625)
    def _load_state_dict(self, model_state_disk, *, strict=True):
        state_dict = self.state_dict()
        spconv_keys = find_all_spconv_keys(self)
        update = {}
        for key, val in model_state_disk.items():
            if key in spconv_keys and key in state_dict and state_dict[key].shape != val.shape:
                # spconv 1.x stored (k1,k2,k3,Cin,Cout); ours (= spconv 2.x implicit-gemm) is (Cout,k1,k2,k3,Cin)
                native = val.transpose(-1, -2)
                if native.shape == state_dict[key].shape:
                    val = native.contiguous()
                else:
                    assert val.dim() == 5, 'currently only spconv 3D is supported'
                    implicit = val.permute(4, 0, 1, 2, 3)
                    if implicit.shape == state_dict[key].shape:
                        val = implicit.contiguous()
            if key in state_dict and state_dict[key].shape == val.shape:
                update[key] = val
        if strict:
            self.load_state_dict(update)
        else:
            state_dict.update(update)
            self.load_state_dict(state_dict)
        return state_dict, update

    def load_params_from_file(self, filename, logger, to_cpu=False):
        if not os.path.isfile(filename):
            raise FileNotFoundError
        logger.info('==> Loading parameters from checkpoint %s to %s' % (filename, 'CPU' if to_cpu else 'GPU'))
        checkpoint = torch.load(filename, map_location=torch.device('cpu') if to_cpu else None, weights_only=True)
        state_dict, update = self._load_state_dict(checkpoint['model_state'], strict=False)
        for key in state_dict:
            if key not in update:
                logger.info('Not updated weight %s: %s' % (key, str(state_dict[key].shape)))
        logger.info('==> Done (loaded %d/%d)' % (len(update), len(state_dict)))

    def load_params_with_optimizer(self, filename, to_cpu=False, optimizer=None, logger=None):
        if not os.path.isfile(filename):
            raise FileNotFoundError
        checkpoint = torch.load(filename, map_location=torch.device('cpu') if to_cpu else None, weights_only=True)
        epoch, it = checkpoint.get('epoch', -1), checkpoint.get('it', 0.0)
        self._load_state_dict(checkpoint['model_state'], strict=True)
        if optimizer is not None and checkpoint.get('optimizer_state', None) is not None:
            optimizer.load_state_dict(checkpoint['optimizer_state'])
        return it, epoch
