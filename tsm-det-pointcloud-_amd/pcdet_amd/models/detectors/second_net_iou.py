"""SECONDNetIoU (reference pcdet/models/detectors/second_net_iou.py:7-177): SECOND with the SECONDHead IoU branch as its
second stage.  The NMS score of a box is its predicted IoU, its class score, or a mix of the two (NMS_CONFIG.SCORE_TYPE).

Two departures, both recorded in DESIGN.md §6h:
  * score_by_class walks all num_class classes.  The reference walks range(len(torch.unique(labels))), which reads the
    label set back to the host and leaves class c at score 0 whenever a class below c is absent from the frame.
  * num_pts_iou_cls (a CPU points-in-boxes count per frame) is refused by name."""
import torch

from ..model_utils.model_nms_utils import class_agnostic_nms
from .detector3d_template import Detector3DTemplate


class SECONDNetIoU(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        batch_dict['dataset_cfg'] = self.dataset.dataset_cfg
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        disp_dict = {}
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        loss = loss_rpn + loss_rcnn
        return loss, tb_dict, disp_dict

    def set_nms_score_by_class(self, iou_preds, cls_preds, label_preds, score_by_class):
        nms_scores = torch.zeros_like(iou_preds)
        for i in range(self.num_class):
            score_type = score_by_class[self.class_names[i]]
            if score_type not in ('iou', 'cls'):
                raise NotImplementedError('SCORE_BY_CLASS %s' % score_type)
            nms_scores = torch.where(label_preds == (i + 1), iou_preds if score_type == 'iou' else cls_preds, nms_scores)
        return nms_scores

    def post_processing(self, batch_dict):
        """batch_cls_preds (B, N, 1 | classes): the head's IoU logits; roi_scores (B, N): the first stage's class scores;
        batch_box_preds (B, N, 7 + C); roi_labels (B, N) in 1 .. classes.  Returns pred_dicts with pred_boxes, pred_scores,
        pred_labels, pred_cls_scores, pred_iou_scores, and the recall record taken on the RoIs."""
        post_process_cfg = self.model_cfg.POST_PROCESSING
        nms_config = post_process_cfg.NMS_CONFIG
        batch_size = batch_dict['batch_size']
        if nms_config.MULTI_CLASSES_NMS:
            raise NotImplementedError('MULTI_CLASSES_NMS')
        if post_process_cfg.get('OUTPUT_RAW_SCORE', False):
            raise NotImplementedError('OUTPUT_RAW_SCORE')
        score_type = nms_config.get('SCORE_TYPE', None)
        pred_dicts = []
        for index in range(batch_size):
            if batch_dict.get('batch_index', None) is not None:
                assert batch_dict['batch_cls_preds'].dim() == 2
                batch_mask = (batch_dict['batch_index'] == index)
            else:
                assert batch_dict['batch_cls_preds'].dim() == 3
                batch_mask = index
            box_preds = batch_dict['batch_box_preds'][batch_mask]
            iou_preds = batch_dict['batch_cls_preds'][batch_mask]
            cls_preds = batch_dict['roi_scores'][batch_mask]
            assert iou_preds.shape[1] in [1, self.num_class]
            if not batch_dict['cls_preds_normalized']:
                iou_preds = torch.sigmoid(iou_preds)
                cls_preds = torch.sigmoid(cls_preds)
            iou_preds, label_preds = torch.max(iou_preds, dim=-1)
            label_preds = batch_dict['roi_labels'][index] if batch_dict.get('has_class_labels', False) else label_preds + 1
            if nms_config.get('SCORE_BY_CLASS', None) and score_type == 'score_by_class':
                nms_scores = self.set_nms_score_by_class(iou_preds, cls_preds, label_preds, nms_config.SCORE_BY_CLASS)
            elif score_type == 'iou' or score_type is None:
                nms_scores = iou_preds
            elif score_type == 'cls':
                nms_scores = cls_preds
            elif score_type == 'weighted_iou_cls':
                nms_scores = nms_config.SCORE_WEIGHTS.iou * iou_preds + nms_config.SCORE_WEIGHTS.cls * cls_preds
            elif score_type == 'num_pts_iou_cls':
                raise NotImplementedError('SCORE_TYPE num_pts_iou_cls is not supported')
            else:
                raise NotImplementedError('SCORE_TYPE %s' % score_type)
            selected, selected_scores = class_agnostic_nms(box_scores=nms_scores, box_preds=box_preds, nms_config=nms_config,
                                                           score_thresh=post_process_cfg.SCORE_THRESH)
            pred_dicts.append({'pred_boxes': box_preds[selected], 'pred_scores': selected_scores,
                               'pred_labels': label_preds[selected], 'pred_cls_scores': cls_preds[selected],
                               'pred_iou_scores': iou_preds[selected]})
        recall_dict = {}
        thresh_list = list(post_process_cfg.get('RECALL_THRESH_LIST', None) or [])
        if batch_dict.get('gt_boxes', None) is not None and thresh_list and batch_size > 0:
            recall_dict = self._roi_recall(batch_dict, thresh_list)
        return pred_dicts, recall_dict

    def _roi_recall(self, batch_dict, thresh_list):
        """The reference's generate_recall_record with box_preds = the RoIs (second_net_iou.py:161-165): the head does not
        move the boxes, so roi_* and rcnn_* are the same counts.  One host read for the batch."""
        from spx import ops
        rois = batch_dict['rois'] if batch_dict.get('rois', None) is not None else batch_dict['batch_box_preds']
        boxes = rois[..., 0:7].float().contiguous()
        count = torch.full((boxes.shape[0],), boxes.shape[1], dtype=torch.int32, device=boxes.device)
        recalled, num_gt = ops.recall_count(boxes, count, batch_dict['gt_boxes'], thresh_list)
        recall_dict = self._recall_dict(thresh_list, recalled.tolist(), num_gt.tolist())
        for t in thresh_list:
            recall_dict['roi_%s' % str(t)] = recall_dict['rcnn_%s' % str(t)]
        return recall_dict
