"""CenterPoint (reference pcdet/models/detectors/centerpoint.py:4-50): run the module list, then the centre head's loss
or its already decoded and NMS-ed boxes with the recall record.  In static mode (`static_caps` in the batch dict, what
models/inference.py::GraphedCenterPoint captures) the boxes and the recall counts stay on the device at static capacity
(post_processing_static); pred_dicts_from_static turns them into the usual return value with one host read."""
import torch

from .detector3d_template import Detector3DTemplate


class CenterPoint(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        if 'final_box_static' in batch_dict:        # static mode (static_caps in the batch dict): no host read
            return self.post_processing_static(batch_dict)
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {'loss_rpn': loss_rpn.detach(), **tb_dict}
        return loss_rpn, tb_dict, {}

    def post_processing_static(self, batch_dict):
        """Static mode (`static_caps` in the batch dict): the head's `final_box_static` — pred_boxes (B, cap, 7 | 9),
        pred_scores (B, cap), pred_labels (B, cap) int64, count (B) int32, zeros past count — and, with gt_boxes and
        RECALL_THRESH_LIST, recalled (B, T) int32 and num_gt (B) int32 (spx.ops.recall_count).  No host read."""
        from spx import ops
        if 'final_box_static' not in batch_dict:
            raise KeyError('post_processing_static needs the static outputs of the centre head: put static_caps in the '
                           'batch dict and run the model in eval mode')
        out = dict(batch_dict['final_box_static'])
        thresh_list = self.model_cfg.POST_PROCESSING.get('RECALL_THRESH_LIST', None)
        if batch_dict.get('gt_boxes', None) is not None and thresh_list:
            out['recalled'], out['num_gt'] = ops.recall_count(out['pred_boxes'][..., :7].contiguous(), out['count'],
                                                              batch_dict['gt_boxes'], list(thresh_list))
        return out

    def pred_dicts_from_static(self, static):
        """What forward returns in eval, (pred_dicts, recall_dict), from post_processing_static's dict: ONE host read."""
        b = static['count'].shape[0]
        parts = [static['count'].to(torch.int64)]
        if 'recalled' in static:
            parts += [static['num_gt'].to(torch.int64), static['recalled'].to(torch.int64).view(-1)]
        host = torch.cat(parts).tolist()
        pred_dicts = [{'pred_boxes': static['pred_boxes'][i, :host[i]], 'pred_scores': static['pred_scores'][i, :host[i]],
                       'pred_labels': static['pred_labels'][i, :host[i]]} for i in range(b)]
        recall_dict = {}
        if 'recalled' in static and b > 0:
            thresh_list = list(self.model_cfg.POST_PROCESSING.RECALL_THRESH_LIST)
            t = len(thresh_list)
            rec = host[2 * b:]
            recall_dict = self._recall_dict(thresh_list, [rec[i * t:(i + 1) * t] for i in range(b)], host[b:2 * b])
        return pred_dicts, recall_dict

    def post_processing(self, batch_dict):
        """The head has decoded, thresholded and NMS-ed `final_box_dicts`; what is left of the template's
        post-processing is the recall record (gt, roi_*, rcnn_* per RECALL_THRESH_LIST) over those boxes."""
        final_pred_dict = batch_dict['final_box_dicts']
        thresh_list = list(self.model_cfg.POST_PROCESSING.get('RECALL_THRESH_LIST', None) or [])
        recall_dict = {}
        if batch_dict.get('gt_boxes', None) is not None and thresh_list and batch_dict['batch_size'] > 0:
            recall_dict = self._eager_recall(final_pred_dict, batch_dict['gt_boxes'], thresh_list)
        return final_pred_dict, recall_dict
