"""CenterPoint (reference pcdet/models/detectors/centerpoint.py:4-50): run the module list, then the centre head's loss
or its already decoded and NMS-ed boxes with the recall record."""
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
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {'loss_rpn': loss_rpn.detach(), **tb_dict}
        return loss_rpn, tb_dict, {}

    def post_processing(self, batch_dict):
        """The head has decoded, thresholded and NMS-ed `final_box_dicts`; what is left of the template's
        post-processing is the recall record (gt, roi_*, rcnn_* per RECALL_THRESH_LIST) over those boxes."""
        final_pred_dict = batch_dict['final_box_dicts']
        thresh_list = list(self.model_cfg.POST_PROCESSING.get('RECALL_THRESH_LIST', None) or [])
        recall_dict = {}
        if batch_dict.get('gt_boxes', None) is not None and thresh_list and batch_dict['batch_size'] > 0:
            recall_dict = self._eager_recall(final_pred_dict, batch_dict['gt_boxes'], thresh_list)
        return final_pred_dict, recall_dict
