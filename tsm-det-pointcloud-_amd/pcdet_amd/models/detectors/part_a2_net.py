"""PartA2Net (reference pcdet/models/detectors/PartA2_net.py): MeanVFE, the UNetV2 encoder-decoder, SECOND's BEV first
stage, PointIntraPartOffsetHead on the decoder's full-resolution features and PartA2FCHead.  forward and
get_training_loss as in the reference; post_processing is the template's.  tb_dict holds 0-dim tensors.

Departure: the point head and the RoI head read batch_dict['point_coords']; UNetV2 writes the voxel
centres of its point_features as 'raw_points_bxyz' (what the fork's other consumers read), so forward sets
point_coords = raw_points_bxyz in front of the point head, as upstream OpenPCDet's UNetV2 does itself."""
from .detector3d_template import Detector3DTemplate


class PartA2Net(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        for cur_module in self.module_list:
            if cur_module is self.point_head:
                batch_dict['point_coords'] = batch_dict['raw_points_bxyz']
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        disp_dict = {}
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_point, tb_dict = self.point_head.get_loss(tb_dict)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)

        loss = loss_rpn + loss_point + loss_rcnn
        return loss, tb_dict, disp_dict
