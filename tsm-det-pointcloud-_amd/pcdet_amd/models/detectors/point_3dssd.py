"""Point3DSSD (reference pcdet/models/detectors/point_3dssd.py), registered as '3DSSD': the fork's fast_cpc detector,
a VoxelPointNet2FSMSGDistillation backbone and a PointHeadVoteSASAStatisticDistillation head.  Eval only for now:
forward returns post_processing(batch_dict); training raises until the point-head losses are ported."""
from .detector3d_template import Detector3DTemplate


class Point3DSSD(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError('Point3DSSD: training is not ported (the point head has no targets or losses '
                                      'yet); use model.eval()')
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        pred_dicts, recall_dicts = self.post_processing(batch_dict)
        return pred_dicts, recall_dicts

    def get_training_loss(self):
        return self.point_head.get_loss()
