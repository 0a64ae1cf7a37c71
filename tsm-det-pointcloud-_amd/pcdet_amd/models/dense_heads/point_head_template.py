"""PointHeadTemplate (reference pcdet/models/dense_heads/point_head_template.py): loss-module construction,
make_fc_layers and generate_predicted_boxes of the point heads.  Target assignment and the loss terms belong to the
point-head training path, which is not ported yet."""
import torch.nn as nn
import torch.nn.functional as F

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

    def generate_predicted_boxes(self, points, point_cls_preds, point_box_preds):
        """points (N, 3), point_cls_preds (N, num_class), point_box_preds (N, code_size) ->
        point_cls_preds (N, num_class), point_box_preds (N, 7 + C) decoded at the points."""
        _, pred_classes = point_cls_preds.max(dim=-1)
        point_box_preds = self.box_coder.decode_torch(point_box_preds, points, pred_classes + 1)
        return point_cls_preds, point_box_preds

    def forward(self, **kwargs):
        raise NotImplementedError
