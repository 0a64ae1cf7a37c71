"""PointHeadVoteSASAStatisticDistillation — the fork's fast_cpc vote head (reference
pcdet/models/dense_heads/point_head_vote_sasa_statistic_distillation.py).

The constructor is the reference's whole constructor (teacher and student branches, the statistic buffers,
init_weights), so state_dict keys and shapes equal the reference's and fork checkpoints load.  Only the EVAL forward is
ported: the student branch with self.training False (reference forward, lines 1013-1295).  Its vote step and its tail
after s_shared_fc_layer run as two HIP ops (csrc/point_head.hip, include/spx.h §14) that read the modules' own
parameters at every call; the S_VSA_module and s_shared_fc_layer are the existing fused SA path and a GEMM.  The ops
compute no gradient, so the head's outputs carry no autograd history.

The training FORWARD is still not ported: forward in train mode raises NotImplementedError (the teacher branch, autograd
through the two fused ops and the statistic momentum update are missing), and get_loss, which reads what that forward
would leave behind, raises with it.  The two ends of training around it are here:
  - the target assignment, assign_targets_simple / assign_targets / assign_stu_targets, each one HIP launch for the
    whole batch with no host read (point_targets.py, csrc/point_targets.hip, include/spx.h §16);
  - the losses on a forward_ret_dict with the reference's keys, get_loss_torch (the torch composition) and
    get_loss_fused (point_losses.py, csrc/point_loss.hip, include/spx.h §17: vote, cls and box loss with their
    gradients from one launch group, each SASA layer from another, no host read).  Their tb_dict holds 0-d tensors
    instead of .item() floats, as AnchorHeadTemplate's does.
"""
import numpy as np
import torch
import torch.nn as nn

from spx import ops as spx_ops

from ...ops.pointnet2.pointnet2_batch import pointnet2_modules
from ...utils import box_coder_utils, loss_utils
from . import point_losses, point_targets
from .point_head_template import PointHeadTemplate


def _mlp_params(seq):
    """(w1, bn_mean, bn_var, bn_weight, bn_bias, eps, w2, b2) of Sequential(Conv1d, BatchNorm1d, ReLU, Conv1d)."""
    conv1, bn, relu, conv2 = seq
    assert isinstance(conv1, nn.Conv1d) and conv1.bias is None and isinstance(bn, nn.BatchNorm1d) \
        and isinstance(relu, nn.ReLU) and isinstance(conv2, nn.Conv1d) and conv2.bias is not None, \
        'the fused point-head tail needs Conv1d -> BatchNorm1d -> ReLU -> Conv1d(bias)'
    assert bn.track_running_stats and bn.affine
    return (conv1.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, conv2.weight, conv2.bias)


class PointHeadVoteSASAStatisticDistillation(PointHeadTemplate):
    """A vote-based detection head (3DSSD, https://arxiv.org/abs/2002.10187) with a teacher and a student branch and
    class-statistic-modulated classification blocks."""

    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        use_bn = self.model_cfg.USE_BN
        self.predict_boxes_when_training = predict_boxes_when_training
        self.voxel_size = kwargs['voxel_size']
        self.point_cloud_range = kwargs['point_cloud_range']

        self.vote_cfg = self.model_cfg.VOTE_CONFIG
        self.vote_layers = self.make_fc_layers(
            input_channels=input_channels, output_channels=3, fc_list=self.vote_cfg.VOTE_FC)

        self.vsa_cfg = self.model_cfg.VSA_CONFIG
        self.VSA_module, channel_out = self._vsa_module(self.vsa_cfg, 256, use_bn)

        self.shared_fc_layer = self._shared_fc(channel_out, self.model_cfg.DP_RATIO)
        channel_in = self.model_cfg.SHARED_FC[-1]

        self.cls_block = nn.ModuleList([self._cls_block() for _ in range(self.num_class)])
        self.register_buffer('object_statistic_features', torch.zeros(num_class, channel_in))
        self.register_buffer('object_momentum', torch.zeros(num_class, channel_in))
        self.register_buffer('object_mean', torch.zeros(num_class, channel_in))
        target_cfg = self.model_cfg.TARGET_CONFIG
        self.box_coder = getattr(box_coder_utils, target_cfg.BOX_CODER)(**target_cfg.BOX_CODER_CONFIG)

        self.reg_channel = self.box_coder.code_size

        self.reg_feature_layer = nn.Sequential(
            nn.Conv1d(in_channels=256, out_channels=64, kernel_size=1, bias=False),
            nn.BatchNorm1d(64, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True),
            nn.ReLU(),
        )
        self.reg_weight = nn.Parameter(torch.Tensor(1, 64, self.reg_channel))
        self.weight_gate = nn.Sequential(
            nn.Conv1d(in_channels=256, out_channels=512, kernel_size=1, bias=False),
            nn.BatchNorm1d(512, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True),
            nn.ReLU(),
            nn.Conv1d(in_channels=512, out_channels=64 * self.reg_channel, kernel_size=1, bias=False),
            nn.Sigmoid(),
        )
        self.weight_bias = nn.Sequential(
            nn.Conv1d(in_channels=256, out_channels=64, kernel_size=1, bias=False),
            nn.BatchNorm1d(64, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True),
            nn.ReLU(),
            nn.Conv1d(in_channels=64, out_channels=self.reg_channel, kernel_size=1, bias=True),
        )

        # student
        input_channels = 128
        self.s_vote_cfg = self.model_cfg.S_VOTE_CONFIG
        self.s_vote_layers = self.make_fc_layers(
            input_channels=input_channels, output_channels=3, fc_list=self.s_vote_cfg.VOTE_FC)

        self.s_vsa_cfg = self.model_cfg.S_VSA_CONFIG
        self.S_VSA_module, channel_out = self._vsa_module(self.s_vsa_cfg, 128, use_bn)

        self.s_shared_fc_layer = self._shared_fc(channel_out, self.model_cfg.S_FC_CONFIG.DP_RATIO)
        channel_in = self.model_cfg.SHARED_FC[-1]
        self.s_cls_block = nn.ModuleList([self._cls_block() for _ in range(self.num_class)])
        self.s_reg_layers = self.make_fc_layers(
            input_channels=channel_in, output_channels=self.box_coder.code_size, fc_list=self.model_cfg.REG_FC)
        self.init_weights(weight_init='kaiming')

    def _vsa_module(self, vsa_cfg, channel_in, use_bn):
        mlps = [[channel_in] + list(m) for m in vsa_cfg.MLPS]
        module = pointnet2_modules.VoxelPointnetSAModuleFSMSGDistillation(
            radii=vsa_cfg.RADIUS, query_range=vsa_cfg.QUERY_RANGE, sp_stride=vsa_cfg.SPARSE_TENSOR_STRIDE,
            stride=vsa_cfg.STRIDE, nsamples=vsa_cfg.NSAMPLE, mlps=mlps, pool_method='max_pool', use_xyz=True, bn=use_bn,
            sa_layer_idx=6, dilated_radius_group=vsa_cfg.get('DILATED_RADIUS_GROUP', False),
            voxel_size=self.voxel_size, point_cloud_range=self.point_cloud_range)
        return module, sum(m[-1] for m in mlps)

    def _shared_fc(self, channel_in, dp_ratio):
        layers = []
        fc = self.model_cfg.SHARED_FC
        for k in range(len(fc)):
            layers.extend([nn.Conv1d(channel_in, fc[k], kernel_size=1, bias=False), nn.BatchNorm1d(fc[k]), nn.ReLU()])
            channel_in = fc[k]
            if k != len(fc) - 1 and dp_ratio > 0:
                layers.append(nn.Dropout(dp_ratio))
        return nn.Sequential(*layers)

    @staticmethod
    def _cls_block():
        return nn.Sequential(
            nn.Conv1d(in_channels=256, out_channels=64, kernel_size=1, bias=False),
            nn.BatchNorm1d(64),
            nn.ReLU(),
            nn.Conv1d(in_channels=64, out_channels=1, kernel_size=1, bias=True),
        )

    def init_weights(self, weight_init='kaiming'):
        if weight_init == 'kaiming':
            init_func = nn.init.kaiming_normal_
        elif weight_init == 'xavier':
            init_func = nn.init.xavier_normal_
        elif weight_init == 'normal':
            init_func = nn.init.normal_
        else:
            raise NotImplementedError

        for m in self.modules():
            if isinstance(m, nn.Conv2d) or isinstance(m, nn.Conv1d):
                if weight_init == 'normal':
                    init_func(m.weight, mean=0, std=0.001)
                else:
                    init_func(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

        pi = 0.01
        for i in range(self.num_class):
            nn.init.constant_(self.cls_block[i][3].bias, -np.log((1 - pi) / pi))
            nn.init.constant_(self.s_cls_block[i][3].bias, -np.log((1 - pi) / pi))
        nn.init.kaiming_normal_(self.reg_weight)
        nn.init.constant_(self.weight_bias[3].bias, 0)

    def build_losses(self, losses_cfg):
        """The reference's loss modules (parameter- and buffer-free); their forward is the training PR's."""
        if losses_cfg.LOSS_CLS.startswith('WeightedBinaryCrossEntropy'):
            self.add_module('cls_loss_func', loss_utils.WeightedBinaryCrossEntropyLoss())
        elif losses_cfg.LOSS_CLS == 'WeightedCrossEntropy':
            self.add_module('cls_loss_func', loss_utils.WeightedCrossEntropyLoss())
        elif losses_cfg.LOSS_CLS == 'FocalLoss':
            self.add_module('cls_loss_func',
                            loss_utils.SigmoidFocalClassificationLoss(**losses_cfg.get('LOSS_CLS_CONFIG', {})))
        else:
            raise NotImplementedError

        if losses_cfg.LOSS_REG == 'WeightedSmoothL1Loss':
            self.add_module('reg_loss_func', loss_utils.WeightedSmoothL1Loss(
                code_weights=losses_cfg.LOSS_WEIGHTS.get('code_weights', None),
                **losses_cfg.get('LOSS_REG_CONFIG', {})))
        else:
            raise NotImplementedError('LOSS_REG %s is not ported' % losses_cfg.LOSS_REG)

        loss_sasa_cfg = losses_cfg.get('LOSS_SASA_CONFIG', None)
        if loss_sasa_cfg is not None:
            self.enable_sasa = True
            self.add_module('loss_point_sasa', loss_utils.PointSASALoss(**loss_sasa_cfg))
        else:
            self.enable_sasa = False

    def make_fc_layers(self, input_channels, output_channels, fc_list):
        fc_layers = []
        pre_channel = input_channels
        for k in range(0, fc_list.__len__()):
            fc_layers.extend([
                nn.Conv1d(pre_channel, fc_list[k], kernel_size=1, bias=False),
                nn.BatchNorm1d(fc_list[k]),
                nn.ReLU()
            ])
            pre_channel = fc_list[k]
        fc_layers.append(nn.Conv1d(pre_channel, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*fc_layers)

    def assign_targets_simple(self, points, gt_boxes, extra_width=None, set_ignore_flag=True):
        """The vote targets.  points (N1 + N2 + ..., 4) [bs_idx, x, y, z], gt_boxes (B, M, 8) -> point_cls_labels,
        point_reg_labels (., 3)."""
        return point_targets.assign_targets_simple(points, gt_boxes, extra_width=extra_width,
                                                   set_ignore_flag=set_ignore_flag)

    def _assign_mask_targets(self, points, gt_boxes):
        target_cfg = self.model_cfg.TARGET_CONFIG
        if target_cfg.ASSIGN_METHOD != 'mask':
            raise NotImplementedError('ASSIGN_METHOD %s is not ported (the fast_cpc configs use mask)'
                                      % target_cfg.ASSIGN_METHOD)
        return point_targets.assign_stack_targets_mask(points, gt_boxes, self.box_coder, self.num_class,
                                                       central_radius=target_cfg.get('GT_CENTRAL_RADIUS', 2.0))

    def assign_targets(self, input_dict):
        """The teacher's targets on point_vote_coords (N1 + N2 + ..., 4) against gt_boxes (B, M, 8) ->
        point_cls_labels, point_reg_labels (., code_size), point_box_labels (., 7)."""
        return self._assign_mask_targets(input_dict['point_vote_coords'], input_dict['gt_boxes'])

    def assign_stu_targets(self, input_dict):
        """The student's targets: the same on s_point_vote_coords."""
        return self._assign_mask_targets(input_dict['s_point_vote_coords'], input_dict['gt_boxes'])

    def get_loss(self, tb_dict=None):
        raise NotImplementedError('PointHeadVoteSASAStatisticDistillation: training is not ported (needs the teacher '
                                  'forward, the vote, cls, box, corner, iou and SASA losses and the statistic momentum '
                                  'update; their targets are assign_targets_simple / assign_targets / '
                                  'assign_stu_targets)')

    def _get_loss(self, ret_dict, tb_dict, fused):
        ret_dict = self.forward_ret_dict if ret_dict is None else ret_dict
        if ret_dict is None:
            raise ValueError('no ret_dict given and no forward_ret_dict to read')
        tb_dict = {} if tb_dict is None else tb_dict
        head_loss = point_losses.head_loss_fused if fused else point_losses.head_loss_torch
        point_loss, parts = head_loss(ret_dict, self.model_cfg, self.box_coder, self.reg_loss_func, self.cls_loss_func)
        tb_dict.update({'point_loss_vote': parts[0], 'point_loss_cls': parts[1], 'point_loss_box': parts[2],
                        'vote_loss_reg': parts[0],
                        'point_pos_num': (ret_dict['s_point_cls_labels'] > 0).sum()})
        if self.enable_sasa:
            layer_losses = self.loss_point_sasa.loss_forward(
                ret_dict['point_sasa_preds'], ret_dict['point_sasa_labels'], ret_dict['point_sasa'],
                ret_dict['point_sasa_boxes'], ret_dict['point_sasa_parts'], fused=fused)
            point_loss_sasa = None
            for i, layer_loss in enumerate(layer_losses):
                if layer_loss is None:
                    continue
                layer_loss = layer_loss.reshape(())
                point_loss_sasa = layer_loss if point_loss_sasa is None else point_loss_sasa + layer_loss
                tb_dict['point_loss_sasa_layer_%d' % i] = layer_loss.detach()
            if point_loss_sasa is not None:
                tb_dict['point_loss_sasa'] = point_loss_sasa.detach()
                point_loss = point_loss + point_loss_sasa
        return point_loss, tb_dict

    def get_loss_torch(self, ret_dict=None, tb_dict=None):
        """The reference's get_loss as a torch composition on ret_dict (default: forward_ret_dict) with the keys listed
        in point_losses.py, plus point_sasa_preds / point_sasa_labels / point_sasa / point_sasa_boxes / point_sasa_parts
        when SASA is enabled -> (point_loss, tb_dict of 0-d tensors)."""
        return self._get_loss(ret_dict, tb_dict, fused=False)

    def get_loss_fused(self, ret_dict=None, tb_dict=None):
        """The same through the fused HIP ops: GPU tensors only, no host read (captures in a graph).  Settings the kernel
        does not cover raise NotImplementedError."""
        return self._get_loss(ret_dict, tb_dict, fused=True)

    def forward(self, batch_dict):
        """Eval forward of the student branch.
        batch_dict: batch_size, s_point_coords (B * N, 4) [bs_idx, x, y, z], s_point_features (B * N, 128),
            s_last_features, s_last_sp_tensor, s_last_centroids, s_last_centroid_voxel_idxs.
        Adds s_batch_index, s_point_candidate_coords, s_point_vote_coords (M, 4), s_point_cls_scores, s_point_box_preds,
            batch_cls_preds (M, num_class) logits, batch_box_preds (M, 7), cls_preds_normalized False, batch_index."""
        if self.training:
            raise NotImplementedError('PointHeadVoteSASAStatisticDistillation: only the eval forward is ported; training '
                                      'needs the teacher branch, target assignment and the point-head losses')
        if self.box_coder.use_mean_size or self.box_coder.pred_velo:
            raise NotImplementedError('the fused point-head decode supports PointBinResidualCoder with '
                                      'use_mean_size False and pred_velo False (the fast_cpc setting)')
        batch_size = batch_dict['batch_size']
        s_point_coords = batch_dict['s_point_coords']
        s_batch_idx, s_point_coords = s_point_coords[:, 0], s_point_coords[:, 1:4]
        s_batch_idx = s_batch_idx.view(batch_size, -1, 1)
        s_point_coords = s_point_coords.view(batch_size, -1, 3).contiguous()
        s_point_features = batch_dict['s_point_features'].reshape(
            batch_size, s_point_coords.size(1), -1).permute(0, 2, 1).contiguous()

        lo, hi = self.model_cfg.SAMPLE_RANGE
        s_sample_batch_idx = s_batch_idx[:, lo:hi, :].contiguous()
        s_candidate_coords = s_point_coords[:, lo:hi, :].contiguous()
        s_vote_coords = spx_ops.point_vote(s_point_features, s_point_coords, lo, hi, _mlp_params(self.s_vote_layers),
                                           self.s_vote_cfg.MAX_TRANSLATION_RANGE)
        ret_dict = {
            'batch_size': batch_size,
            's_point_candidate_coords': s_candidate_coords.view(-1, 3),
            's_point_vote_coords': s_vote_coords.view(-1, 3),
        }
        s_sample_batch_idx_flatten = s_sample_batch_idx.view(-1, 1)
        batch_dict['s_batch_index'] = s_sample_batch_idx_flatten.squeeze(-1)
        batch_dict['s_point_candidate_coords'] = torch.cat(
            (s_sample_batch_idx_flatten, ret_dict['s_point_candidate_coords']), dim=-1)
        batch_dict['s_point_vote_coords'] = torch.cat(
            (s_sample_batch_idx_flatten, ret_dict['s_point_vote_coords']), dim=-1)

        _, s_point_features, _, _, _, _, _, _ = self.S_VSA_module(
            xyz=s_point_coords, new_xyz=s_vote_coords, features=batch_dict['s_last_features'],
            sp_tensor=batch_dict['s_last_sp_tensor'], centroids=batch_dict['s_last_centroids'],
            centroid_voxel_idxs=batch_dict['s_last_centroid_voxel_idxs'])
        s_point_features = self.s_shared_fc_layer(s_point_features)

        # the student's class blocks are modulated by the TEACHER's statistic buffer, as in the reference
        s_point_cls_preds, s_point_reg_preds, s_point_box_preds = spx_ops.point_head_predict(
            s_point_features, self.object_statistic_features, ret_dict['s_point_vote_coords'],
            [_mlp_params(m) for m in self.s_cls_block], _mlp_params(self.s_reg_layers), self.box_coder.angle_bin_num)
        s_point_cls_scores = torch.sigmoid(s_point_cls_preds)
        batch_dict['s_point_cls_scores'] = s_point_cls_scores
        batch_dict['s_point_box_preds'] = s_point_box_preds
        ret_dict.update({'s_point_cls_preds': s_point_cls_preds,
                         's_point_reg_preds': s_point_reg_preds,
                         's_point_box_preds': s_point_box_preds,
                         's_point_cls_scores': s_point_cls_scores})

        batch_dict['batch_cls_preds'] = s_point_cls_preds
        batch_dict['batch_box_preds'] = s_point_box_preds
        batch_dict['cls_preds_normalized'] = False
        batch_dict['batch_index'] = batch_dict['s_batch_index']
        self.forward_ret_dict = ret_dict
        return batch_dict
