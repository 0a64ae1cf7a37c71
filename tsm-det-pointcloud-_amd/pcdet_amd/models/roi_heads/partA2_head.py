"""PartA2FCHead (reference pcdet/models/roi_heads/partA2_head.py:10-224): RoI-aware pooling of the point head's part
locations (avg) and of the backbone's point features (max) into a sparse o x o x o grid per RoI, two sparse conv
branches, shared FC layers and a class / box branch.  Reference constructor signature, submodule tree (state_dict
keys), init_weights, post_act_block and fake_sparse_idx.

Three pooling paths (ROI_AWARE_POOL.FUSED / STATIC_ROWS), recorded with the other departures in DESIGN.md §6l:
  * FUSED: False — the composition: the reference's per-frame loop over RoIAwarePool3d (two calls per frame into dense
    (N, o, o, o, C) grids), sum(-1).nonzero() and the gather of the non-empty cells;
  * FUSED: True — spx.ops.roiaware_sparse_collect, ONE host read of n_rows, roiaware_sparse_pool(rows = n_rows), then
    ordinary SparseConvTensors (csrc/roiaware_sparse.hip, include/spx.h §30);
  * FUSED with STATIC_ROWS: <cap> — no host read: the pool writes `cap` rows, the sparse tensors carry n_valid, conv_part,
    conv_rpn and .dense() run at capacity; an overflow is reported in the device status word (spx.ops.check_status),
    `faked` invalidates the training labels with torch.where.
ROI_AWARE_POOL.MAX_FRAME_POINTS (optional, fused paths) is a host bound on the longest frame: it sizes the per-RoI point
records (default: all points); a longer frame is reported in the status word.
The fused paths are defined for non-negative part values, so DISABLE_PART (raw coordinates as part features) is refused
on them by name.  The SEG_MASK_SCORE_THRESH mask is a torch.where instead of a masked assignment (no host read).  A
static-capacity sparse tensor on the input side (encoded_spconv_tensor with n_valid set) is refused by name: the point
features would carry dead rows."""
import numpy as np
import torch
import torch.nn as nn

from spx import ops

from ...ops.roiaware_pool3d import roiaware_pool3d_utils
from ...utils.spconv_utils import spconv
from .roi_head_template import RoIHeadTemplate

FUSED_DEFAULT = True       # decided by tools/part_a2_bench.py: no measured row loses (profiles/part_a2_bench.log)


class PartA2FCHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg

        self.SA_modules = nn.ModuleList()
        block = self.post_act_block

        c0 = self.model_cfg.ROI_AWARE_POOL.NUM_FEATURES // 2
        self.conv_part = spconv.SparseSequential(
            block(4, 64, 3, padding=1, indice_key='rcnn_subm1'),
            block(64, c0, 3, padding=1, indice_key='rcnn_subm1_1'),
        )
        self.conv_rpn = spconv.SparseSequential(
            block(input_channels, 64, 3, padding=1, indice_key='rcnn_subm2'),
            block(64, c0, 3, padding=1, indice_key='rcnn_subm1_2'),
        )

        shared_fc_list = []
        pool_size = self.model_cfg.ROI_AWARE_POOL.POOL_SIZE
        pre_channel = self.model_cfg.ROI_AWARE_POOL.NUM_FEATURES * pool_size * pool_size * pool_size
        for k in range(0, self.model_cfg.SHARED_FC.__len__()):
            shared_fc_list.extend([
                nn.Conv1d(pre_channel, self.model_cfg.SHARED_FC[k], kernel_size=1, bias=False),
                nn.BatchNorm1d(self.model_cfg.SHARED_FC[k]),
                nn.ReLU()
            ])
            pre_channel = self.model_cfg.SHARED_FC[k]

            if k != self.model_cfg.SHARED_FC.__len__() - 1 and self.model_cfg.DP_RATIO > 0:
                shared_fc_list.append(nn.Dropout(self.model_cfg.DP_RATIO))

        self.shared_fc_layer = nn.Sequential(*shared_fc_list)

        self.cls_layers = self.make_fc_layers(
            input_channels=pre_channel, output_channels=self.num_class, fc_list=self.model_cfg.CLS_FC
        )
        self.reg_layers = self.make_fc_layers(
            input_channels=pre_channel,
            output_channels=self.box_coder.code_size * self.num_class,
            fc_list=self.model_cfg.REG_FC
        )

        self.roiaware_pool3d_layer = roiaware_pool3d_utils.RoIAwarePool3d(
            out_size=self.model_cfg.ROI_AWARE_POOL.POOL_SIZE,
            max_pts_each_voxel=self.model_cfg.ROI_AWARE_POOL.MAX_POINTS_PER_VOXEL
        )
        self.fused = bool(self.model_cfg.ROI_AWARE_POOL.get('FUSED', FUSED_DEFAULT))
        self.static_rows = self.model_cfg.ROI_AWARE_POOL.get('STATIC_ROWS', None)
        if self.static_rows is not None and not self.fused:
            raise NotImplementedError('PartA2FCHead: ROI_AWARE_POOL.STATIC_ROWS needs ROI_AWARE_POOL.FUSED')
        if self.fused and self.model_cfg.get('DISABLE_PART', False):
            raise NotImplementedError('PartA2FCHead: DISABLE_PART is not supported on the fused RoI-aware pooling (its emit '
                                      'rule is defined for non-negative part values); set ROI_AWARE_POOL.FUSED: False')
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
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
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    def post_act_block(self, in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0, conv_type='subm'):
        if conv_type == 'subm':
            m = spconv.SparseSequential(
                spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key),
                nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01),
                nn.ReLU(),
            )
        elif conv_type == 'spconv':
            m = spconv.SparseSequential(
                spconv.SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                                    bias=False, indice_key=indice_key),
                nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01),
                nn.ReLU(),
            )
        elif conv_type == 'inverseconv':
            m = spconv.SparseSequential(
                spconv.SparseInverseConv3d(in_channels, out_channels, kernel_size,
                                           indice_key=indice_key, bias=False),
                nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01),
                nn.ReLU(),
            )
        else:
            raise NotImplementedError
        return m

    def part_features(self, batch_dict):
        """(N, 4): the part offsets (the coordinates with DISABLE_PART), zeroed below SEG_MASK_SCORE_THRESH, and the
        detached score."""
        point_coords = batch_dict['point_coords'][:, 1:4]
        scores = batch_dict['point_cls_scores'].view(-1, 1).detach()
        offsets = batch_dict['point_part_offset'] if not self.model_cfg.get('DISABLE_PART', False) else point_coords
        offsets = torch.where(scores < self.model_cfg.SEG_MASK_SCORE_THRESH, torch.zeros_like(offsets), offsets)
        return torch.cat((offsets, scores.to(offsets.dtype)), dim=1)

    def roiaware_pool(self, batch_dict):
        """The composition: rois (B, num_rois, 7 + C), point_coords (num_points, 4) [bs_idx, x, y, z], point_features
        (num_points, C), point_cls_scores, point_part_offset -> dense pooled part (B * N, o, o, o, 4) and rpn features
        (B * N, o, o, o, C)."""
        batch_size = batch_dict['batch_size']
        batch_idx = batch_dict['point_coords'][:, 0]
        point_coords = batch_dict['point_coords'][:, 1:4]
        point_features = batch_dict['point_features']
        part_features = self.part_features(batch_dict)

        rois = batch_dict['rois']

        pooled_part_features_list, pooled_rpn_features_list = [], []

        for bs_idx in range(batch_size):
            bs_mask = (batch_idx == bs_idx)
            cur_point_coords = point_coords[bs_mask]
            cur_part_features = part_features[bs_mask]
            cur_rpn_features = point_features[bs_mask]
            cur_roi = rois[bs_idx][:, 0:7].contiguous()  # (N, 7)

            pooled_part_features = self.roiaware_pool3d_layer.forward(
                cur_roi, cur_point_coords, cur_part_features, pool_method='avg'
            )  # (N, out_x, out_y, out_z, 4)
            pooled_rpn_features = self.roiaware_pool3d_layer.forward(
                cur_roi, cur_point_coords, cur_rpn_features, pool_method='max'
            )  # (N, out_x, out_y, out_z, C)

            pooled_part_features_list.append(pooled_part_features)
            pooled_rpn_features_list.append(pooled_rpn_features)

        pooled_part_features = torch.cat(pooled_part_features_list, dim=0)  # (B * N, out_x, out_y, out_z, 4)
        pooled_rpn_features = torch.cat(pooled_rpn_features_list, dim=0)  # (B * N, out_x, out_y, out_z, C)

        return pooled_part_features, pooled_rpn_features

    @staticmethod
    def fake_sparse_idx(sparse_idx, batch_size_rcnn):
        # at most one sample is non-empty, then fake the first voxels of each sample(BN needs at least
        # two values each channel) as non-empty for the below calculation
        sparse_idx = sparse_idx.new_zeros((batch_size_rcnn, 3))
        bs_idxs = torch.arange(batch_size_rcnn).type_as(sparse_idx).view(-1, 1)
        sparse_idx = torch.cat((bs_idxs, sparse_idx), dim=1)
        return sparse_idx

    def sparse_pool_composed(self, batch_dict, targets_dict):
        """-> part rows (n, 4), rpn rows (n, C), coords (n, 4) int32 [r, x, y, z], n_valid None."""
        pooled_part_features, pooled_rpn_features = self.roiaware_pool(batch_dict)
        batch_size_rcnn = pooled_part_features.shape[0]  # (B * N, out_x, out_y, out_z, 4)
        sparse_idx = pooled_part_features.sum(dim=-1).nonzero()  # (non_empty_num, 4) ==> [bs_idx, x_idx, y_idx, z_idx]
        if sparse_idx.shape[0] < 3:
            sparse_idx = self.fake_sparse_idx(sparse_idx, batch_size_rcnn)
            if self.training:
                # these are invalid samples
                targets_dict['rcnn_cls_labels'].fill_(-1)
                targets_dict['reg_valid_mask'].fill_(-1)

        part_features = pooled_part_features[sparse_idx[:, 0], sparse_idx[:, 1], sparse_idx[:, 2], sparse_idx[:, 3]]
        rpn_features = pooled_rpn_features[sparse_idx[:, 0], sparse_idx[:, 1], sparse_idx[:, 2], sparse_idx[:, 3]]
        return part_features, rpn_features, sparse_idx.int().contiguous(), None

    def sparse_pool_fused(self, batch_dict, targets_dict):
        """The same rows from spx.ops.roiaware_sparse_collect / roiaware_sparse_pool; with STATIC_ROWS at capacity, with
        n_valid the device row count.  Writes batch_dict['roiaware_layout_ok'] (0-dim device bool: the points were
        grouped by ascending frame; the results are meaningless otherwise)."""
        pool_cfg = self.model_cfg.ROI_AWARE_POOL
        size = pool_cfg.POOL_SIZE
        out_size = (size, size, size) if isinstance(size, int) else tuple(size)
        state = ops.roiaware_sparse_collect(batch_dict['rois'][:, :, 0:7], batch_dict['point_coords'],
                                            self.part_features(batch_dict), batch_dict['point_features'], out_size,
                                            pool_cfg.MAX_POINTS_PER_VOXEL,
                                            max_frame_points=pool_cfg.get('MAX_FRAME_POINTS', None))
        batch_dict['roiaware_layout_ok'] = state.layout_ok
        if self.static_rows is None:
            rows, n_valid = int(state.n_rows.item()), None            # the one host read of the eager path
        else:
            rows, n_valid = int(self.static_rows), state.n_rows
        out = ops.roiaware_sparse_pool(state, rows)
        if self.training:
            faked = out['faked'] != 0
            for key in ('rcnn_cls_labels', 'reg_valid_mask'):
                targets_dict[key] = torch.where(faked, -torch.ones_like(targets_dict[key]), targets_dict[key])
        return out['part'], out['rpn'], out['coords'], n_valid

    def forward(self, batch_dict):
        encoded = batch_dict.get('encoded_spconv_tensor', None)
        if getattr(encoded, 'n_valid', None) is not None:
            raise NotImplementedError('PartA2FCHead does not support static-capacity sparse tensors (encoded_spconv_tensor '
                                      'has n_valid set): point_features would carry dead rows')
        targets_dict = self.proposal_layer(
            batch_dict, nms_config=self.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST']
        )
        if self.training:
            targets_dict = batch_dict.get('roi_targets_dict', None)
            if targets_dict is None:
                targets_dict = self.assign_targets(batch_dict)
                batch_dict['rois'] = targets_dict['rois']
                batch_dict['roi_labels'] = targets_dict['roi_labels']

        # RoI aware pooling, as sparse rows
        pool = self.sparse_pool_fused if self.fused else self.sparse_pool_composed
        part_features, rpn_features, coords, n_valid = pool(batch_dict, targets_dict)
        batch_size_rcnn = batch_dict['rois'].shape[0] * batch_dict['rois'].shape[1]
        size = self.model_cfg.ROI_AWARE_POOL.POOL_SIZE
        sparse_shape = np.array((size, size, size) if isinstance(size, int) else size, dtype=np.int32)
        part_features = spconv.SparseConvTensor(part_features, coords, sparse_shape, batch_size_rcnn, n_valid=n_valid)
        rpn_features = spconv.SparseConvTensor(rpn_features, coords, sparse_shape, batch_size_rcnn, n_valid=n_valid)

        # forward rcnn network
        x_part = self.conv_part(part_features)
        x_rpn = self.conv_rpn(rpn_features)

        merged_feature = torch.cat((x_rpn.features, x_part.features), dim=1)  # (N, C)
        shared_feature = spconv.SparseConvTensor(merged_feature, coords, sparse_shape, batch_size_rcnn, n_valid=n_valid)
        shared_feature = shared_feature.dense().view(batch_size_rcnn, -1, 1)

        shared_feature = self.shared_fc_layer(shared_feature)

        rcnn_cls = self.cls_layers(shared_feature).transpose(1, 2).contiguous().squeeze(dim=1)  # (B, 1 or 2)
        rcnn_reg = self.reg_layers(shared_feature).transpose(1, 2).contiguous().squeeze(dim=1)  # (B, C)

        if not self.training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg
            )
            batch_dict['batch_cls_preds'] = batch_cls_preds
            batch_dict['batch_box_preds'] = batch_box_preds
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg

            self.forward_ret_dict = targets_dict
        return batch_dict
