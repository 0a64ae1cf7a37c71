"""VoxelRCNNHead (reference pcdet/models/roi_heads/voxelrcnn_head.py:8-262): a dense G x G x G grid per RoI pools the
backbone's multi-scale voxel features through NeighborVoxelSAModuleMSG, shared FC layers and a class / box branch refine
every RoI.  Reference constructor signature, submodule tree (state_dict keys) and init_weights.

Departures, recorded in DESIGN.md §6i:
  * the fork's pool module returns (features, density); the reference head calls .view on that tuple and cannot run.
    Element 0 is taken.
  * batch_idx and the per-frame voxel counts are built without Python loops (comparisons on the device, no host read); the
    fused pooling path does not use the counts at all.
  * ROI_GRID_POOL.FUSED (default True, decided by tools/voxel_rcnn_bench.py) sets `fused` on the pool layers: max_pool on
    device tensors runs spx.ops.voxel_pool_max (csrc/voxel_pool.hip) instead of the torch composition.
  * a sparse tensor with n_valid set (static row capacity) raises NotImplementedError: mlps_in's BatchNorm1d would count
    the dead rows.
  * every MLPS entry must be [c_mid, c_out] style lists whose last value is the layer's output width: the fork's module
    reads entries 0 and 1 of [c_in] + entry only, so an entry of another length would make c_out disagree.  Asserted.
  * voxel_query_fn: an injectable stand-in for voxel_query_utils.voxel_query (as ProposalTargetLayer.iou3d_fn), so the
    head runs in float64 on CPU tensors in the tests.
forward, assign_targets, get_loss and the backward make no host read; tb_dict holds 0-dim tensors (RoIHeadTemplate)."""
import contextlib

import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_stack import voxel_pool_modules as voxelpool_stack_modules
from ...ops.pointnet2.pointnet2_stack import voxel_query_utils
from ...utils import common_utils
from .roi_head_template import RoIHeadTemplate


class VoxelRCNNHead(RoIHeadTemplate):
    voxel_query_fn = None       # staticmethod-style hook: (max_range, radius, nsample, xyz, new_xyz, new_coords, table)

    def __init__(self, backbone_channels, model_cfg, point_cloud_range, voxel_size, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        self.pool_cfg = model_cfg.ROI_GRID_POOL
        LAYER_cfg = self.pool_cfg.POOL_LAYERS
        self.point_cloud_range = point_cloud_range
        self.voxel_size = voxel_size
        # device copies for the voxel centres: building them per call would be a host-to-device copy inside a captured graph
        self.register_buffer('_voxel_size_f32', torch.tensor(list(voxel_size), dtype=torch.float32), persistent=False)
        self.register_buffer('_range_lo_f32', torch.tensor(list(point_cloud_range[0:3]), dtype=torch.float32),
                             persistent=False)

        c_out = 0
        self.roi_grid_pool_layers = nn.ModuleList()
        for src_name in self.pool_cfg.FEATURES_SOURCE:
            mlps = [[backbone_channels[src_name]] + list(m) for m in LAYER_cfg[src_name].MLPS]
            for m in mlps:
                # the fork's module builds Conv1d(m[0], m[1]): its output width is m[1], which c_out below takes as m[-1]
                assert len(m) >= 2 and m[1] == m[-1], 'MLPS entry %s: the pool module uses entries 0 and 1 only' % (m[1:],)
            pool_layer = voxelpool_stack_modules.NeighborVoxelSAModuleMSG(
                query_ranges=LAYER_cfg[src_name].QUERY_RANGES,
                nsamples=LAYER_cfg[src_name].NSAMPLE,
                radii=LAYER_cfg[src_name].POOL_RADIUS,
                mlps=mlps,
                pool_method=LAYER_cfg[src_name].POOL_METHOD,
            )
            self.roi_grid_pool_layers.append(pool_layer)
            c_out += sum([x[-1] for x in mlps])

        GRID_SIZE = self.model_cfg.ROI_GRID_POOL.GRID_SIZE
        pre_channel = GRID_SIZE * GRID_SIZE * GRID_SIZE * c_out

        shared_fc_list = []
        for k in range(0, self.model_cfg.SHARED_FC.__len__()):
            shared_fc_list.extend([nn.Linear(pre_channel, self.model_cfg.SHARED_FC[k], bias=False),
                                   nn.BatchNorm1d(self.model_cfg.SHARED_FC[k]), nn.ReLU(inplace=True)])
            pre_channel = self.model_cfg.SHARED_FC[k]
            if k != self.model_cfg.SHARED_FC.__len__() - 1 and self.model_cfg.DP_RATIO > 0:
                shared_fc_list.append(nn.Dropout(self.model_cfg.DP_RATIO))
        self.shared_fc_layer = nn.Sequential(*shared_fc_list)

        cls_fc_list = []
        for k in range(0, self.model_cfg.CLS_FC.__len__()):
            cls_fc_list.extend([nn.Linear(pre_channel, self.model_cfg.CLS_FC[k], bias=False),
                                nn.BatchNorm1d(self.model_cfg.CLS_FC[k]), nn.ReLU()])
            pre_channel = self.model_cfg.CLS_FC[k]
            if k != self.model_cfg.CLS_FC.__len__() - 1 and self.model_cfg.DP_RATIO > 0:
                cls_fc_list.append(nn.Dropout(self.model_cfg.DP_RATIO))
        self.cls_fc_layers = nn.Sequential(*cls_fc_list)
        self.cls_pred_layer = nn.Linear(pre_channel, self.num_class, bias=True)

        # as in the reference, the box branch starts from the class branch's last width
        reg_fc_list = []
        for k in range(0, self.model_cfg.REG_FC.__len__()):
            reg_fc_list.extend([nn.Linear(pre_channel, self.model_cfg.REG_FC[k], bias=False),
                                nn.BatchNorm1d(self.model_cfg.REG_FC[k]), nn.ReLU()])
            pre_channel = self.model_cfg.REG_FC[k]
            if k != self.model_cfg.REG_FC.__len__() - 1 and self.model_cfg.DP_RATIO > 0:
                reg_fc_list.append(nn.Dropout(self.model_cfg.DP_RATIO))
        self.reg_fc_layers = nn.Sequential(*reg_fc_list)
        self.reg_pred_layer = nn.Linear(pre_channel, self.box_coder.code_size * self.num_class, bias=True)

        self.init_weights()

    def init_weights(self):
        init_func = nn.init.xavier_normal_
        for module_list in [self.shared_fc_layer, self.cls_fc_layers, self.reg_fc_layers]:
            for m in module_list.modules():
                if isinstance(m, nn.Linear):
                    init_func(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.cls_pred_layer.weight, 0, 0.01)
        nn.init.constant_(self.cls_pred_layer.bias, 0)
        nn.init.normal_(self.reg_pred_layer.weight, mean=0, std=0.001)
        nn.init.constant_(self.reg_pred_layer.bias, 0)

    @contextlib.contextmanager
    def _voxel_query(self):
        """voxel_query_utils.voxel_query is voxel_query_fn for the duration, when one is injected."""
        fn = self.voxel_query_fn      # set on an instance, or on the class wrapped in staticmethod
        if fn is None:
            yield
            return
        real = voxel_query_utils.voxel_query
        voxel_query_utils.voxel_query = fn
        try:
            yield
        finally:
            voxel_query_utils.voxel_query = real

    def roi_grid_pool(self, batch_dict):
        """rois (B, N, 7 + C), multi_scale_3d_features[src] sparse tensors -> (B * N, G^3, sum of the levels' channels)."""
        rois = batch_dict['rois']
        batch_size = batch_dict['batch_size']
        with_vf_transform = batch_dict.get('with_voxel_feature_transform', False)
        grid = self.pool_cfg.GRID_SIZE
        fused = bool(self.pool_cfg.get('FUSED', True))

        roi_grid_xyz, _ = self.get_global_grid_points_of_roi(rois, grid_size=grid)      # (B x N, G^3, 3)
        roi_grid_xyz = roi_grid_xyz.view(batch_size, -1, 3)                             # (B, N x G^3, 3)

        # voxel coordinates of the grid points: float floor division, as the reference
        roi_grid_coords_x = (roi_grid_xyz[:, :, 0:1] - self.point_cloud_range[0]) // self.voxel_size[0]
        roi_grid_coords_y = (roi_grid_xyz[:, :, 1:2] - self.point_cloud_range[1]) // self.voxel_size[1]
        roi_grid_coords_z = (roi_grid_xyz[:, :, 2:3] - self.point_cloud_range[2]) // self.voxel_size[2]
        roi_grid_coords = torch.cat([roi_grid_coords_x, roi_grid_coords_y, roi_grid_coords_z], dim=-1)

        per_frame = roi_grid_coords.shape[1]
        batch_idx = torch.arange(batch_size, device=rois.device, dtype=rois.dtype).view(-1, 1, 1).expand(-1, per_frame, 1)
        roi_grid_batch_cnt = torch.full((batch_size,), per_frame, dtype=torch.int32, device=rois.device)

        pooled_features_list = []
        with self._voxel_query():
            for k, src_name in enumerate(self.pool_cfg.FEATURES_SOURCE):
                pool_layer = self.roi_grid_pool_layers[k]
                pool_layer.fused = fused
                cur_stride = batch_dict['multi_scale_3d_strides'][src_name]
                key = 'multi_scale_3d_features_post' if with_vf_transform else 'multi_scale_3d_features'
                cur_sp_tensors = batch_dict[key][src_name]
                if getattr(cur_sp_tensors, 'n_valid', None) is not None:
                    raise NotImplementedError('VoxelRCNNHead does not support static-capacity sparse tensors (%s has n_valid '
                                              'set): mlps_in BatchNorm1d would count the dead rows' % src_name)

                cur_coords = cur_sp_tensors.indices
                # common_utils.get_voxel_centers in its float32 arithmetic, from the cached device constants
                xyz_idx = torch.stack((cur_coords[:, 3], cur_coords[:, 2], cur_coords[:, 1]), dim=1)     # no index list: capturable
                cur_voxel_xyz = (xyz_idx.float() + 0.5) * (self._voxel_size_f32.float() * cur_stride) \
                    + self._range_lo_f32.float()
                frames = torch.arange(batch_size, device=cur_coords.device, dtype=cur_coords.dtype)
                cur_voxel_xyz_batch_cnt = (cur_coords[:, 0:1] == frames.view(1, -1)).sum(dim=0).int()
                v2p_ind_tensor = common_utils.generate_voxel2pinds(cur_sp_tensors)
                # the grid coordinates at this scale, (b, x, y, z)
                cur_roi_grid_coords = roi_grid_coords // cur_stride
                cur_roi_grid_coords = torch.cat([batch_idx, cur_roi_grid_coords], dim=-1).int()
                pooled_features = pool_layer(
                    xyz=cur_voxel_xyz.contiguous(),
                    xyz_batch_cnt=cur_voxel_xyz_batch_cnt,
                    new_xyz=roi_grid_xyz.contiguous().view(-1, 3),
                    new_xyz_batch_cnt=roi_grid_batch_cnt,
                    new_coords=cur_roi_grid_coords.contiguous().view(-1, 4),
                    features=cur_sp_tensors.features.contiguous(),
                    voxel2point_indices=v2p_ind_tensor
                )[0]                                                                    # (features, density)
                pooled_features = pooled_features.view(-1, grid ** 3, pooled_features.shape[-1])      # (B x N, G^3, C)
                pooled_features_list.append(pooled_features)
        return torch.cat(pooled_features_list, dim=-1)

    def get_global_grid_points_of_roi(self, rois, grid_size):
        rois = rois.view(-1, rois.shape[-1])
        batch_size_rcnn = rois.shape[0]
        local_roi_grid_points = self.get_dense_grid_points(rois, batch_size_rcnn, grid_size)      # (B, G^3, 3)
        global_roi_grid_points = common_utils.rotate_points_along_z(local_roi_grid_points.clone(), rois[:, 6]).squeeze(dim=1)
        global_center = rois[:, 0:3].clone()
        global_roi_grid_points = global_roi_grid_points + global_center.unsqueeze(dim=1)
        return global_roi_grid_points, local_roi_grid_points

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        """(x_idx, y_idx, z_idx) of every cell in row-major order (the reference's ones(...).nonzero(), without its host
        read), scaled into the RoI's local box."""
        r = torch.arange(grid_size, device=rois.device)
        dense_idx = torch.stack(torch.meshgrid(r, r, r, indexing='ij'), dim=-1).view(1, -1, 3).float()      # float32, as there
        local_roi_size = rois.view(batch_size_rcnn, -1)[:, 3:6]
        return (dense_idx + 0.5) / grid_size * local_roi_size.unsqueeze(dim=1) - (local_roi_size.unsqueeze(dim=1) / 2)

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(
            batch_dict, nms_config=self.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']

        pooled_features = self.roi_grid_pool(batch_dict)                 # (B x N, G^3, C)
        pooled_features = pooled_features.reshape(pooled_features.size(0), -1)
        shared_features = self.shared_fc_layer(pooled_features)
        rcnn_cls = self.cls_pred_layer(self.cls_fc_layers(shared_features))
        rcnn_reg = self.reg_pred_layer(self.reg_fc_layers(shared_features))

        if not self.training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['batch_cls_preds'] = batch_cls_preds
            batch_dict['batch_box_preds'] = batch_box_preds
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
