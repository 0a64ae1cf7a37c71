"""VoxelSetAbstraction (reference pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:124-411): PV-RCNN's keypoint
encoder.  Keypoints are sampled from the cloud, and every keypoint gathers the BEV map (bilinear), the raw points and the
sparse backbone's levels (StackSAModuleMSG each) into one feature row.  Reference constructor signature, config keys and
state_dict keys (SA_layers.*, SA_rawpoints.*, vsa_point_feature_fusion.*).

forward makes no Python loop over frames and no host read.  Departures, recorded in DESIGN.md §6j:
  * keypoints: ONE call of the stack FPS over the frame-contiguous cloud, with the per-frame counts taken on the device.
    The reference samples frame by frame with the batch FPS; the two samplers pick the same points except on exact
    distance ties.  A frame with n < NUM_KEYPOINTS points repeats its n picks cyclically (pick k % n), as the reference.
  * rows of `points` (voxel_coords for voxel_centers) must be grouped by ascending batch index, as the collate leaves
    them; batch_dict['pfe_layout_ok'] is a 0-dim device bool that says whether they were (the results are meaningless
    when it is False).  A frame without points is outside the contract.
  * the BEV interpolation is one gather of four rows per keypoint from the channels-last map for the whole batch, with the
    reference's clamping and its weights from the CLAMPED corners; the gradient to the map has a fixed summation order.
  * PFE.FUSED sets `fused` on every SA module: in eval mode under no_grad their two-layer scales run
    spx.ops.sa_mlp2_max (csrc/sa_mlp.hip).
  * SAMPLE_METHOD SPC, FILTER_NEIGHBOR_WITH_ROI and VectorPoolAggregationModuleMSG (PV-RCNN++) raise NotImplementedError;
    a sparse tensor with n_valid set (static row capacity) is refused by name."""
import torch
import torch.nn as nn

from ....config import AttrDict
from ....ops.pointnet2.pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ....ops.pointnet2.pointnet2_stack import pointnet2_utils as pointnet2_stack_utils

FUSED_DEFAULT = False      # decided by tools/pv_rcnn_bench.py (profiles/pv_rcnn_bench.log)


def bilinear_interpolate_torch(im, x, y):
    """The reference's per-frame function (voxel_set_abstraction.py:11-42): im (H, W, C), x / y (N) -> (N, C).  Kept as
    the statement that interpolate_from_bev_features is tested against."""
    x0 = torch.floor(x).long()
    x1 = x0 + 1
    y0 = torch.floor(y).long()
    y1 = y0 + 1
    x0 = torch.clamp(x0, 0, im.shape[1] - 1)
    x1 = torch.clamp(x1, 0, im.shape[1] - 1)
    y0 = torch.clamp(y0, 0, im.shape[0] - 1)
    y1 = torch.clamp(y1, 0, im.shape[0] - 1)
    Ia, Ib, Ic, Id = im[y0, x0], im[y1, x0], im[y0, x1], im[y1, x1]
    wa = (x1.type_as(x) - x) * (y1.type_as(y) - y)
    wb = (x1.type_as(x) - x) * (y - y0.type_as(y))
    wc = (x - x0.type_as(x)) * (y1.type_as(y) - y)
    wd = (x - x0.type_as(x)) * (y - y0.type_as(y))
    return torch.t((torch.t(Ia) * wa)) + torch.t(torch.t(Ib) * wb) + torch.t(torch.t(Ic) * wc) + torch.t(torch.t(Id) * wd)


def _own_mlps(config):
    """A copy of an SA_LAYER entry whose MLPS lists build_local_aggregation_module may edit in place."""
    return AttrDict(dict(config, MLPS=[list(m) for m in config.MLPS]))


class VoxelSetAbstraction(nn.Module):
    def __init__(self, model_cfg, voxel_size, point_cloud_range, num_bev_features=None,
                 num_rawpoint_features=None, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        if self.model_cfg.SAMPLE_METHOD != 'FPS':
            raise NotImplementedError('VoxelSetAbstraction SAMPLE_METHOD %s: only FPS is ported (SPC, the sectorized '
                                      'proposal-centric sampling of PV-RCNN++, is not)' % self.model_cfg.SAMPLE_METHOD)
        if self.model_cfg.POINT_SOURCE not in ('raw_points', 'voxel_centers'):
            raise NotImplementedError('VoxelSetAbstraction POINT_SOURCE %s' % self.model_cfg.POINT_SOURCE)
        # device copies for the voxel centres: building them per call would be a host-to-device copy inside a captured graph
        self.register_buffer('_voxel_size_f32', torch.tensor(list(voxel_size), dtype=torch.float32), persistent=False)
        self.register_buffer('_range_lo_f32', torch.tensor(list(point_cloud_range[0:3]), dtype=torch.float32),
                             persistent=False)

        SA_cfg = self.model_cfg.SA_LAYER
        for src_name in self.model_cfg.FEATURES_SOURCE:
            if src_name != 'bev' and SA_cfg[src_name].get('FILTER_NEIGHBOR_WITH_ROI', False):
                raise NotImplementedError('VoxelSetAbstraction SA_LAYER.%s.FILTER_NEIGHBOR_WITH_ROI (PV-RCNN++) is not '
                                          'ported' % src_name)

        self.SA_layers = nn.ModuleList()
        self.SA_layer_names = []
        self.downsample_times_map = {}
        c_in = 0
        for src_name in self.model_cfg.FEATURES_SOURCE:
            if src_name in ['bev', 'raw_points']:
                continue
            self.downsample_times_map[src_name] = SA_cfg[src_name].DOWNSAMPLE_FACTOR

            if SA_cfg[src_name].get('INPUT_CHANNELS', None) is None:
                input_channels = SA_cfg[src_name].MLPS[0][0] \
                    if isinstance(SA_cfg[src_name].MLPS[0], list) else SA_cfg[src_name].MLPS[0]
            else:
                input_channels = SA_cfg[src_name]['INPUT_CHANNELS']

            cur_layer, cur_num_c_out = pointnet2_stack_modules.build_local_aggregation_module(
                input_channels=input_channels, config=_own_mlps(SA_cfg[src_name])
            )
            self.SA_layers.append(cur_layer)
            self.SA_layer_names.append(src_name)

            c_in += cur_num_c_out

        if 'bev' in self.model_cfg.FEATURES_SOURCE:
            c_bev = num_bev_features
            c_in += c_bev

        if 'raw_points' in self.model_cfg.FEATURES_SOURCE:
            self.SA_rawpoints, cur_num_c_out = pointnet2_stack_modules.build_local_aggregation_module(
                input_channels=num_rawpoint_features - 3, config=_own_mlps(SA_cfg['raw_points'])
            )

            c_in += cur_num_c_out

        self.vsa_point_feature_fusion = nn.Sequential(
            nn.Linear(c_in, self.model_cfg.NUM_OUTPUT_FEATURES, bias=False),
            nn.BatchNorm1d(self.model_cfg.NUM_OUTPUT_FEATURES),
            nn.ReLU(),
        )
        self.num_point_features = self.model_cfg.NUM_OUTPUT_FEATURES
        self.num_point_features_before_fusion = c_in

        fused = bool(self.model_cfg.get('FUSED', FUSED_DEFAULT))
        for layer in self.sa_modules():
            layer.fused = fused

    def sa_modules(self):
        layers = list(self.SA_layers)
        if hasattr(self, 'SA_rawpoints'):
            layers.append(self.SA_rawpoints)
        return layers

    @staticmethod
    def frame_counts(bs_idxs, batch_size):
        """(batch_size,) int32 rows per frame, counted on the device by comparison (no bincount, no host read)."""
        frames = torch.arange(batch_size, device=bs_idxs.device, dtype=bs_idxs.dtype)
        return (bs_idxs.reshape(-1, 1) == frames.view(1, -1)).sum(dim=0).int()

    def voxel_centers(self, coords, downsample_times):
        """common_utils.get_voxel_centers in its float32 arithmetic, from the cached device constants: coords (N, 3)
        (z, y, x) -> (N, 3) float32 (x, y, z)."""
        xyz_idx = torch.stack((coords[:, 2], coords[:, 1], coords[:, 0]), dim=1)      # no index list: capturable
        return (xyz_idx.float() + 0.5) * (self._voxel_size_f32.float() * downsample_times) + self._range_lo_f32.float()

    def interpolate_from_bev_features(self, keypoints, bev_features, batch_size, bev_stride):
        """keypoints (N1 + N2 + ..., 4), bev_features (B, C, H, W) -> (N1 + N2 + ..., C): the reference's bilinear
        interpolation (clamped corners, weights from the clamped corners) for the whole batch at once."""
        x_idxs = (keypoints[:, 1] - self.point_cloud_range[0]) / self.voxel_size[0]
        y_idxs = (keypoints[:, 2] - self.point_cloud_range[1]) / self.voxel_size[1]
        x = x_idxs / bev_stride
        y = y_idxs / bev_stride
        b, c, h, w = bev_features.shape
        x0 = torch.floor(x).long()
        x1 = x0 + 1
        y0 = torch.floor(y).long()
        y1 = y0 + 1
        x0, x1 = torch.clamp(x0, 0, w - 1), torch.clamp(x1, 0, w - 1)
        y0, y1 = torch.clamp(y0, 0, h - 1), torch.clamp(y1, 0, h - 1)
        wa = (x1.type_as(x) - x) * (y1.type_as(y) - y)
        wb = (x1.type_as(x) - x) * (y - y0.type_as(y))
        wc = (x - x0.type_as(x)) * (y1.type_as(y) - y)
        wd = (x - x0.type_as(x)) * (y - y0.type_as(y))
        base = keypoints[:, 0].long().clamp(0, b - 1) * (h * w)
        rows = torch.stack((base + y0 * w + x0, base + y1 * w + x0, base + y0 * w + x1, base + y1 * w + x1), dim=1)
        table = bev_features.permute(0, 2, 3, 1).reshape(b * h * w, c)            # a view of a channels-last map
        n_rows = torch.full((1,), b * h * w, dtype=torch.int32, device=table.device)
        n_idx = torch.full((1,), rows.shape[0], dtype=torch.int32, device=table.device)
        corners = pointnet2_stack_utils.grouping_operation(table.contiguous(), n_rows, rows.int().contiguous(), n_idx)
        ia, ib, ic, id_ = corners[:, :, 0], corners[:, :, 1], corners[:, :, 2], corners[:, :, 3]      # (N, C) each
        return ia * wa[:, None] + ib * wb[:, None] + ic * wc[:, None] + id_ * wd[:, None]

    def get_sampled_points(self, batch_dict):
        """-> keypoints (B * NUM_KEYPOINTS, 4) [bs_idx, x, y, z], frame after frame; writes batch_dict['pfe_layout_ok']."""
        batch_size = batch_dict['batch_size']
        num = self.model_cfg.NUM_KEYPOINTS
        if self.model_cfg.POINT_SOURCE == 'raw_points':
            src_points = batch_dict['points'][:, 1:4]
            batch_indices = batch_dict['points'][:, 0]
        else:
            src_points = self.voxel_centers(batch_dict['voxel_coords'][:, 1:4], 1)
            batch_indices = batch_dict['voxel_coords'][:, 0]
        src_points = src_points.contiguous()
        batch_dict['pfe_layout_ok'] = (batch_indices[1:] >= batch_indices[:-1]).all()
        cnt = self.frame_counts(batch_indices, batch_size)
        npoint = torch.full((batch_size,), num, dtype=torch.int32, device=cnt.device)
        picks = pointnet2_stack_utils.stack_farthest_point_sample(src_points, cnt, npoint, total=batch_size * num)
        picks = picks.long().view(batch_size, num)
        # a frame of n < NUM_KEYPOINTS points: its first n picks, repeated (pick k % n); k % n = k where n >= NUM_KEYPOINTS
        k = torch.arange(num, device=picks.device).view(1, -1) % cnt.long().clamp(min=1).view(-1, 1)
        picks = torch.gather(picks, 1, k).view(-1)
        batch_idx = torch.arange(batch_size, device=picks.device).view(-1, 1).expand(-1, num).reshape(-1, 1)
        return torch.cat((batch_idx.to(src_points.dtype), src_points[picks]), dim=1)

    @staticmethod
    def aggregate_keypoint_features_from_one_source(
            batch_size, aggregate_func, xyz, xyz_features, xyz_bs_idxs, new_xyz, new_xyz_batch_cnt,
            filter_neighbors_with_roi=False, radius_of_neighbor=None, num_max_points_of_part=200000, rois=None
    ):
        """xyz (N, 3), xyz_features (N, C) or None, xyz_bs_idxs (N) ascending, new_xyz (M, 3) -> (M, C_out)."""
        if filter_neighbors_with_roi:
            raise NotImplementedError('VoxelSetAbstraction FILTER_NEIGHBOR_WITH_ROI (PV-RCNN++) is not ported')
        xyz_batch_cnt = VoxelSetAbstraction.frame_counts(xyz_bs_idxs, batch_size)
        pooled_points, pooled_features = aggregate_func(
            xyz=xyz.contiguous(),
            xyz_batch_cnt=xyz_batch_cnt,
            new_xyz=new_xyz,
            new_xyz_batch_cnt=new_xyz_batch_cnt,
            features=None if xyz_features is None else xyz_features.contiguous(),
        )
        return pooled_features

    def forward(self, batch_dict):
        """points (N, 1 + 3 + C), spatial_features (B, C, H, W), multi_scale_3d_features -> point_features (B * K, C),
        point_features_before_fusion, point_coords (B * K, 4), pfe_layout_ok."""
        keypoints = self.get_sampled_points(batch_dict)
        batch_size = batch_dict['batch_size']

        point_features_list = []
        if 'bev' in self.model_cfg.FEATURES_SOURCE:
            point_bev_features = self.interpolate_from_bev_features(
                keypoints, batch_dict['spatial_features'], batch_size,
                bev_stride=batch_dict['spatial_features_stride']
            )
            point_features_list.append(point_bev_features)

        new_xyz = keypoints[:, 1:4].contiguous()
        new_xyz_batch_cnt = torch.full((batch_size,), self.model_cfg.NUM_KEYPOINTS, dtype=torch.int32,
                                       device=new_xyz.device)

        if 'raw_points' in self.model_cfg.FEATURES_SOURCE:
            raw_points = batch_dict['points']
            pooled_features = self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_rawpoints,
                xyz=raw_points[:, 1:4],
                xyz_features=raw_points[:, 4:].contiguous() if raw_points.shape[1] > 4 else None,
                xyz_bs_idxs=raw_points[:, 0],
                new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt,
            )
            point_features_list.append(pooled_features)

        for k, src_name in enumerate(self.SA_layer_names):
            cur_sp_tensor = batch_dict['multi_scale_3d_features'][src_name]
            if getattr(cur_sp_tensor, 'n_valid', None) is not None:
                raise NotImplementedError('VoxelSetAbstraction does not support static-capacity sparse tensors (%s has '
                                          'n_valid set): the dead rows would enter the ball queries' % src_name)
            cur_coords = cur_sp_tensor.indices
            cur_features = cur_sp_tensor.features.contiguous()
            xyz = self.voxel_centers(cur_coords[:, 1:4], self.downsample_times_map[src_name])
            pooled_features = self.aggregate_keypoint_features_from_one_source(
                batch_size=batch_size, aggregate_func=self.SA_layers[k],
                xyz=xyz.contiguous(), xyz_features=cur_features, xyz_bs_idxs=cur_coords[:, 0],
                new_xyz=new_xyz, new_xyz_batch_cnt=new_xyz_batch_cnt,
            )
            point_features_list.append(pooled_features)

        point_features = torch.cat(point_features_list, dim=-1)

        batch_dict['point_features_before_fusion'] = point_features.view(-1, point_features.shape[-1])
        point_features = self.vsa_point_feature_fusion(point_features.view(-1, point_features.shape[-1]))

        batch_dict['point_features'] = point_features  # (BxN, C)
        batch_dict['point_coords'] = keypoints  # (BxN, 4)
        return batch_dict
