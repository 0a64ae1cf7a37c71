"""VoxelPointNet2FSMSGDistillation: the point backbone of the fork's fast_cpc model (reference
pcdet/models/backbones_3d/pointnet2_backbone.py:619-923).

A teacher stack of VoxelPointnetSAModuleFSMSGDistillation layers (SA_CONFIG) runs under no_grad; a student layer
(S_SA_CONFIG, its layers from 1 on) runs with grad on the teacher's layer-0 output.  Same constructor, submodules and
batch_dict keys as the reference.

Static mode (batch_dict['static_caps'] is not None, the key of the SECOND path; eval and no_grad only): the forward
reads nothing back from the device, so it can be captured in a graph.  Every frame must hold points.shape[0] /
batch_size points.  What the backbone exposes per voxel (s_last_sp_tensor, s_last_centroids,
s_last_centroid_voxel_idxs, s_last_scores, s_statistic_feature, point_coords_list[0], point_scores_list) then has
B * NPOINT_LIST[0] rows of which only the first batch_dict['voxel_num_valid'] (device int64[1]) are live; the dead rows
hold whatever the buffers held.  batch_dict['static_flags'] holds device booleans, in the manner of
post_processing_static's layout_ok: 'layout_ok' (the frame index column is 0..B-1, each repeated equally often, in
order) and 'in_range' (every sampled point fell into a voxel of the grid).  Where one of them is False the results of
the batch are meaningless; nothing is raised, the caller reads the flags when convenient.
"""
import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_batch import pointnet2_modules


def _sa_layer(sa_cfg, k, channel_in, prev_spconv_mlps, aggregation_mlps, confidence_mlps, use_xyz, dilated_group,
              skip_connection, weight_gamma, voxel_size, grid_size, point_cloud_range):
    """Layer k of an SA stack -> (module, channel_out, spconv_mlps), the reference's channel bookkeeping."""
    mlps = sa_cfg.MLPS[k].copy()
    spconv_mlps = sa_cfg.SPCONV_MLPS_PRE[k].copy()
    channel_out = 0
    if k <= 2:
        for idx in range(len(mlps)):
            mlps[idx] = [channel_in] + mlps[idx]
            channel_out += mlps[idx][-1]
    else:
        channel_out = prev_spconv_mlps[-1]
    if skip_connection:
        channel_out += channel_in
    if aggregation_mlps and aggregation_mlps[k]:
        aggregation_mlp = aggregation_mlps[k].copy()
        if len(aggregation_mlp) == 0:
            aggregation_mlp = None
        else:
            channel_out = aggregation_mlp[-1]
    else:
        aggregation_mlp = None
    spconv_mlps = ([channel_out] if k == 0 else [prev_spconv_mlps[-1]]) + spconv_mlps
    if confidence_mlps and confidence_mlps[k]:
        confidence_mlp = confidence_mlps[k].copy()
        if len(confidence_mlp) == 0:
            confidence_mlp = None
    else:
        confidence_mlp = None
    module = pointnet2_modules.VoxelPointnetSAModuleFSMSGDistillation(
        npoint_list=sa_cfg.NPOINT_LIST[k],
        sample_range_list=sa_cfg.SAMPLE_RANGE_LIST[k],
        sample_method_list=sa_cfg.SAMPLE_METHOD_LIST[k],
        sp_stride=sa_cfg.SPARSE_TENSOR_STRIDE[k],
        query_range=sa_cfg.QUERY_RANGE[k],
        stride=sa_cfg.STRIDE[k],
        radii=sa_cfg.RADIUS[k],
        nsamples=sa_cfg.NSAMPLE[k],
        mlps=mlps,
        spconv_mlps=spconv_mlps,
        pool_method=sa_cfg.POOL_METHOD[k],
        use_xyz=use_xyz,
        dilated_radius_group=dilated_group,
        skip_connection=skip_connection,
        weight_gamma=weight_gamma,
        aggregation_mlp=aggregation_mlp,
        confidence_mlp=confidence_mlp,
        sa_layer_idx=k,
        voxel_size=voxel_size,
        grid_size=grid_size,
        point_cloud_range=point_cloud_range,
    )
    return module, channel_out, spconv_mlps


class VoxelPointNet2FSMSGDistillation(nn.Module):
    def __init__(self, model_cfg, input_channels, grid_size, voxel_size, point_cloud_range, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.grid_size = grid_size
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range

        sa_cfg = self.model_cfg.SA_CONFIG
        use_xyz = sa_cfg.get('USE_XYZ', True)
        dilated_group = sa_cfg.get('DILATED_RADIUS_GROUP', False)
        skip_connection = sa_cfg.get('SKIP_CONNECTION', False)
        weight_gamma = sa_cfg.get('WEIGHT_GAMMA', 1.0)
        common = dict(use_xyz=use_xyz, dilated_group=dilated_group, skip_connection=skip_connection,
                      weight_gamma=weight_gamma, voxel_size=voxel_size, grid_size=grid_size,
                      point_cloud_range=point_cloud_range)

        # teacher
        self.SA_modules = nn.ModuleList()
        self.aggregation_mlps = sa_cfg.get('AGGREGATION_MLPS', None)
        self.confidence_mlps = sa_cfg.get('CONFIDENCE_MLPS', None)
        self.num_points_each_layer = []
        channel_in = input_channels - 3
        last_spconv_mlps = []
        for k in range(len(sa_cfg.NPOINT_LIST)):
            module, channel_out, last_spconv_mlps = _sa_layer(sa_cfg, k, channel_in, last_spconv_mlps,
                                                              self.aggregation_mlps, self.confidence_mlps, **common)
            self.SA_modules.append(module)
            self.num_points_each_layer.append(sum(sa_cfg.NPOINT_LIST[k]))
            channel_in = channel_out
        self.num_point_features = channel_out

        self.switch = True
        self.num_class = 3

        # student: layers 1.. on the teacher's layer-0 output
        s_cfg = self.model_cfg.S_SA_CONFIG
        self.S_SA_modules = nn.ModuleList()
        self.s_aggregation_mlps = s_cfg.get('AGGREGATION_MLPS', None)
        self.s_confidence_mlps = s_cfg.get('CONFIDENCE_MLPS', None)
        self.s_num_points_each_layer = []
        channel_in = last_spconv_mlps[0]
        s_last_spconv_mlps = [last_spconv_mlps[0]]
        for k in range(1, len(s_cfg.NPOINT_LIST)):
            module, channel_out, s_last_spconv_mlps = _sa_layer(s_cfg, k, channel_in, s_last_spconv_mlps,
                                                                self.s_aggregation_mlps, self.s_confidence_mlps, **common)
            self.S_SA_modules.append(module)
            self.s_num_points_each_layer.append(sum(s_cfg.NPOINT_LIST[k]))
            channel_in = channel_out
        self.FP_modules = None
        self.s_num_point_features = channel_out

    def break_up_pc(self, pc):
        batch_idx = pc[:, 0]
        xyz = pc[:, 1:4].contiguous()
        features = (pc[:, 4:].contiguous() if pc.size(-1) > 4 else None)
        return batch_idx, xyz, features

    @staticmethod
    def _run(module, l, i, static=False):
        return module(l['xyz'][i], l['features'][i], scores=l['scores'][i], part_scores=l['part_scores'][i],
                      sp_tensor=l['sp_tensor'][i], centroids=l['centroids'][i],
                      centroid_voxel_idxs=l['centroid_voxel_idxs'][i], unique_idxs=l['unique_idxs'][i], static=static)

    def forward(self, batch_dict):
        """
        Args:
            batch_dict:
                batch_size: int
                points: (num_points, 4 + C), [batch_idx, x, y, z, ...], the same number of points in every frame
        Returns:
            batch_dict with last_* (training), s_last_*, point_coords_list, point_scores_list, point_part_scores_list,
            point_features / point_coords / point_scores / statistic_feature (training) and their s_ counterparts
        """
        batch_size = batch_dict['batch_size']
        points = batch_dict['points']
        batch_idx, xyz, features = self.break_up_pc(points)
        static = batch_dict.get('static_caps', None) is not None
        if static:
            if self.training or torch.is_grad_enabled():
                raise RuntimeError('VoxelPointNet2FSMSGDistillation: static_caps (the static-capacity path) is inference '
                                   'only: it needs model.eval() and torch.no_grad()')
            if batch_size < 1 or points.shape[0] == 0 or points.shape[0] % batch_size:
                raise ValueError('VoxelPointNet2FSMSGDistillation: static mode needs %d equal, non-empty frames, got %d '
                                 'points' % (batch_size, points.shape[0]))
            frame = torch.arange(batch_size, device=points.device, dtype=batch_idx.dtype).view(-1, 1)
            layout_ok = (batch_idx.view(batch_size, -1) == frame).all()
        else:
            xyz_batch_cnt = torch.bincount(batch_idx.long(), minlength=batch_size)[:batch_size]
            assert xyz_batch_cnt.min() == xyz_batch_cnt.max()
        xyz = xyz.view(batch_size, -1, 3).contiguous()
        features = features.view(batch_size, -1, features.shape[-1]) if features is not None else None
        features = features.permute(0, 2, 1).contiguous() if features is not None else None

        batch_idx = batch_idx.view(batch_size, -1).float()
        names = ('xyz', 'features', 'scores', 'sp_tensor', 'centroids', 'centroid_voxel_idxs', 'unique_idxs',
                 'part_scores')
        l = {n: [None] for n in names}
        l['xyz'], l['features'] = [xyz], [features]

        with torch.no_grad():
            aggregation_num = len(self.SA_modules) if self.training else len(self.SA_modules) - 1
            for i in range(aggregation_num):
                for n, v in zip(names, self._run(self.SA_modules[i], l, i, static=static)):
                    l[n].append(v)

        # student, on the teacher's layer-0 output
        for n, v in zip(names, self._run(self.S_SA_modules[0], l, 1)):
            l[n].append(v)

        if self.training:
            batch_dict['last_sp_tensor'] = l['sp_tensor'][-2]
            batch_dict['last_centroids'] = l['centroids'][-2]
            batch_dict['last_features'] = l['features'][-2]
            batch_dict['last_centroid_voxel_idxs'] = l['centroid_voxel_idxs'][-2]
            batch_dict['last_scores'] = l['scores'][-2]
            batch_dict['last_unique_idxs'] = l['unique_idxs'][-2]
        batch_dict['s_last_sp_tensor'] = l['sp_tensor'][-1]
        batch_dict['s_last_centroids'] = l['centroids'][-1]
        batch_dict['s_last_features'] = l['features'][-1]
        batch_dict['s_last_centroid_voxel_idxs'] = l['centroid_voxel_idxs'][-1]
        batch_dict['s_last_scores'] = l['scores'][-1]
        batch_dict['s_last_unique_idxs'] = l['unique_idxs'][-1]

        # for the confidence loss
        l_scores_flatten, l_part_scores_flatten = [], []
        for s in l['scores'][1:]:
            if s is None:
                l_scores_flatten.append(None)
                l_part_scores_flatten.append(None)
            else:
                l_scores_flatten.append(s.reshape(-1, self.num_class))
        batch_dict['point_coords_list'] = list(l['centroids'][1:])
        batch_dict['point_scores_list'] = l_scores_flatten
        batch_dict['point_part_scores_list'] = l_part_scores_flatten

        if self.training:
            point_features = l['features'][-2].permute(0, 2, 1).contiguous()  # (B, N, C)
            batch_dict['point_features'] = point_features.view(-1, point_features.shape[-2])
            batch_dict['point_coords'] = torch.cat((
                batch_idx[:, :l['xyz'][-2].size(1)].reshape(-1, 1).float(), l['xyz'][-2].view(-1, 3)), dim=1)
            batch_dict['point_scores'] = l['scores'][-2]
            batch_dict['statistic_feature'] = l['sp_tensor'][-2].features

        s_point_features = l['features'][-1].permute(0, 2, 1).contiguous()  # (B, N, C)
        batch_dict['s_point_features'] = s_point_features.view(-1, s_point_features.shape[-1])
        batch_dict['s_point_coords'] = torch.cat((
            batch_idx[:, :l['xyz'][-1].size(1)].reshape(-1, 1).float(), l['xyz'][-1].view(-1, 3)), dim=1)
        batch_dict['s_point_scores'] = l['scores'][-1]
        batch_dict['s_statistic_feature'] = l['sp_tensor'][-1].features
        if static:
            batch_dict['voxel_num_valid'] = l['sp_tensor'][-1].n_valid
            batch_dict['static_flags'] = {'layout_ok': layout_ok, 'in_range': (l['unique_idxs'][1] >= 0).all()}
        return batch_dict
