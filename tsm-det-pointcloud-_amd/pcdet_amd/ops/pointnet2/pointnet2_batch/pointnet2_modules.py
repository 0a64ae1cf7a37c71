"""The fork's voxel-point set-abstraction modules (reference pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py:
_VoxelPointnetSAModuleFSDistillationBase, VoxelPointnetSAModuleFSMSGDistillation, VoxelPointnetSAModuleFSDistillation).

Same constructor keywords, submodule tree (so the same state_dict keys and shapes), forward semantics and 8-tuple return
as the reference.  What differs is how each grouper's first 1x1 conv is evaluated: the reference materialises the
grouped tensor (B, 3 + C, npoint, nsample) and runs point_mlps[i][0] (and pos_mlps[i][0]) on it; here those convs go
through pointnet2_utils.group_project (include/spx.h §13), which gathers, subtracts the centre, masks empty balls and
writes the conv output in NCHW without building the grouped tensor.  The conv modules still hold the weights; the rest
of each MLP (BatchNorm2d, ReLU, ...) runs unchanged on the result.

Deliberate differences: the device of the voxel-size / range tensors follows the inputs (the reference hard-codes
'cuda:0'), and torch.arange replaces the deprecated torch.range (same values).

Static mode (forward(..., static=True) at layer 0; later layers follow sp_tensor.n_valid): inference with no host read,
so that the whole forward can be captured in a graph.  The voxel tensors keep a row CAPACITY (B * npoint of layer 0) and
the live row count stays on the device in sp_tensor.n_valid: of scores, centroids, centroid_voxel_idxs and
sp_tensor.features / .indices only the first n_valid rows are live, the rest hold whatever the buffers held.  The cell
table and the sparse update's per-voxel mean come from spx.ops.voxel_table_build / voxel_rows_mean (include/spx.h §19),
which never read a dead row; row-local torch modules (confidence_mlp, the ori_scores product) compute on dead rows too,
and nothing reduces over them.  A sampled point outside the grid gets voxel row -1 in unique_idxs (the backbone reports
it in static_flags); the eager path would have failed on it.
"""
from functools import partial
from typing import List

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import pointnet2_utils
from ..pointnet2_stack import voxel_query_utils
from ....utils import common_utils, voxel_aggregation_utils
from ....utils.spconv_utils import replace_feature, spconv
from spx import ops as spx_ops

__all__ = ["VoxelPointnetSAModuleFSMSGDistillation", "VoxelPointnetSAModuleFSDistillation"]


_stage_hook = None    # callable(name) or None: a profiler's marker at the END of each stage (tools/point_head_bench.py)


def _stage(name):
    if _stage_hook is not None:
        _stage_hook(name)


def _conv_weight(conv):
    """nn.Conv2d(k=1) weight (Cout, Cin, 1, 1) -> (Cout, Cin) view."""
    return conv.weight.view(conv.weight.shape[0], conv.weight.shape[1])


class _VoxelPointnetSAModuleFSDistillationBase(nn.Module):

    def __init__(self):
        super().__init__()
        self.groupers = None
        self.mlps = None
        self.spconv_mlps = None
        self.npoint_list = []
        self.sample_range_list = [[0, -1]]
        self.sample_method_list = ['d-fps']
        self.sp_stride = None
        self.radii = []
        self.point_mlps = None

        self.pool_method = 'max_pool'
        self.dilated_radius_group = False
        self.weight_gamma = 1.0
        self.skip_connection = False

        self.aggregation_mlp = None
        self.confidence_mlp = None
        self.voxel_size = []
        self.grid_size = []
        self.point_cloud_range = []

    def _grid_tensors(self, device):
        """(voxel_size, point_cloud_range) as float32 tensors on `device`, built once per device and setting: the
        host-to-device copy behind torch.tensor(list) cannot be captured in a graph."""
        key = (device, tuple(float(v) for v in self.voxel_size), tuple(float(v) for v in self.point_cloud_range))
        cache = self.__dict__.setdefault('_grid_cache', {})
        if key not in cache:
            cache[key] = (torch.tensor(self.voxel_size, device=device).float(),
                          torch.tensor(self.point_cloud_range, device=device).float())
        return cache[key]

    # ------------------------------------------------------------------------------------------- sampling
    def _sample(self, xyz, features, scores, batch_size):
        sample_idx_list = []
        for i in range(len(self.sample_method_list)):
            lo, hi = self.sample_range_list[i]
            xyz_slice = xyz[:, lo:hi, :].contiguous()
            method = self.sample_method_list[i]
            if method == 'd-fps':
                if self.sa_layer_idx == 0:
                    sample_idx = pointnet2_utils.furthest_point_sample(xyz_slice, self.npoint_list[i])
                else:
                    sample_idx = torch.arange(0, self.npoint_list[i], device=xyz_slice.device, dtype=torch.int32)
                    sample_idx = sample_idx.unsqueeze(0).repeat(len(xyz_slice), 1)
            elif method == 'f-fps':
                features_slice = features[:, :, lo:hi]
                dist_matrix = pointnet2_utils.calc_dist_matrix_for_sampling(xyz_slice, features_slice.permute(0, 2, 1),
                                                                            self.weight_gamma)
                sample_idx = pointnet2_utils.furthest_point_sample_matrix(dist_matrix, self.npoint_list[i])
            elif method == 's-fps':
                assert scores is not None
                scores_slice = scores[:, lo:hi].contiguous()
                scores_slice = scores_slice.sigmoid() ** self.weight_gamma
                sample_idx = pointnet2_utils.furthest_point_sample_weights(xyz_slice, scores_slice, self.npoint_list[i])
            elif method == 's-topk':
                assert scores is not None
                scores, sample_idx = torch.topk(scores, k=self.npoint_list[i], dim=-1)
                sample_idx = sample_idx.int()
            elif method == 'd-fps-faraware':
                pts_depth = torch.norm(xyz_slice, p=2, dim=-1)
                _, sorted_idx = torch.sort(pts_depth, dim=-1)
                pts_near_idx = sorted_idx[:, :-256]
                pts_far_idx = sorted_idx[:, -256:]
                pts_near = torch.stack([xyz_slice[b][pts_near_idx[b]] for b in range(batch_size)], dim=0)
                base_near = pointnet2_utils.furthest_point_sample(pts_near.contiguous(), self.npoint_list[i] - 256)
                sample_near_idx = torch.stack([pts_near_idx[b][base_near[b].long()] for b in range(batch_size)], dim=0)
                sample_idx = torch.cat([sample_near_idx, pts_far_idx], dim=-1).int()
            else:
                raise NotImplementedError
            sample_idx_list.append(sample_idx + lo)
            _stage('sample:' + method)
        return torch.cat(sample_idx_list, dim=-1)

    # ------------------------------------------------------------------------------------------- groupers
    def _point_group(self, i, xyz, new_xyz, features):
        """Point branch (QueryAndGroup[Dilated], idx_cnt mask): -> point_mlps[i] output (B, Cout, npoint, nsample)."""
        grouper = self.groupers[i]
        if isinstance(grouper, pointnet2_utils.QueryAndGroupDilated):
            idx_cnt, idx = pointnet2_utils.ball_query_dilated(grouper.radius_in, grouper.radius_out, grouper.nsample,
                                                              xyz, new_xyz)
        else:
            idx_cnt, idx = pointnet2_utils.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz)
        _stage('ball_query')
        batch_size, n, _ = xyz.shape
        npoint = new_xyz.shape[1]
        rows = idx + (torch.arange(batch_size, device=idx.device, dtype=idx.dtype) * n).view(-1, 1, 1)
        w = _conv_weight(self.point_mlps[i][0])
        if features is not None:
            wx, wf = (w[:, :3], w[:, 3:]) if grouper.use_xyz else (None, w)
            src = features.transpose(1, 2).reshape(batch_size * n, features.shape[1])
        else:
            assert grouper.use_xyz, "Cannot have not features and not use xyz as a feature!"
            wx, wf, src = w, None, None
        y = pointnet2_utils.group_project(src, wf, wx, xyz.reshape(-1, 3), new_xyz.reshape(-1, 3),
                                          rows.view(batch_size * npoint, -1), (idx_cnt == 0).view(-1), batch_size)
        return self.point_mlps[i][1:](y)

    def _voxel_group(self, i, new_xyz, point_grid_coords, voxel_xyz, features_in, v2p_ind_tensor):
        """Voxel branch (VoxelQueryAndGrouping[Dilated], empty balls zeroed): -> relu(point_mlp + pos_mlp)."""
        grouper = self.groupers[i]
        ctr = new_xyz.reshape(-1, 3)
        if isinstance(grouper, voxel_query_utils.VoxelQueryAndGroupingDilated):
            idx, empty_ball_mask, _ = voxel_query_utils.voxel_query_dilated(
                grouper.max_range, grouper.stride, grouper.former_radius, grouper.radius, grouper.nsample, voxel_xyz,
                ctr, point_grid_coords, v2p_ind_tensor)
        else:
            idx, empty_ball_mask, _ = voxel_query_utils.voxel_query(grouper.max_range, grouper.radius, grouper.nsample,
                                                                    voxel_xyz, ctr, point_grid_coords, v2p_ind_tensor)
        _stage('voxel_query')
        batch_size = new_xyz.shape[0]
        yf = pointnet2_utils.group_project(features_in, _conv_weight(self.point_mlps[i][0]), None, voxel_xyz, ctr, idx,
                                           empty_ball_mask, batch_size)
        yx = pointnet2_utils.group_project(None, None, _conv_weight(self.pos_mlps[i][0]), voxel_xyz, ctr, idx,
                                           empty_ball_mask, batch_size)
        return self.relu(self.point_mlps[i][1:](yf) + self.pos_mlps[i][1:](yx))

    # ------------------------------------------------------------------------------------------- forward
    def forward(self, xyz: torch.Tensor, features: torch.Tensor = None, new_xyz=None, scores=None, part_scores=None,
                sp_tensor=None, unique_idxs=None, switch=False, centroids=None, centroid_voxel_idxs=None, static=False):
        """
        :param xyz: (B, N, 3) tensor of the xyz coordinates of the features
        :param features: (B, C, N) tensor of the descriptors of the features
        :param new_xyz: (B, npoint, 3) centres, or None to sample them
        :param scores: (N', 3) confidence logits of the previous layer's voxels, required when using s-fps
        :param sp_tensor / centroids / centroid_voxel_idxs / unique_idxs: the previous layer's voxel aggregation
        :param static: layer 0 only: aggregate at static row capacity with no host read (module docstring); later
                 layers take the mode from sp_tensor.n_valid
        :return: new_xyz (B, npoint, 3), new_features (B, C', npoint), new_scores or None, sp_tensor, centroids,
                 centroid_voxel_idxs, unique_idxs, None
        """
        new_features_list = []
        batch_size = len(xyz)
        static = bool(static) if sp_tensor is None else sp_tensor.n_valid is not None
        if static and (self.training or torch.is_grad_enabled()):
            raise RuntimeError('the static-capacity path of the voxel-point SA modules is inference only: it needs '
                               'model.eval() and torch.no_grad() (training %s, grad %s)'
                               % (self.training, torch.is_grad_enabled()))
        ori_scores = None
        old_features = None
        voxel_size_tensor, point_cloud_range_tensor = self._grid_tensors(xyz.device)
        xyz_flipped = xyz.transpose(1, 2).contiguous()
        if scores is not None:
            ori_scores = torch.max(scores.sigmoid(), dim=1, keepdim=True)[0]
            scores, _ = torch.max(scores, dim=1, keepdim=True)
            if unique_idxs is not None:
                scores = scores[unique_idxs]
                scores = scores.view(batch_size, -1)
        if new_xyz is None:
            assert len(self.npoint_list) == len(self.sample_range_list) == len(self.sample_method_list)
            sample_idx = self._sample(xyz, features, scores, batch_size)
            new_xyz = pointnet2_utils.gather_operation(xyz_flipped, sample_idx).transpose(1, 2).contiguous()
            if self.skip_connection:
                old_features = pointnet2_utils.gather_operation(features, sample_idx) if features is not None else None

        if unique_idxs is not None:
            sample_idx = sample_idx + (torch.arange(sample_idx.shape[0], device=sample_idx.device,
                                                    dtype=sample_idx.dtype) * xyz.shape[1]).view(-1, 1)
            unique_idxs = unique_idxs[sample_idx.view(-1).long()]

        if sp_tensor is not None:
            if static:
                v2p_ind_tensor = spx_ops.voxel_table_build(sp_tensor.indices, sp_tensor.batch_size,
                                                           sp_tensor.spatial_shape, d_n=sp_tensor.n_valid)
            else:
                v2p_ind_tensor = common_utils.generate_voxel2pinds(sp_tensor)
            num_points = new_xyz.shape[1]
            pgc = new_xyz.clone().view(-1, 3)
            pgc_x = (pgc[:, 0:1] - point_cloud_range_tensor[0]) / voxel_size_tensor[0]
            pgc_y = (pgc[:, 1:2] - point_cloud_range_tensor[1]) / voxel_size_tensor[1]
            pgc_z = (pgc[:, 2:] - point_cloud_range_tensor[2]) / voxel_size_tensor[2]
            point_batch_idx = torch.arange(batch_size, device=new_xyz.device, dtype=new_xyz.dtype)
            point_batch_idx = point_batch_idx.view(-1, 1).expand(batch_size, num_points).reshape(-1, 1)
            point_grid_coords = torch.cat([point_batch_idx, pgc_z, pgc_y, pgc_x], dim=-1).contiguous().int()
            # the centroids' xyz columns only lead back to sampled coordinates, which carry no gradient
            voxel_xyz = centroids[:, 1:4].detach().contiguous()
            features_in = sp_tensor.features.contiguous()
            _stage('voxel_table')

        for i in range(len(self.groupers)):
            if sp_tensor is None:
                new_features = self._point_group(i, xyz, new_xyz, features)
            else:
                new_features = self._voxel_group(i, new_xyz, point_grid_coords, voxel_xyz, features_in, v2p_ind_tensor)

            if self.pool_method == 'max_pool':
                pooled_features = F.max_pool2d(new_features, kernel_size=[1, new_features.size(3)])
            elif self.pool_method == 'avg_pool':
                pooled_features = F.avg_pool2d(new_features, kernel_size=[1, new_features.size(3)])
            elif self.pool_method == 'weight_pool':
                pos_weights = self.pos_mlps[i](new_features)
                new_features = new_features * pos_weights
                pooled_features = torch.sum(new_features, dim=-1)
            else:
                raise NotImplementedError
            new_features_list.append(pooled_features.squeeze(-1))  # (B, mlp[-1], npoint)
            _stage('mlp_pool')

        if self.skip_connection and old_features is not None:
            new_features_list.append(old_features)
        new_features = torch.cat(new_features_list, dim=1)
        if self.aggregation_mlp is not None:
            new_features = self.aggregation_mlp(new_features)
        _stage('mlp_pool')

        if sp_tensor is None:
            batch_size, channel, num_points = new_features.shape
            voxel_idxs = voxel_aggregation_utils.get_voxel_indices(new_xyz.clone().view(-1, 3).contiguous(),
                                                                   voxel_size=voxel_size_tensor,
                                                                   point_cloud_range=point_cloud_range_tensor)
            batch_idx = torch.arange(batch_size, device=new_xyz.device).view(-1, 1).expand(batch_size, num_points)
            batch_idx = batch_idx.reshape(-1, 1).long()
            voxel_idxs = torch.cat((batch_idx, torch.flip(voxel_idxs, dims=[1])), dim=-1)   # (b, z, y, x)
            xyz_for_voxel = torch.cat([batch_idx.to(new_xyz.dtype), new_xyz.view(-1, 3)], dim=-1)
            features_for_voxel = new_features.permute(0, 2, 1).contiguous().view(-1, channel)
            point_for_voxel = torch.cat([xyz_for_voxel, features_for_voxel], dim=-1)   # bxyz + features
            sparse_shape = np.asarray(self.grid_size)[::-1].astype(np.int64)
            if static:
                # B * npoint rows, as many as there are points: no overflow; the live count stays on the device
                centroids_coords_features, centroid_voxel_idxs, _, unique_idxs, n_valid = \
                    voxel_aggregation_utils.get_centroid_per_voxel(
                        point_for_voxel, voxel_idxs, extent=[batch_size] + [int(v) for v in sparse_shape], sync=False)
                static_kw = dict(n_valid=n_valid, static_caps={})
            else:
                centroids_coords_features, centroid_voxel_idxs, _, unique_idxs = \
                    voxel_aggregation_utils.get_centroid_per_voxel(point_for_voxel, voxel_idxs)
                static_kw = {}
            centroids = centroids_coords_features[:, 0:4].contiguous()
            sp_tensor = spconv.SparseConvTensor(features=centroids_coords_features[:, 4:].contiguous(),
                                                indices=centroid_voxel_idxs.int(), spatial_shape=sparse_shape,
                                                batch_size=batch_size, **static_kw)
            _stage('centroid_aggregation')
        elif self.sa_layer_idx > 0 and self.sa_layer_idx < 3:
            sp_tensor = self._unet_update(new_xyz, new_features, sp_tensor, centroid_voxel_idxs, ori_scores,
                                          voxel_size_tensor, point_cloud_range_tensor,
                                          v2p_ind_tensor if static else None)
            _stage('unet')

        if self.confidence_mlp is not None:
            new_scores = self.confidence_mlp(sp_tensor.features.unsqueeze(-1)).squeeze(2)
            return new_xyz.contiguous(), new_features.contiguous(), new_scores.contiguous(), \
                sp_tensor, centroids, centroid_voxel_idxs.contiguous(), unique_idxs, None
        return new_xyz.contiguous(), new_features.contiguous(), None, \
            sp_tensor, centroids, centroid_voxel_idxs.contiguous(), unique_idxs, None

    def _unet_source_static(self, new_xyz, new_features, sp_tensor, centroid_voxel_idxs, table):
        """The U-Net's input at static capacity: the per-voxel mean of the new point features at the rows of sp_tensor,
        one op instead of the eager chain below (same live rows, bit for bit; dead rows are not written)."""
        feats = spx_ops.voxel_rows_mean(new_xyz, new_features, table, self.point_cloud_range[0:3], self.voxel_size,
                                        sp_tensor.features.shape[0], d_n_rows=sp_tensor.n_valid)
        return spconv.SparseConvTensor(features=feats, indices=centroid_voxel_idxs.int(),
                                       spatial_shape=sp_tensor.spatial_shape, batch_size=new_xyz.shape[0],
                                       n_valid=sp_tensor.n_valid, static_caps=sp_tensor.static_caps)

    def _unet_update(self, new_xyz, new_features, sp_tensor, centroid_voxel_idxs, ori_scores, voxel_size_tensor,
                     point_cloud_range_tensor, static_table=None):
        """Layers 1-2: aggregate the new point features into the voxels of sp_tensor, run the sparse U-Net on them and
        add the result, weighted by the previous layer's confidence, to sp_tensor's own 1x1 update.
        static_table: sp_tensor's cell table in static mode (sp_tensor.n_valid is the live row count)."""
        if static_table is not None:
            source_tensor = self._unet_source_static(new_xyz, new_features, sp_tensor, centroid_voxel_idxs, static_table)
        else:
            source_tensor = self._unet_source(new_xyz, new_features, sp_tensor, centroid_voxel_idxs, voxel_size_tensor,
                                              point_cloud_range_tensor)
        _stage('unet_source')
        sp4x_tensor = self.spconv4x_mlps(source_tensor)
        sp8x_tensor = self.spconv8x_mlps(sp4x_tensor)
        sp16x_tensor = self.spconv16x_mlps(sp8x_tensor)
        spinv16x_tensor = self.spconvinv16x_mlps(sp16x_tensor)
        spinv16x_tensor = replace_feature(spinv16x_tensor, spinv16x_tensor.features + sp16x_tensor.features)
        spinv8x_tensor = self.spconvinv8x_mlps(spinv16x_tensor)
        spinv8x_tensor = replace_feature(spinv8x_tensor, spinv8x_tensor.features + sp8x_tensor.features)
        spinv4x_tensor = self.spconvinv4x_mlps(spinv8x_tensor)
        spinv4x_tensor = replace_feature(spinv4x_tensor, spinv4x_tensor.features + sp4x_tensor.features)
        dest_tensor = self.spconv_out_mlps(spinv4x_tensor)
        sp_tensor = self.spconv_mlps(sp_tensor)
        return replace_feature(sp_tensor, self.update_relu(sp_tensor.features + ori_scores * dest_tensor.features))

    def _unet_source(self, new_xyz, new_features, sp_tensor, centroid_voxel_idxs, voxel_size_tensor,
                     point_cloud_range_tensor):
        """The U-Net's input: the per-voxel mean of the new point features at the rows of sp_tensor, zeros elsewhere."""
        batch_size, last_channel, num_points = new_features.shape
        new_point_idxs = voxel_aggregation_utils.get_voxel_indices(new_xyz.view(-1, 3), voxel_size=voxel_size_tensor,
                                                                   point_cloud_range=point_cloud_range_tensor)
        new_batch_idx = torch.arange(batch_size, device=new_xyz.device).view(-1, 1).expand(batch_size, num_points)
        new_batch_idx = new_batch_idx.reshape(-1, 1).long()
        new_voxel_idxs = torch.cat((new_batch_idx, new_point_idxs), dim=-1)[:, [0, 3, 2, 1]]
        new_xyz_for_voxel = torch.cat([new_batch_idx.to(new_xyz.dtype), new_xyz.view(-1, 3)], dim=-1)
        new_features_for_voxel = new_features.permute(0, 2, 1).contiguous().view(-1, last_channel)
        point_for_voxel = torch.cat([new_xyz_for_voxel, new_features_for_voxel], dim=-1)
        new_centroids, new_centroid_voxel_idxs, _, _ = \
            voxel_aggregation_utils.get_centroid_per_voxel(point_for_voxel, new_voxel_idxs)
        update_indices_nonempty, update_nonempty_mask = \
            voxel_aggregation_utils.get_nonempty_voxel_feature_indices(new_centroid_voxel_idxs, sp_tensor)
        source_features = new_centroids.new_zeros([sp_tensor.features.shape[0], new_centroids.shape[1] - 4])
        source_features[update_indices_nonempty] = new_centroids[:, 4:][update_nonempty_mask]
        return spconv.SparseConvTensor(features=source_features.contiguous(), indices=centroid_voxel_idxs.int(),
                                       spatial_shape=sp_tensor.spatial_shape, batch_size=batch_size)


class VoxelPointnetSAModuleFSMSGDistillation(_VoxelPointnetSAModuleFSDistillationBase):
    """Pointnet set abstraction layer with fusion sampling and multiscale grouping"""

    def __init__(self, *,
                 npoint_list: List[int] = None,
                 sample_range_list: List[List[int]] = None,
                 sample_method_list: List[str] = None,
                 query_range: List[List[int]] = None,
                 sp_stride: int = None,
                 stride: List[List[int]] = None,
                 radii: List[float],
                 nsamples: List[int],
                 mlps: List[List[int]],
                 spconv_mlps: List[int] = None,
                 spconv_mlps_post: List[int] = None,
                 bn: bool = True,
                 use_xyz: bool = True,
                 pool_method='max_pool',
                 dilated_radius_group: bool = False,
                 skip_connection: bool = False,
                 weight_gamma: float = 1.0,
                 aggregation_mlp: List[int] = None,
                 confidence_mlp: List[int] = None,
                 sa_layer_idx=1,
                 voxel_size=None,
                 grid_size=None,
                 point_cloud_range=None
                 ):
        """
        :param npoint_list: list of int, number of samples for every sampling method
        :param sample_range_list: list of list of int, sample index range [left, right] for every sampling method
        :param sample_method_list: list of str, d-fps, f-fps, s-fps, s-topk or d-fps-faraware
        :param query_range / stride: per radius, the voxel-query search extents and strides (layers > 0)
        :param radii: list of float, list of radii to group with
        :param nsamples: list of int, number of samples in each ball query
        :param mlps: list of list of int, spec of the pointnet before the global pooling for each scale
        :param spconv_mlps: channels of the sparse update at layers 1-2
        :param use_xyz: whether the point branch feeds relative xyz to its first conv
        :param pool_method: max_pool / avg_pool / weight_pool
        :param dilated_radius_group: whether to use radius dilated group
        :param skip_connection: whether to add skip connection
        :param weight_gamma: gamma for s-fps, default: 1.0
        :param aggregation_mlp: list of int, spec aggregation mlp
        :param confidence_mlp: list of int, spec confidence mlp
        :param sa_layer_idx: 0 = point branch + voxel aggregation; > 0 = voxel branch (1-2 also run the sparse U-Net)
        """
        super().__init__()

        assert npoint_list is None or len(npoint_list) == len(sample_range_list) == len(sample_method_list)
        assert len(radii) == len(nsamples) == len(mlps)

        self.npoint_list = npoint_list
        self.sample_range_list = sample_range_list
        self.sample_method_list = sample_method_list
        self.query_range = query_range
        self.sp_stride = sp_stride
        self.stride = stride
        self.radii = radii
        self.spconv_mlps = spconv_mlps
        self.spconv_mlps_post = spconv_mlps_post
        self.groupers = nn.ModuleList()
        self.sa_layer_idx = sa_layer_idx
        self.pool_method = pool_method
        self.voxel_size = voxel_size
        self.grid_size = grid_size
        self.point_cloud_range = point_cloud_range

        if mlps[0]:
            self.point_mlps = nn.ModuleList()
            if self.sa_layer_idx > 0:
                self.pos_mlps = nn.ModuleList()
        if self.pool_method == "weight_pool":
            self.pos_mlps = nn.ModuleList()

        former_radius = 0.0
        in_channels, out_channels = 0, 0
        for i in range(len(radii)):
            radius = radii[i]
            query_ranges = query_range[i]
            strides = stride[i]
            nsample = nsamples[i]
            if dilated_radius_group:
                if sa_layer_idx == 0:
                    self.groupers.append(
                        pointnet2_utils.QueryAndGroupDilated(former_radius, radius, nsample, use_xyz=use_xyz))
                else:
                    self.groupers.append(voxel_query_utils.VoxelQueryAndGroupingDilated(
                        query_ranges, strides, former_radius, radius, nsample))
            else:
                if sa_layer_idx == 0:
                    self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz))
                else:
                    self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(query_ranges, radius, nsample))
            former_radius = radius

            if mlps[0] and self.sa_layer_idx == 0:
                mlp_spec = mlps[i]
                if use_xyz:
                    mlp_spec[0] += 3
                ori_mlp_spec_in = mlp_spec[0]
                shared_point_mlp = []
                for k in range(len(mlp_spec) - 1):
                    shared_point_mlp.extend([
                        nn.Conv2d(mlp_spec[k], mlp_spec[k + 1], kernel_size=1, bias=False),
                        nn.BatchNorm2d(mlp_spec[k + 1]),
                        nn.ReLU()
                    ])
                self.point_mlps.append(nn.Sequential(*shared_point_mlp))
                mlp_spec[0] = ori_mlp_spec_in
                in_channels = mlp_spec[0] - 3 if use_xyz else mlp_spec[0]
                out_channels += mlp_spec[-1]
            else:
                mlp_spec = mlps[i]
                ori_mlp_spec_in = mlp_spec[0]
                shared_point_mlp = []
                for k in range(len(mlp_spec) - 2):
                    shared_point_mlp.extend([
                        nn.Conv2d(mlp_spec[k], mlp_spec[k + 1], kernel_size=1, bias=False),
                        nn.BatchNorm2d(mlp_spec[k + 1]),
                        nn.ReLU()
                    ])
                shared_point_mlp.extend([
                    nn.Conv2d(mlp_spec[-2], mlp_spec[-1], kernel_size=1, bias=False),
                    nn.BatchNorm2d(mlp_spec[-1]),
                ])
                self.point_mlps.append(nn.Sequential(*shared_point_mlp))
                self.pos_mlps.append(nn.Sequential(
                    nn.Conv2d(3, mlp_spec[-1] // 2, kernel_size=1, bias=False),
                    nn.BatchNorm2d(mlp_spec[-1] // 2),
                    nn.ReLU(),
                    nn.Conv2d(mlp_spec[-1] // 2, mlp_spec[-1], kernel_size=1, bias=False),
                    nn.BatchNorm2d(mlp_spec[-1]),
                ))
                self.relu = nn.ReLU()
                mlp_spec[0] = ori_mlp_spec_in
                in_channels = mlp_spec[0] - 3 if use_xyz else mlp_spec[0]
                out_channels += mlp_spec[-1]

        self.pool_method = pool_method
        self.dilated_radius_group = dilated_radius_group
        self.skip_connection = skip_connection
        self.weight_gamma = weight_gamma

        if skip_connection:
            out_channels += in_channels

        if aggregation_mlp is not None:
            shared_mlp = []
            for k in range(len(aggregation_mlp)):
                shared_mlp.extend([
                    nn.Conv1d(out_channels, aggregation_mlp[k], kernel_size=1, bias=False),
                    nn.BatchNorm1d(aggregation_mlp[k]),
                    nn.ReLU()
                ])
                out_channels = aggregation_mlp[k]
            self.aggregation_mlp = nn.Sequential(*shared_mlp)
        else:
            self.aggregation_mlp = None

        if (self.sa_layer_idx <= 2) and (self.sa_layer_idx > 0):
            norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
            tagspconv8x = "spconv8x%d" % sa_layer_idx
            tagspconv16x = "spconv16x%d" % sa_layer_idx
            n_EnDe = int(out_channels // 2)
            n_EnDe2x = n_EnDe
            n_EnDe4x = n_EnDe * 2

            self.spconv4x_mlps = spconv.SparseSequential(
                spconv.SubMConv3d(out_channels, n_EnDe, 1, padding=0, bias=False, indice_key="subm4x"),
                norm_fn(n_EnDe),
                nn.ReLU(),
            )
            self.spconv8x_mlps = spconv.SparseSequential(
                spconv.SparseConv3d(n_EnDe, n_EnDe2x, 3, stride=2, padding=1, bias=False, indice_key=tagspconv8x),
                norm_fn(n_EnDe2x),
                nn.ReLU(),
            )
            self.spconv16x_mlps = spconv.SparseSequential(
                spconv.SparseConv3d(n_EnDe2x, n_EnDe4x, 3, stride=2, padding=1, bias=False, indice_key=tagspconv16x),
                norm_fn(n_EnDe4x),
                nn.ReLU(),
            )
            self.spconvinv16x_mlps = spconv.SparseSequential(
                spconv.SubMConv3d(n_EnDe4x, n_EnDe4x, 3, padding=1, bias=False, indice_key="subm16x"),
                norm_fn(n_EnDe4x),
                nn.ReLU(),
                spconv.SubMConv3d(n_EnDe4x, n_EnDe4x, 3, padding=1, bias=False, indice_key="subm16x"),
                norm_fn(n_EnDe4x),
                nn.ReLU(),
            )
            self.spconvinv8x_mlps = spconv.SparseSequential(
                spconv.SparseInverseConv3d(n_EnDe4x, n_EnDe2x, 3, indice_key=tagspconv16x, bias=False),
                norm_fn(n_EnDe2x),
                nn.ReLU(),
                spconv.SubMConv3d(n_EnDe2x, n_EnDe2x, 3, padding=1, bias=False, indice_key="subm8x"),
                norm_fn(n_EnDe2x),
                nn.ReLU(),
                spconv.SubMConv3d(n_EnDe2x, n_EnDe2x, 3, padding=1, bias=False, indice_key="subm8x"),
                norm_fn(n_EnDe2x),
                nn.ReLU(),
            )
            self.spconvinv4x_mlps = spconv.SparseSequential(
                spconv.SparseInverseConv3d(n_EnDe2x, n_EnDe, 3, indice_key=tagspconv8x, bias=False),
                norm_fn(n_EnDe),
                nn.ReLU(),
                spconv.SubMConv3d(n_EnDe, n_EnDe, 3, padding=1, bias=False, indice_key="subm4x"),
                norm_fn(n_EnDe),
                nn.ReLU(),
                spconv.SubMConv3d(n_EnDe, n_EnDe, 3, padding=1, bias=False, indice_key="subm4x"),
                norm_fn(n_EnDe),
                nn.ReLU(),
            )
            self.spconv_out_mlps = spconv.SparseSequential(
                spconv.SubMConv3d(n_EnDe, out_channels, 1, padding=0, bias=False, indice_key="submencoder"),
                norm_fn(out_channels),
            )
            self.spconv_mlps = spconv.SparseSequential(
                spconv.SubMConv3d(spconv_mlps[-2], spconv_mlps[-1], 1, padding=0, bias=False, indice_key="subm"),
                norm_fn(spconv_mlps[-1]),
            )
            self.update_relu = nn.ReLU()
            out_channels = spconv_mlps[-1]

        if confidence_mlp is not None:
            shared_mlp = []
            for k in range(len(confidence_mlp)):
                shared_mlp.extend([
                    nn.Conv1d(out_channels, confidence_mlp[k], kernel_size=1, bias=False),
                    nn.BatchNorm1d(confidence_mlp[k]),
                    nn.ReLU()
                ])
                out_channels = confidence_mlp[k]
            shared_mlp.append(nn.Conv1d(out_channels, 3, kernel_size=1, bias=True))
            self.confidence_mlp = nn.Sequential(*shared_mlp)
            pi = 0.01
            nn.init.constant_(self.confidence_mlp[3].bias, -np.log((1 - pi) / pi))
        else:
            self.confidence_mlp = None


class VoxelPointnetSAModuleFSDistillation(VoxelPointnetSAModuleFSMSGDistillation):
    """Pointnet set abstraction layer with fusion sampling (one radius)"""

    def __init__(self, *,
                 mlp: List[int],
                 npoint_list: List[int] = None,
                 sample_range_list: List[List[int]] = None,
                 sample_method_list: List[str] = None,
                 query_range: List[List[int]] = None,
                 sp_stride: int = None,
                 stride: List[List[int]] = None,
                 spconv_mlps: List[int] = None,
                 spconv_mlps_post: List[int] = None,
                 radius: float = None,
                 nsample: int = None,
                 bn: bool = True,
                 use_xyz: bool = True,
                 pool_method='max_pool',
                 dilated_radius_group: bool = False,
                 skip_connection: bool = False,
                 weight_gamma: float = 1.0,
                 aggregation_mlp: List[int] = None,
                 confidence_mlp: List[int] = None,
                 sa_layer_idx=None,
                 voxel_size=None,
                 grid_size=None,
                 point_cloud_range=None
                 ):
        super().__init__(
            mlps=[mlp], npoint_list=npoint_list, sample_range_list=sample_range_list,
            sample_method_list=sample_method_list, query_range=query_range, sp_stride=sp_stride, stride=stride,
            radii=[radius], nsamples=[nsample], spconv_mlps=spconv_mlps, spconv_mlps_post=spconv_mlps_post,
            bn=bn, use_xyz=use_xyz, pool_method=pool_method, dilated_radius_group=dilated_radius_group,
            skip_connection=skip_connection, weight_gamma=weight_gamma,
            aggregation_mlp=aggregation_mlp, confidence_mlp=confidence_mlp,
            sa_layer_idx=sa_layer_idx, voxel_size=voxel_size, grid_size=grid_size, point_cloud_range=point_cloud_range
        )
