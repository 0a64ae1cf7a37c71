"""The fork's NeighborVoxelSAModuleMSG (reference pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py): a voxel
query around every new voxel centre, a per-scale Conv1d on the source features BEFORE grouping, a position encoding of
the grouped offsets, and max / avg / weighted-sum pooling.  Same constructor arguments, submodule tree (state_dict keys)
and return values; the search and grouping are voxel_query_utils.VoxelQueryAndGrouping (csrc/voxel_query.hip)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import voxel_query_utils


class NeighborVoxelSAModuleMSG(nn.Module):

    def __init__(self, *, query_ranges, radii, nsamples, mlps, use_xyz=True, pool_method='max_pool'):
        """query_ranges: (z, y, x) cells scanned each way per scale; radii / nsamples: the ball of each scale; mlps:
        [c_in, c_out] per scale; pool_method: max_pool / avg_pool / weight_sum."""
        super().__init__()

        assert len(query_ranges) == len(nsamples) == len(mlps)

        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_pos_ws = nn.ModuleList()
        for i in range(len(query_ranges)):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(query_ranges[i], radii[i], nsamples[i]))
            mlp_spec = mlps[i]

            cur_mlp_in = nn.Sequential(
                nn.Conv1d(mlp_spec[0], mlp_spec[1], kernel_size=1, bias=False),
                nn.BatchNorm1d(mlp_spec[1])
            )
            cur_mlp_pos = nn.Sequential(
                nn.Conv2d(3, mlp_spec[1], kernel_size=1, bias=False),
                nn.BatchNorm2d(mlp_spec[1])
            )
            cur_mlp_pos_ws = nn.Sequential(
                nn.Conv2d(3, 16, kernel_size=1, bias=False),
                nn.ReLU(),
                nn.Conv2d(16, 16, kernel_size=1, bias=False),
                nn.ReLU(),
                nn.Conv2d(16, mlp_spec[1], kernel_size=1, bias=False),
                nn.Sigmoid()
            )

            self.mlps_in.append(cur_mlp_in)
            self.mlps_pos.append(cur_mlp_pos)
            self.mlps_pos_ws.append(cur_mlp_pos_ws)

        self.relu = nn.ReLU()
        self.pool_method = pool_method

        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d) or isinstance(m, nn.Conv1d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d) or isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), new_coords (M1 + M2 ..., 4) = (b, x, y, z) voxel
        coordinates, features (N1 + N2 ..., C), voxel2point_indices (B, Z, Y, X) ->
        new_features (M1 + M2 ..., sum_k c_out_k [* 2 for weight_sum]), mean density score (M1 + M2 ..., 1)."""
        # change the order to [batch_idx, z, y, x]
        new_coords = new_coords[:, [0, 3, 2, 1]].contiguous()
        new_features_list = []
        cur_scale_density = 0
        for k in range(len(self.groupers)):
            features_in = features.permute(1, 0).unsqueeze(0)           # (1, C, N1 + N2)
            features_in = self.mlps_in[k](features_in)
            features_in = features_in.permute(0, 2, 1).contiguous()     # (1, N1 + N2, C)
            features_in = features_in.view(-1, features_in.shape[-1])   # (N1 + N2, C)
            # grouped_features (M1 + M2, C, nsample), grouped_xyz (M1 + M2, 3, nsample)
            grouped_features, grouped_xyz, empty_ball_mask, density_score = self.groupers[k](
                new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in, voxel2point_indices
            )
            cur_scale_density = cur_scale_density + density_score
            empty = empty_ball_mask[:, None, None]
            grouped_features = grouped_features.masked_fill(empty, 0)

            grouped_features = grouped_features.permute(1, 0, 2).unsqueeze(dim=0)   # (1, C, M1 + M2, nsample)
            grouped_xyz = (grouped_xyz - new_xyz.unsqueeze(-1)).masked_fill(empty, 0)
            grouped_xyz = grouped_xyz.permute(1, 0, 2).unsqueeze(0)                 # (1, 3, M1 + M2, nsample)
            position_features = self.mlps_pos[k](grouped_xyz)
            position_ws = self.mlps_pos_ws[k](grouped_xyz)
            new_features = grouped_features + position_features
            new_features = self.relu(new_features)
            grouped_features = self.relu(grouped_features)
            ws_features = grouped_features * position_ws

            if self.pool_method == 'max_pool':
                new_features = F.max_pool2d(
                    new_features, kernel_size=[1, new_features.size(3)]
                ).squeeze(dim=-1)  # (1, C, M1 + M2 ...)
            elif self.pool_method == 'avg_pool':
                new_features = F.avg_pool2d(
                    new_features, kernel_size=[1, new_features.size(3)]
                ).squeeze(dim=-1)  # (1, C, M1 + M2 ...)
            elif self.pool_method == 'weight_sum':
                new_features = F.max_pool2d(
                    new_features, kernel_size=[1, new_features.size(3)]
                ).squeeze(dim=-1)
                ws_features = torch.sum(ws_features, dim=-1)
                new_features = torch.cat([new_features, ws_features], dim=1)
            else:
                raise NotImplementedError

            new_features = new_features.squeeze(dim=0).permute(1, 0)  # (M1 + M2 ..., C)
            new_features_list.append(new_features)

        new_features = torch.cat(new_features_list, dim=1)  # (M1 + M2 ..., C)
        cur_scale_density = cur_scale_density / len(self.groupers)
        return new_features, cur_scale_density
