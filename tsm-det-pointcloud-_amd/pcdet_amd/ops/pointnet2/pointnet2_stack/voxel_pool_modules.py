"""The fork's NeighborVoxelSAModuleMSG (reference pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py): a voxel
query around every new voxel centre, a per-scale Conv1d on the source features BEFORE grouping, a position encoding of
the grouped offsets, and max / avg / weighted-sum pooling.  Same constructor arguments, submodule tree (state_dict keys)
and return values; the search and grouping are voxel_query_utils.VoxelQueryAndGrouping (csrc/voxel_query.hip).

With `fused` set (off by default), max_pool on device tensors runs the tail after the query as one HIP op
(csrc/voxel_pool.hip, include/spx.h §27) with the position BatchNorm folded into an affine map; avg_pool and weight_sum
keep the composition."""
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
        # max_pool on device tensors through spx.ops.voxel_pool_max (pool_tail_fused) instead of the composition
        self.fused = False

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
        # (columns stacked, not indexed by a list: a list becomes a host-to-device copy, which a captured graph refuses)
        new_coords = torch.stack((new_coords[:, 0], new_coords[:, 3], new_coords[:, 2], new_coords[:, 1]), dim=1)
        new_features_list = []
        cur_scale_density = 0
        fused = self.fused and features.is_cuda and self.pool_method == 'max_pool'
        for k in range(len(self.groupers)):
            features_in = features.permute(1, 0).unsqueeze(0)           # (1, C, N1 + N2)
            features_in = self.mlps_in[k](features_in)
            features_in = features_in.permute(0, 2, 1).contiguous()     # (1, N1 + N2, C)
            features_in = features_in.view(-1, features_in.shape[-1])   # (N1 + N2, C)
            if fused:
                # the table holds global rows and the op gathers by them: no per-frame counts, no host read
                grouper = self.groupers[k]
                idx, empty_ball_mask, density_score = voxel_query_utils.voxel_query(
                    grouper.max_range, grouper.radius, grouper.nsample, xyz, new_xyz, new_coords, voxel2point_indices)
                new_features = self.pool_tail_fused(k, features_in, xyz, new_xyz, idx, empty_ball_mask)
            else:
                # grouped_features (M1 + M2, C, nsample), grouped_xyz (M1 + M2, 3, nsample)
                grouped_features, grouped_xyz, empty_ball_mask, density_score = self.groupers[k](
                    new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in, voxel2point_indices
                )
                new_features = self._tail_grouped(k, grouped_features, grouped_xyz, new_xyz, empty_ball_mask)
            cur_scale_density = cur_scale_density + density_score
            new_features_list.append(new_features)

        new_features = torch.cat(new_features_list, dim=1)  # (M1 + M2 ..., C)
        cur_scale_density = cur_scale_density / len(self.groupers)
        return new_features, cur_scale_density

    def pool_tail(self, k, features_in, xyz, new_xyz, idx, empty):
        """The composition of scale k for given neighbour lists: features_in (N, C) = mlps_in[k]'s output, idx (M, nsample)
        GLOBAL rows of xyz / features_in, empty (M) bool -> (M, C [* 2 for weight_sum]).  Runs on any device and dtype;
        it is what pool_tail_fused is compared against."""
        rows = idx.long()
        grouped_features = features_in[rows].permute(0, 2, 1).contiguous()     # (M, C, nsample)
        grouped_xyz = xyz[rows].permute(0, 2, 1).contiguous()                  # (M, 3, nsample)
        return self._tail_grouped(k, grouped_features, grouped_xyz, new_xyz, empty)

    def _tail_grouped(self, k, grouped_features, grouped_xyz, new_xyz, empty_ball_mask):
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

        return new_features.squeeze(dim=0).permute(1, 0)  # (M1 + M2 ..., C)

    def fold_position_bn(self, k, moments, n_cols):
        """mlps_pos[k] = Conv2d(3, C, 1, bias=False) + BatchNorm2d as one affine map of the offset d: -> A (C, 3), b (C)
        with BN(W d) = A d + b, in the weight's dtype and differentiable in W, gamma, beta.
        Training: moments = float64[9] (sum d, upper triangle of sum d d^T) over the n_cols = M * nsample columns the
        BatchNorm would see; per channel mean = W . mu and var = W^T Sigma W (Sigma = E[d d^T] - mu mu^T, in float64
        because it cancels), and the running statistics are updated as nn.BatchNorm2d updates them.  The moments are
        geometry only, so no gradient goes through them.  Eval: the running statistics; moments is not read."""
        conv, bn = self.mlps_pos[k][0], self.mlps_pos[k][1]
        w = conv.weight.view(conv.weight.shape[0], 3)
        w64 = w.double()
        if bn.training or not bn.track_running_stats:
            n = int(n_cols)
            if n < 2:
                raise ValueError('Expected more than 1 value per channel when training, got %d columns' % n)
            mom = moments.detach().double()
            mu = mom[:3] / n
            tri = mom[3:] / n
            second = torch.stack((tri[0], tri[1], tri[2], tri[1], tri[3], tri[4], tri[2], tri[4], tri[5])).view(3, 3)
            sigma = second - mu[:, None] * mu[None, :]
            mean = w64 @ mu
            var = ((w64 @ sigma) * w64).sum(dim=1).clamp_min(0)
            if bn.training and bn.track_running_stats:
                with torch.no_grad():
                    bn.num_batches_tracked += 1
                    if bn.momentum is None:
                        factor = 1.0 / bn.num_batches_tracked.double()
                    else:
                        factor = bn.momentum
                    bn.running_mean.mul_(1 - factor).add_((mean * factor).to(bn.running_mean.dtype))
                    bn.running_var.mul_(1 - factor).add_((var * (n / (n - 1.0)) * factor).to(bn.running_var.dtype))
        else:
            mean, var = bn.running_mean.double(), bn.running_var.double()
        gamma = bn.weight.double() if bn.affine else torch.ones_like(mean)
        scale = gamma / torch.sqrt(var + bn.eps)
        a = scale[:, None] * w64
        b = -scale * mean
        if bn.affine:
            b = b + bn.bias.double()
        return a.to(w.dtype), b.to(w.dtype)

    def pool_tail_fused(self, k, features_in, xyz, new_xyz, idx, empty):
        """Scale k on spx.ops.voxel_pool_max (include/spx.h §27; max_pool, device tensors): the moments of the offsets
        (training), the BatchNorm fold on C x 3 numbers in torch, one fused gather + affine + max.  mlps_pos_ws is not
        evaluated: max_pool never uses it."""
        from spx import ops
        xyz, new_xyz = xyz.detach(), new_xyz.detach()
        bn = self.mlps_pos[k][1]
        moments = None
        if bn.training or not bn.track_running_stats:
            if idx.numel() < 2:
                raise ValueError('Expected more than 1 value per channel when training, got %d columns' % idx.numel())
            moments = ops.voxel_pool_moments(xyz, new_xyz, idx, empty)
        a, b = self.fold_position_bn(k, moments, idx.numel())
        return ops.voxel_pool_max(features_in, xyz, new_xyz, idx, empty, a, b)
