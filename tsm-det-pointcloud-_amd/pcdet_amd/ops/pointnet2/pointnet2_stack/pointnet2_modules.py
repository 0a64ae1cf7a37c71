"""Stacked set-abstraction and feature-propagation modules on libspx (reference
pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py: StackSAModuleMSG, StackPointnetFPModule,
build_local_aggregation_module).  Same constructor arguments, submodule tree (state_dict keys) and return values; the
grouping and interpolation run the HIP kernels of csrc/pointnet2_stack.hip through pointnet2_utils.  The vector-pool
modules of PV-RCNN++ are not ported.

With `fused` set (off by default), StackSAModuleMSG in eval mode under no_grad runs every two-layer max_pool scale after
its ball query as one HIP op, spx.ops.sa_mlp2_max (include/spx.h §28): the first conv's feature columns become one GEMM
over the source rows, both BatchNorms are folded from their running statistics, and only the (M, C_out) result reaches
memory.  Every other case, training included, runs the composition unchanged."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from spx import ops

from . import pointnet2_utils


def build_local_aggregation_module(input_channels, config):
    local_aggregation_name = config.get('NAME', 'StackSAModuleMSG')

    if local_aggregation_name == 'StackSAModuleMSG':
        mlps = config.MLPS
        for k in range(len(mlps)):
            mlps[k] = [input_channels] + mlps[k]
        cur_layer = StackSAModuleMSG(
            radii=config.POOL_RADIUS, nsamples=config.NSAMPLE, mlps=mlps, use_xyz=True, pool_method='max_pool',
        )
        num_c_out = sum([x[-1] for x in mlps])
    elif local_aggregation_name == 'VectorPoolAggregationModuleMSG':
        raise NotImplementedError("VectorPoolAggregationModuleMSG: vector pooling (vector_pool_gpu.cu, PV-RCNN++) is not "
                                  "ported")
    else:
        raise NotImplementedError

    return cur_layer, num_c_out


class StackSAModuleMSG(nn.Module):

    def __init__(self, *, radii, nsamples, mlps, use_xyz=True, pool_method='max_pool'):
        """radii / nsamples: one ball query per scale; mlps: the pointnet of each scale ([c_in, ...], c_in without the
        3 xyz channels, which are added here when use_xyz); pool_method: max_pool / avg_pool."""
        super().__init__()

        assert len(radii) == len(nsamples) == len(mlps)

        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for i in range(len(radii)):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radii[i], nsamples[i], use_xyz=use_xyz))
            mlp_spec = mlps[i]
            if use_xyz:
                mlp_spec[0] += 3

            shared_mlps = []
            for k in range(len(mlp_spec) - 1):
                shared_mlps.extend([
                    nn.Conv2d(mlp_spec[k], mlp_spec[k + 1], kernel_size=1, bias=False),
                    nn.BatchNorm2d(mlp_spec[k + 1]),
                    nn.ReLU()
                ])
            self.mlps.append(nn.Sequential(*shared_mlps))
        self.pool_method = pool_method
        # eval + no_grad + device tensors + max_pool: two-layer scales of a supported shape through spx.ops.sa_mlp2_max
        # (scale_fused) instead of the composition
        self.fused = False

        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def scale_is_fusable(self, k, xyz, features):
        """Whether scale k may take the fused path for these inputs (the conditions of the module docstring)."""
        if not self.fused or self.training or torch.is_grad_enabled() or self.pool_method != 'max_pool':
            return False
        if not xyz.is_cuda or xyz.dtype != torch.float32 or (features is not None and features.dtype != torch.float32):
            return False
        mlp, grouper = self.mlps[k], self.groupers[k]
        if len(mlp) != 6 or not grouper.use_xyz:
            return False
        conv1, bn1, conv2, bn2 = mlp[0], mlp[1], mlp[3], mlp[4]
        if conv1.bias is not None or conv2.bias is not None or conv1.weight.dtype != torch.float32:
            return False
        if not (bn1.track_running_stats and bn2.track_running_stats):
            return False
        if conv1.in_channels != 3 + (0 if features is None else features.shape[1]):
            return False
        return ops.sa_mlp2_supported(conv1.out_channels, conv2.out_channels, grouper.nsample)

    @staticmethod
    def fold_bn(bn):
        """Eval-mode BatchNorm2d as the affine map (a, b), from the running statistics, in float64 then rounded once."""
        a = torch.rsqrt(bn.running_var.double() + bn.eps)
        if bn.weight is not None:
            a = a * bn.weight.double()
        b = -bn.running_mean.double() * a
        if bn.bias is not None:
            b = b + bn.bias.double()
        return a.float(), b.float()

    @staticmethod
    def global_row_offset(xyz_batch_cnt, new_xyz_batch_cnt, m):
        """(M, 1) int32: the first source row of the frame each query row belongs to, from cumulative sums of the counts
        on the device (no host read).  Dead query rows get the last frame's; their lists are never read."""
        dev = new_xyz_batch_cnt.device
        ends = torch.cumsum(new_xyz_batch_cnt.long(), dim=0)
        frame = torch.searchsorted(ends, torch.arange(m, device=dev), right=True).clamp_(max=ends.shape[0] - 1)
        src = xyz_batch_cnt.long()
        return (torch.cumsum(src, dim=0) - src)[frame].int().unsqueeze(1)

    def scale_fused(self, k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, row_offset):
        """Scale k in eval mode: the ball query, frame-local -> global rows, P = features Wf^T, then one fused op."""
        grouper, mlp = self.groupers[k], self.mlps[k]
        idx, empty = pointnet2_utils.ball_query(grouper.radius, grouper.nsample, xyz, xyz_batch_cnt, new_xyz,
                                                new_xyz_batch_cnt)
        w1 = mlp[0].weight.detach()[:, :, 0, 0]
        p = None if features is None else features.detach() @ w1[:, 3:].t()
        a1, b1 = self.fold_bn(mlp[1])
        a2, b2 = self.fold_bn(mlp[4])
        return ops.sa_mlp2_max(p, xyz, new_xyz, idx + row_offset, empty, w1[:, :3], a1, b1,
                               mlp[3].weight.detach()[:, :, 0, 0], a2, b2)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        """xyz (N1 + N2 ..., 3), new_xyz (M1 + M2 ..., 3), features (N1 + N2 ..., C) ->
        new_xyz, new_features (M1 + M2 ..., sum_k mlps[k][-1])."""
        new_features_list = []
        row_offset = None
        for k in range(len(self.groupers)):
            if self.scale_is_fusable(k, xyz, features):
                if row_offset is None:
                    row_offset = self.global_row_offset(xyz_batch_cnt, new_xyz_batch_cnt, new_xyz.shape[0])
                new_features_list.append(self.scale_fused(k, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features,
                                                          row_offset))
                continue
            new_features, ball_idxs = self.groupers[k](
                xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features
            )  # (M1 + M2, C, nsample)
            new_features = new_features.permute(1, 0, 2).unsqueeze(dim=0)  # (1, C, M1 + M2 ..., nsample)
            new_features = self.mlps[k](new_features)  # (1, C, M1 + M2 ..., nsample)

            if self.pool_method == 'max_pool':
                new_features = F.max_pool2d(
                    new_features, kernel_size=[1, new_features.size(3)]
                ).squeeze(dim=-1)  # (1, C, M1 + M2 ...)
            elif self.pool_method == 'avg_pool':
                new_features = F.avg_pool2d(
                    new_features, kernel_size=[1, new_features.size(3)]
                ).squeeze(dim=-1)  # (1, C, M1 + M2 ...)
            else:
                raise NotImplementedError
            new_features = new_features.squeeze(dim=0).permute(1, 0)  # (M1 + M2 ..., C)
            new_features_list.append(new_features)

        new_features = torch.cat(new_features_list, dim=1)  # (M1 + M2 ..., C)

        return new_xyz, new_features


class StackPointnetFPModule(nn.Module):
    def __init__(self, *, mlp):
        super().__init__()
        shared_mlps = []
        for k in range(len(mlp) - 1):
            shared_mlps.extend([
                nn.Conv2d(mlp[k], mlp[k + 1], kernel_size=1, bias=False),
                nn.BatchNorm2d(mlp[k + 1]),
                nn.ReLU()
            ])
        self.mlp = nn.Sequential(*shared_mlps)

    def forward(self, unknown, unknown_batch_cnt, known, known_batch_cnt, unknown_feats=None, known_feats=None):
        """unknown (N1 + N2 ..., 3), known (M1 + M2 ..., 3), unknown_feats (N1 + N2 ..., C1), known_feats
        (M1 + M2 ..., C2) -> (N1 + N2 ..., C_out).  A frame without known points has weights of 0 / 0, as in the
        reference; dead rows of `unknown` interpolate to 0 (their counts go to three_interpolate)."""
        dist, idx = pointnet2_utils.three_nn(unknown, unknown_batch_cnt, known, known_batch_cnt)
        dist_recip = 1.0 / (dist + 1e-8)
        norm = torch.sum(dist_recip, dim=-1, keepdim=True)
        weight = dist_recip / norm

        interpolated_feats = pointnet2_utils.three_interpolate(known_feats, idx, weight, unknown_batch_cnt)

        if unknown_feats is not None:
            new_features = torch.cat([interpolated_feats, unknown_feats], dim=1)  # (N1 + N2 ..., C2 + C1)
        else:
            new_features = interpolated_feats
        new_features = new_features.permute(1, 0)[None, :, :, None]  # (1, C, N1 + N2 ..., 1)
        new_features = self.mlp(new_features)

        new_features = new_features.squeeze(dim=0).squeeze(dim=-1).permute(1, 0)  # (N1 + N2 ..., C)
        return new_features
