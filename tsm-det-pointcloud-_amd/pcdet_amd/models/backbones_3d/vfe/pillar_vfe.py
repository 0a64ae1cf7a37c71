"""PillarVFE on libspx (reference pcdet/models/backbones_3d/vfe/pillar_vfe.py:8-123).

Same constructor signatures, config keys (`USE_ABSLOTE_XYZ` sic) and state_dict keys (`pfn_layers.<i>.linear.weight`,
`pfn_layers.<i>.norm.*`) as the reference.  Two entry modes like MeanVFE:
  * batch_dict already holds `voxels` / `voxel_num_points` / `voxel_coords` (the reference's CPU-dataloader contract);
  * batch_dict holds only `points [N, 1+C]`: the GPU voxeliser runs here from VFE.VOXELIZE; with `static_caps` in the
    batch dict it runs without a host read, rows stay at capacity and the live count goes on as a device tensor.
Two paths, both writing `pillar_features [M, C_out]`:
  * fused (default where eligible: one PFN layer, USE_NORM, 64 filters, fp32 on the GPU): spx.ops.pillar_vfe, which never
    builds the [M, T, C_out] tensor the composition passes over five times (include/spx.h §23);
  * the torch composition restating the reference's PFNLayer: every other configuration, or VFE.FUSED: False.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from spx import ops

from .vfe_template import VFETemplate


class PFNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            out_channels = out_channels // 2
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)

    def forward(self, inputs):
        x = self.linear(inputs)
        x = self.norm(x.permute(0, 2, 1)).permute(0, 2, 1) if self.use_norm else x
        x = F.relu(x)
        x_max = torch.max(x, dim=1, keepdim=True)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.repeat(1, inputs.shape[1], 1)], dim=2)


class PillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = self.model_cfg.USE_NORM
        self.with_distance = self.model_cfg.WITH_DISTANCE
        self.use_absolute_xyz = self.model_cfg.USE_ABSLOTE_XYZ
        self.num_raw_features = int(num_point_features)
        self.num_point_features = self.num_raw_features      # columns of a point after the frame index, as in MeanVFE
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1

        self.num_filters = self.model_cfg.NUM_FILTERS
        assert len(self.num_filters) > 0
        num_filters = [num_point_features] + list(self.num_filters)
        pfn_layers = []
        for i in range(len(num_filters) - 1):
            pfn_layers.append(PFNLayer(num_filters[i], num_filters[i + 1], self.use_norm,
                                       last_layer=(i >= len(num_filters) - 2)))
        self.pfn_layers = nn.ModuleList(pfn_layers)

        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_x, self.voxel_y, self.voxel_z = self.voxel_size
        self.x_offset = self.voxel_x / 2 + self.point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + self.point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + self.point_cloud_range[2]

        get = model_cfg.get if hasattr(model_cfg, 'get') else (lambda k, d=None: d)
        self.fused = get('FUSED', None)        # None: fused where eligible; True: fused or an error; False: composition
        vcfg = get('VOXELIZE', None)
        self.max_points = int(vcfg.get('MAX_POINTS_PER_VOXEL', 32)) if vcfg else 32
        mv = vcfg.get('MAX_NUMBER_OF_VOXELS', None) if vcfg else None
        mv = mv if mv is not None else {'train': 16000, 'test': 40000}
        self.max_voxels = dict(mv) if isinstance(mv, dict) else {'train': int(mv), 'test': int(mv)}

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def get_paddings_indicator(self, actual_num, max_num, axis=0):
        actual_num = torch.unsqueeze(actual_num, axis + 1)
        max_num_shape = [1] * len(actual_num.shape)
        max_num_shape[axis + 1] = -1
        max_num = torch.arange(max_num, dtype=torch.int, device=actual_num.device).view(max_num_shape)
        return actual_num.int() > max_num

    def fused_refusal(self, voxels):
        """None when spx.ops.pillar_vfe covers this configuration and input, else the reason it does not."""
        if len(self.pfn_layers) != 1 or not self.use_norm:
            return 'the fused op covers one PFN layer with USE_NORM'
        bn = self.pfn_layers[0].norm
        if self.pfn_layers[0].linear.out_features != ops.PILLAR_VFE_C_OUT:
            return 'the fused op is built for %d filters' % ops.PILLAR_VFE_C_OUT
        if not (bn.affine and bn.track_running_stats and bn.momentum is not None):
            return 'the fused op needs an affine BatchNorm1d with running statistics and a fixed momentum'
        if not (voxels.is_cuda and voxels.dtype == torch.float32 and bn.weight.dtype == torch.float32):
            return 'the fused op takes float32 tensors on the GPU'
        if torch.is_autocast_enabled():
            return 'the fused op does not run under autocast'
        if not (1 <= voxels.shape[1] <= ops.PILLAR_VFE_MAX_T and 3 <= voxels.shape[2] <= 6):
            return 'the fused op takes 1..%d points of 3..6 columns per pillar' % ops.PILLAR_VFE_MAX_T
        return None

    def point_features(self, voxel_features, voxel_num_points, coords):
        """The reference's per-point features [M, T, C_in], zero on the padding rows, term by term."""
        points_mean = voxel_features[:, :, :3].sum(dim=1, keepdim=True) \
            / voxel_num_points.type_as(voxel_features).view(-1, 1, 1)
        f_cluster = voxel_features[:, :, :3] - points_mean
        f_center = torch.zeros_like(voxel_features[:, :, :3])
        dt = voxel_features.dtype
        f_center[:, :, 0] = voxel_features[:, :, 0] - (coords[:, 3].to(dt).unsqueeze(1) * self.voxel_x + self.x_offset)
        f_center[:, :, 1] = voxel_features[:, :, 1] - (coords[:, 2].to(dt).unsqueeze(1) * self.voxel_y + self.y_offset)
        f_center[:, :, 2] = voxel_features[:, :, 2] - (coords[:, 1].to(dt).unsqueeze(1) * self.voxel_z + self.z_offset)
        if self.use_absolute_xyz:
            features = [voxel_features, f_cluster, f_center]
        else:
            features = [voxel_features[..., 3:], f_cluster, f_center]
        if self.with_distance:
            features.append(torch.norm(voxel_features[:, :, :3], 2, 2, keepdim=True))
        features = torch.cat(features, dim=-1)
        mask = self.get_paddings_indicator(voxel_num_points, features.shape[1], axis=0)
        return features * torch.unsqueeze(mask, -1).type_as(voxel_features)

    def _compose(self, voxel_features, voxel_num_points, coords):
        """The reference's forward as torch ops."""
        features = self.point_features(voxel_features, voxel_num_points, coords)
        for pfn in self.pfn_layers:
            features = pfn(features)
        return features.view(features.shape[0], -1)      # the reference's squeeze() drops the pillar axis at M == 1

    def _fused(self, voxels, num, coords, d_n):
        pfn = self.pfn_layers[0]
        bn = pfn.norm
        out, _arg, _mean, _invstd = ops.pillar_vfe(
            voxels, num, coords, pfn.linear.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var,
            bn.num_batches_tracked, bn.momentum, bn.eps, self.voxel_size, (self.x_offset, self.y_offset, self.z_offset),
            use_absolute_xyz=self.use_absolute_xyz, with_distance=self.with_distance, training=bn.training, d_n=d_n)
        return out

    def forward(self, batch_dict, **kwargs):
        d_n = None
        if 'voxels' in batch_dict:
            voxels, num, coords = batch_dict['voxels'], batch_dict['voxel_num_points'], batch_dict['voxel_coords']
            d_n = batch_dict.get('voxel_num_valid', None)
        else:
            mode = 'train' if self.training else 'test'
            static = batch_dict.get('static_caps', None) is not None      # no host read, rows at capacity
            out = ops.voxelize(batch_dict['points'], self.point_cloud_range, self.voxel_size, self.max_points,
                               self.max_voxels[mode], batch_size=int(batch_dict['batch_size']), batch_col=0, xyz_col=1,
                               feat_col=1, num_features=self.num_raw_features, want_voxels=True, want_mean=False,
                               sync=not static)
            voxels, num, coords = out['voxels'], out['num_points'], out['coords']
            if static:
                d_n = batch_dict['voxel_num_valid'] = out['d_num_voxels']
            batch_dict['voxel_coords'] = coords
            batch_dict['voxel_num_points'] = num
        why = None if self.fused is False else self.fused_refusal(voxels)
        if self.fused and why is not None:
            raise RuntimeError('PillarVFE: VFE.FUSED is set, but %s' % why)
        if self.fused is not False and why is None:
            batch_dict['pillar_features'] = self._fused(voxels, num, coords, d_n)
        else:
            if d_n is not None:
                raise RuntimeError('PillarVFE: rows at static capacity need the fused op, but %s'
                                   % (why or 'VFE.FUSED is False'))
            batch_dict['pillar_features'] = self._compose(voxels, num, coords)
        return batch_dict
