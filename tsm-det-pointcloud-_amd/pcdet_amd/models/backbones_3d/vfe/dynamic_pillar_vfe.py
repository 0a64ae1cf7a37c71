"""DynamicPillarVFE on libspx (reference pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:14-142).

Same constructor signature, config keys (`USE_ABSLOTE_XYZ` sic) and state_dict keys (`pfn_layers.<i>.linear.weight`,
`pfn_layers.<i>.norm.*`) as the reference; nothing is moved to a device in `__init__`.  Reads `points [N, 1 + C]` =
(batch_idx, x, y, z, ...), keeps every point whose x / y cell lies on the grid (z is not tested, there are no caps) and
writes `pillar_features [M, C_out]`, `voxel_coords [M, 4]` = (b, 0, cy, cx) in torch.unique's order and `point_to_voxel
[N]` (-1 for a dropped point).  Unlike the reference, a point with a NaN coordinate or a batch index outside
[0, batch_size) is dropped: rows of batch index -1 are how a cloud is padded to a static size.
Two paths:
  * fused (default where eligible: one PFN layer, USE_NORM, 64 filters, fp32 on the GPU): spx.ops.dynamic_pillarize +
    spx.ops.dynamic_pillar_vfe, no sort, no host read inside the ops, no [N, C_out] activations (include/spx.h §24,
    DESIGN.md §6g).  With `static_caps` in the batch dict nothing is read back at all: rows stay at the capacity
    VFE.MAX_PILLARS (default: the number of point rows) and `voxel_num_valid` carries the live count;
  * the torch composition restating the reference without torch_scatter (torch.unique, index_add_, scatter_reduce_):
    every other configuration, CPU tensors, or VFE.FUSED: False.
"""
import torch
import torch.nn as nn

from spx import ops

from .vfe_template import VFETemplate


class PFNLayerV2(nn.Module):
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
        self.relu = nn.ReLU()

    def forward(self, inputs, unq_inv, num_pillars=None):
        x = self.linear(inputs)
        x = self.norm(x) if self.use_norm else x
        x = self.relu(x)
        m = int(unq_inv.max()) + 1 if num_pillars is None else int(num_pillars)
        index = unq_inv.view(-1, 1).expand_as(x)
        x_max = x.new_zeros((m, x.shape[1])).scatter_reduce_(0, index, x, 'amax', include_self=False)
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max[unq_inv, :]], dim=1)


class DynamicPillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = self.model_cfg.USE_NORM
        self.with_distance = self.model_cfg.WITH_DISTANCE
        self.use_absolute_xyz = self.model_cfg.USE_ABSLOTE_XYZ
        self.num_raw_features = int(num_point_features)
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1

        self.num_filters = self.model_cfg.NUM_FILTERS
        assert len(self.num_filters) > 0
        num_filters = [num_point_features] + list(self.num_filters)
        pfn_layers = []
        for i in range(len(num_filters) - 1):
            pfn_layers.append(PFNLayerV2(num_filters[i], num_filters[i + 1], self.use_norm,
                                         last_layer=(i >= len(num_filters) - 2)))
        self.pfn_layers = nn.ModuleList(pfn_layers)

        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.grid_size = [int(g) for g in grid_size]
        self.voxel_x, self.voxel_y, self.voxel_z = self.voxel_size
        self.x_offset = self.voxel_x / 2 + self.point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + self.point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + self.point_cloud_range[2]
        self.scale_xy = self.grid_size[0] * self.grid_size[1]
        self.scale_y = self.grid_size[1]

        get = model_cfg.get if hasattr(model_cfg, 'get') else (lambda k, d=None: d)
        self.fused = get('FUSED', None)        # None: fused where eligible; True: fused or an error; False: composition
        mp = get('MAX_PILLARS', None)          # static capacity only; None: one row per point row
        self.max_pillars = None if mp is None else int(mp)

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def fused_refusal(self, points):
        """None when spx.ops.dynamic_pillar_vfe covers this configuration and input, else the reason it does not."""
        if len(self.pfn_layers) != 1 or not self.use_norm:
            return 'the fused op covers one PFN layer with USE_NORM'
        bn = self.pfn_layers[0].norm
        if self.pfn_layers[0].linear.out_features != ops.PILLAR_VFE_C_OUT:
            return 'the fused op is built for %d filters' % ops.PILLAR_VFE_C_OUT
        if not (bn.affine and bn.track_running_stats and bn.momentum is not None):
            return 'the fused op needs an affine BatchNorm1d with running statistics and a fixed momentum'
        if not (points.is_cuda and points.dtype == torch.float32 and bn.weight.dtype == torch.float32):
            return 'the fused op takes float32 tensors on the GPU'
        if torch.is_autocast_enabled():
            return 'the fused op does not run under autocast'
        if not (points.dim() == 2 and points.shape[1] == 1 + self.num_raw_features and 3 <= self.num_raw_features <= 6):
            return 'the fused op takes points of 1 + 3..6 columns'
        return None

    def pillarize(self, points, batch_size):
        """The reference's cells and torch.unique as torch ops: (kept mask [N], cells [K, 2], unq_inv [K], voxel_coords
        [M, 4]).  The range and the voxel size are float32 constants, as the reference's tensors are."""
        lo = torch.tensor(self.point_cloud_range[:2], dtype=torch.float32, device=points.device)
        vs = torch.tensor(self.voxel_size[:2], dtype=torch.float32, device=points.device)
        grid = torch.tensor(self.grid_size[:2], dtype=torch.float32, device=points.device)
        cells = torch.floor((points[:, [1, 2]] - lo) / vs)
        mask = ((cells >= 0) & (cells < grid)).all(dim=1) & (points[:, 0] >= 0) & (points[:, 0] < batch_size)
        cells = cells[mask].int()
        merge = points[mask, 0].int() * self.scale_xy + cells[:, 0] * self.scale_y + cells[:, 1]
        unq, unq_inv = torch.unique(merge, return_inverse=True)
        unq = unq.int()
        zeros = torch.zeros_like(unq)
        coords = torch.stack((unq // self.scale_xy, zeros, unq % self.scale_y, (unq % self.scale_xy) // self.scale_y), dim=1)
        return mask, cells, unq_inv, coords

    def point_features(self, points, cells, unq_inv, num_pillars):
        """The reference's per-point features [K, C_in] of the kept points, term by term."""
        xyz = points[:, 1:4]
        cnt = torch.zeros(num_pillars, dtype=xyz.dtype, device=xyz.device).index_add_(0, unq_inv, torch.ones_like(xyz[:, 0]))
        mean = torch.zeros((num_pillars, 3), dtype=xyz.dtype, device=xyz.device).index_add_(0, unq_inv, xyz) / cnt[:, None]
        f_cluster = xyz - mean[unq_inv, :]
        f_center = torch.zeros_like(xyz)
        f_center[:, 0] = xyz[:, 0] - (cells[:, 0].to(xyz.dtype) * self.voxel_x + self.x_offset)
        f_center[:, 1] = xyz[:, 1] - (cells[:, 1].to(xyz.dtype) * self.voxel_y + self.y_offset)
        f_center[:, 2] = xyz[:, 2] - self.z_offset
        features = [points[:, 1:] if self.use_absolute_xyz else points[:, 4:], f_cluster, f_center]
        if self.with_distance:
            features.append(torch.norm(xyz, 2, dim=1, keepdim=True))
        return torch.cat(features, dim=-1)

    def _compose(self, batch_dict):
        """The reference's forward as torch ops (torch.unique reads the pillar count on the host)."""
        points = batch_dict['points']
        mask, cells, unq_inv, coords = self.pillarize(points, int(batch_dict['batch_size']))
        kept = points[mask]
        m = coords.shape[0]
        features = self.point_features(kept, cells, unq_inv, m)
        for pfn in self.pfn_layers:
            features = pfn(features, unq_inv, m)
        p2v = torch.full((points.shape[0],), -1, dtype=torch.int32, device=points.device)
        p2v[mask] = unq_inv.int()
        batch_dict['pillar_features'] = features
        batch_dict['voxel_coords'] = coords
        batch_dict['point_to_voxel'] = p2v
        return batch_dict

    def _fused(self, batch_dict, static):
        points = batch_dict['points']
        pz = ops.dynamic_pillarize(points, self.point_cloud_range, self.voxel_size, batch_size=int(batch_dict['batch_size']),
                                   batch_col=0, xyz_col=1, max_pillars=self.max_pillars if static else None,
                                   sync=not static)
        pfn = self.pfn_layers[0]
        bn = pfn.norm
        if not static and pz['num_pillars'] == 0:
            out = points.new_zeros((0, ops.PILLAR_VFE_C_OUT))
        else:
            out, _arg = ops.dynamic_pillar_vfe(
                points, pz, pfn.linear.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                bn.momentum, bn.eps, self.voxel_size, (self.x_offset, self.y_offset, self.z_offset),
                use_absolute_xyz=self.use_absolute_xyz, with_distance=self.with_distance, training=bn.training, xyz_col=1,
                num_features=self.num_raw_features)
        if static:
            batch_dict['voxel_num_valid'] = pz['d_num_pillars']
        batch_dict['pillar_features'] = out
        batch_dict['voxel_coords'] = pz['coords']
        batch_dict['point_to_voxel'] = pz['inverse']
        return batch_dict

    def forward(self, batch_dict, **kwargs):
        points = batch_dict['points']                      # (batch_idx, x, y, z, i, e)
        static = batch_dict.get('static_caps', None) is not None      # no host read, rows at capacity
        why = None if self.fused is False else self.fused_refusal(points)
        if self.fused and why is not None:
            raise RuntimeError('DynamicPillarVFE: VFE.FUSED is set, but %s' % why)
        if self.fused is not False and why is None:
            return self._fused(batch_dict, static)
        if static:
            raise RuntimeError('DynamicPillarVFE: rows at static capacity need the fused op, but %s'
                               % (why or 'VFE.FUSED is False'))
        return self._compose(batch_dict)
