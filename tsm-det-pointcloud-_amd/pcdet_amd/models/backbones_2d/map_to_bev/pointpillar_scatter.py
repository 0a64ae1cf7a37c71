"""PointPillarScatter: pillar rows -> BEV map (reference pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py:5-37).

The pillar rows are wrapped as an spx sparse tensor of spatial shape (1, ny, nx) and densified, as HeightCompression
does: libspx's densify kernel is the scatter and densify_bwd (a gather) its gradient; the values equal the reference's
per-frame `spatial_feature[:, indices] = pillars.t()` bit for bit.  The batch size comes from batch_dict['batch_size'];
the reference's `coords[:, 0].max().item()` is a host read.  The map carries the `_spx_source` tag, so BaseBEVBackbone
runs its first ZeroPad2d + Conv2d over the live pillars only."""
import torch.nn as nn

from spx.tensor import SparseConvTensor


class PointPillarScatter(nn.Module):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = self.model_cfg.NUM_BEV_FEATURES
        self.nx, self.ny, self.nz = [int(v) for v in grid_size]
        assert self.nz == 1
        self.channels_last = bool(model_cfg.get('CHANNELS_LAST', True)) if hasattr(model_cfg, 'get') else True

    def forward(self, batch_dict, **kwargs):
        pillar_features, coords = batch_dict['pillar_features'], batch_dict['voxel_coords']
        assert pillar_features.shape[1] == self.num_bev_features
        pillars = SparseConvTensor(pillar_features, coords, (self.nz, self.ny, self.nx), int(batch_dict['batch_size']),
                                   n_valid=batch_dict.get('voxel_num_valid', None),
                                   static_caps=batch_dict.get('static_caps', None))
        dense = pillars.dense(channels_last_memory=self.channels_last)
        n, c, d, h, w = dense.shape
        bev = dense.view(n, c * d, h, w)
        bev._spx_source = (pillars, bev._version)
        batch_dict['spatial_features'] = bev
        return batch_dict
