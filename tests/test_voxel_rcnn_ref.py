"""VoxelRCNNHead against the recordings of the reference's own head (tests/golden/voxel_rcnn.npz, written by
tests/golden/make_golden_voxel_rcnn.py): float64 on the CPU, the voxel query injected through the head's voxel_query_fn.
State_dict keys against voxel_rcnn_head_state_keys.json; the yaml builds a VoxelRCNN.  No GPU."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import voxel_pool_ref as vpr
import voxel_rcnn_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/voxel_rcnn_car.yaml")
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "voxel_rcnn.npz")))


def _numpy_voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, table):
    idx, empty, dens = vpr.voxel_query_bruteforce(max_range, radius, nsample, xyz.numpy(), new_xyz.numpy(),
                                                  new_coords.numpy(), table.numpy())
    return torch.from_numpy(idx), torch.from_numpy(empty), torch.from_numpy(dens).to(xyz.dtype)


def _head(grid):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads import VoxelRCNNHead
    head = VoxelRCNNHead(backbone_channels=dict(V.CHANNELS), model_cfg=AttrDict(V.head_cfg(grid)),
                         point_cloud_range=V.RANGE, voxel_size=V.VOXEL, num_class=1).double().train()
    G = _golden()
    prefix = "g%d/w/" % grid
    state = {k[len(prefix):]: torch.from_numpy(v) for k, v in G.items() if k.startswith(prefix)}
    assert list(state) == list(head.state_dict())
    head.load_state_dict(state)
    head.voxel_query_fn = _numpy_voxel_query
    return head


@pytest.mark.parametrize("grid", [2, 3])
def test_head_equals_the_reference_recordings(grid):
    G = _golden()
    levels, rois, targets = V.scene()
    head = _head(grid)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    batch = dict(batch_size=2, rois=t(rois), multi_scale_3d_strides=dict(V.STRIDES),
                 multi_scale_3d_features={k: V.sparse(v, t) for k, v in levels.items()})
    pooled = head.roi_grid_pool(batch)
    shared = head.shared_fc_layer(pooled.reshape(pooled.size(0), -1))
    rcnn_cls = head.cls_pred_layer(head.cls_fc_layers(shared))
    rcnn_reg = head.reg_pred_layer(head.reg_fc_layers(shared))
    head.forward_ret_dict = dict({k: t(v.copy()) for k, v in targets.items()}, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
    loss, tb = head.get_loss()
    loss.backward()
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in tb.values())
    for name, got in (("pooled", pooled), ("rcnn_cls", rcnn_cls), ("rcnn_reg", rcnn_reg), ("loss", loss)):
        want = G["g%d/%s" % (grid, name)]
        assert float(np.abs(got.detach().numpy() - want).max()) < TOL * max(1.0, float(np.abs(want).max())), name
    named = dict(head.named_parameters())
    for k in V.GRAD_KEYS:
        want = G["g%d/grad/%s" % (grid, k)]
        assert float(np.abs(named[k].grad.numpy() - want).max()) < TOL * max(1.0, float(np.abs(want).max())), k
    assert float(np.abs(G["g%d/grad/%s" % (grid, V.GRAD_KEYS[0])]).max()) > 0
    from pcdet_amd.ops.pointnet2.pointnet2_stack import voxel_query_utils as vq
    assert vq.voxel_query is not _numpy_voxel_query              # the injection does not outlive the call


def test_state_dict_keys_equal_the_reference():
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.models.roi_heads import VoxelRCNNHead
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    head = VoxelRCNNHead(backbone_channels=dict(V.YAML_CHANNELS), model_cfg=cfg.MODEL.ROI_HEAD,
                         point_cloud_range=[0, -40, -3, 70.4, 40, 1], voxel_size=[0.05, 0.05, 0.1], num_class=1)
    want = json.load(open(os.path.join(GOLDEN, "voxel_rcnn_head_state_keys.json")))["voxel_rcnn_car"]
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == want
    assert cfg.MODEL.ROI_HEAD.ROI_GRID_POOL.POOL_LAYERS.x_conv2.MLPS == [[32, 32]]      # the config is not edited in place


def test_yaml_builds_the_detector():
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    from pcdet_amd.models.detectors import VoxelRCNN
    from pcdet_amd.models.roi_heads import VoxelRCNNHead
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=0)
    model = build_network(cfg.MODEL, 1, ds)
    assert isinstance(model, VoxelRCNN) and isinstance(model.roi_head, VoxelRCNNHead)
    assert len(model.roi_head.roi_grid_pool_layers) == 3 and model.roi_head.shared_fc_layer[0].in_features == 216 * 96


def test_mlps_entry_of_another_length_is_refused():
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads import VoxelRCNNHead
    cfg = V.head_cfg(2)
    cfg["ROI_GRID_POOL"]["POOL_LAYERS"]["x_conv3"]["MLPS"] = [[8, 16]]
    with pytest.raises(AssertionError, match="MLPS"):
        VoxelRCNNHead(backbone_channels=dict(V.CHANNELS), model_cfg=AttrDict(cfg), point_cloud_range=V.RANGE,
                      voxel_size=V.VOXEL, num_class=1)
