"""VoxelSetAbstraction, PointHeadSimple and PVRCNNHead against the recordings of the reference's own modules
(tests/golden/pv_rcnn.npz, written by tests/golden/make_golden_pv_rcnn.py): float64 on the CPU, the device ops replaced
by their restatements (pv_rcnn_ref.cpu_ops).  Keypoints and labels exactly, everything else to 1e-10.  State_dict keys
against pv_rcnn_state_keys.json; the yaml builds a PVRCNN; the refusals; the batched BEV interpolation against the
reference's per-frame function on a map where every clamp edge is hit.  No GPU."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import pv_rcnn_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/pv_rcnn.yaml")
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "pv_rcnn.npz")))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _close(got, want, what):
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, what
    assert float(np.abs(got - want).max()) <= TOL * max(1.0, float(np.abs(want).max())), what


def _load(module, prefix):
    G = _golden()
    state = {k[len(prefix):]: torch.from_numpy(v) for k, v in G.items() if k.startswith(prefix)}
    assert list(state) == list(module.state_dict())
    module.load_state_dict(state)
    return module


def _front():
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.backbones_3d.pfe import VoxelSetAbstraction
    from pcdet_amd.models.dense_heads import PointHeadSimple
    vsa = VoxelSetAbstraction(model_cfg=AttrDict(V.pfe_cfg()), voxel_size=V.VOXEL, point_cloud_range=V.RANGE,
                              num_bev_features=V.BEV_CHANNELS, num_rawpoint_features=V.NUM_RAWPOINT_FEATURES)
    head = PointHeadSimple(num_class=1, input_channels=vsa.num_point_features_before_fusion,
                           model_cfg=AttrDict(V.point_head_cfg()))
    return _load(vsa.double().train(), "w/vsa/"), _load(head.double().train(), "w/point/")


def test_pfe_and_point_head_equal_the_reference_recordings():
    G = _golden()
    vsa, head = _front()
    with V.cpu_ops():
        batch = head(vsa(V.batch_of(V.scene(), _t)))
    loss, tb = head.get_loss()
    assert np.array_equal(batch["point_coords"].numpy(), G["keypoints"])                 # exactly
    assert np.array_equal(head.forward_ret_dict["point_cls_labels"].numpy(), G["point_cls_labels"])
    assert set(np.unique(G["point_cls_labels"])) == {-1, 0, 1}
    _close(batch["point_features_before_fusion"], G["point_features_before_fusion"], "before fusion")
    _close(batch["point_features"], G["point_features"], "point_features")
    _close(batch["point_cls_scores"], G["point_cls_scores"], "scores")
    _close(loss, G["point_loss"], "point loss")
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in tb.values()) and "point_loss_cls" in tb
    assert batch["pfe_layout_ok"].dim() == 0 and bool(batch["pfe_layout_ok"])
    # frame 1 holds 20 points: its 32 keypoints are its 20 picks, repeated cyclically
    kp = batch["point_coords"].numpy()[V.NUM_KEYPOINTS:]
    assert (kp[:, 0] == 1).all() and np.array_equal(kp[20:], kp[:12]) and len(np.unique(kp[:20], axis=0)) == 20


@pytest.mark.parametrize("grid", [2, 3])
def test_roi_head_equals_the_reference_recordings(grid):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads import PVRCNNHead
    G = _golden()
    sc = V.scene()
    head = _load(PVRCNNHead(input_channels=16, model_cfg=AttrDict(V.roi_head_cfg(grid)), num_class=1).double().train(),
                 "g%d/w/" % grid)
    kp = G["keypoints"]
    batch = dict(batch_size=2, rois=_t(sc["rois"]), point_coords=_t(kp), point_features=_t(G["point_features"]),
                 point_cls_scores=_t(G["point_cls_scores"]))
    with V.cpu_ops():
        pooled = head.roi_grid_pool(batch)
    n = pooled.shape[0]
    shared = head.shared_fc_layer(pooled.permute(0, 2, 1).contiguous().view(n, -1, 1))
    rcnn_cls = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
    rcnn_reg = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
    head.forward_ret_dict = dict({k: _t(v.copy()) for k, v in sc["targets"].items()}, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
    loss, tb = head.get_loss()
    loss.backward()
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in tb.values())
    for name, got in (("pooled", pooled), ("rcnn_cls", rcnn_cls), ("rcnn_reg", rcnn_reg), ("loss", loss)):
        _close(got, G["g%d/%s" % (grid, name)], name)
    named = dict(head.named_parameters())
    for k in V.ROI_GRAD_KEYS:
        _close(named[k].grad, G["g%d/grad/%s" % (grid, k)], k)
    assert float(np.abs(G["g%d/grad/%s" % (grid, V.ROI_GRAD_KEYS[0])]).max()) > 0


def test_state_dict_keys_equal_the_reference():
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.models.backbones_3d.pfe import VoxelSetAbstraction
    from pcdet_amd.models.dense_heads import PointHeadSimple
    from pcdet_amd.models.roi_heads import PVRCNNHead
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    want = json.load(open(os.path.join(GOLDEN, "pv_rcnn_state_keys.json")))
    vsa = VoxelSetAbstraction(model_cfg=cfg.MODEL.PFE, **V.YAML_KW)
    point = PointHeadSimple(num_class=1, input_channels=vsa.num_point_features_before_fusion,
                            model_cfg=cfg.MODEL.POINT_HEAD)
    roi = PVRCNNHead(input_channels=vsa.num_point_features, model_cfg=cfg.MODEL.ROI_HEAD, num_class=1)
    for name, m in (("pfe", vsa), ("point_head", point), ("roi_head", roi)):
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want[name], name
    assert vsa.num_point_features == 128
    assert vsa.num_point_features_before_fusion == want["num_point_features_before_fusion"] == 640
    assert cfg.MODEL.PFE.SA_LAYER.x_conv2.MLPS == [[32, 32], [32, 32]]            # the config is not edited in place
    assert cfg.MODEL.ROI_HEAD.ROI_GRID_POOL.MLPS == [[64, 64], [64, 64]]
    assert all(not m.fused for m in vsa.sa_modules()) == (not cfg.MODEL.PFE.get("FUSED", vsa.sa_modules()[0].fused))


def test_yaml_builds_the_detector():
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    from pcdet_amd.models.detectors import PVRCNN
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=0)
    model = build_network(cfg.MODEL, 3, ds)
    assert isinstance(model, PVRCNN)
    assert [type(m).__name__ for m in model.module_list] == [
        "MeanVFE", "VoxelBackBone8x", "HeightCompression", "VoxelSetAbstraction", "BaseBEVBackbone", "AnchorHeadSingle",
        "PointHeadSimple", "PVRCNNHead"]
    assert model.point_head.cls_layers[0].in_features == 640 and model.roi_head.shared_fc_layer[0].in_channels == 216 * 128
    assert model.roi_head.num_class == 1 and model.point_head.num_class == 1 and model.dense_head.num_class == 3
    for flag in (True, False):
        cfg2 = cfg_from_yaml_file(YAML, AttrDict())
        cfg2.MODEL.PFE.FUSED = flag
        cfg2.MODEL.ROI_HEAD.ROI_GRID_POOL.FUSED = flag
        m2 = build_network(cfg2.MODEL, 3, ds)
        assert all(layer.fused is flag for layer in m2.pfe.sa_modules()) and m2.roi_head.roi_grid_pool_layer.fused is flag


def test_refusals_by_name():
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    from pcdet_amd.models.backbones_3d.pfe import VoxelSetAbstraction
    kw = dict(voxel_size=V.VOXEL, point_cloud_range=V.RANGE, num_bev_features=V.BEV_CHANNELS,
              num_rawpoint_features=V.NUM_RAWPOINT_FEATURES)
    with pytest.raises(NotImplementedError, match="SPC"):
        VoxelSetAbstraction(model_cfg=AttrDict(V.pfe_cfg(SAMPLE_METHOD="SPC")), **kw)
    cfg = V.pfe_cfg()
    cfg["SA_LAYER"]["x_conv3"]["FILTER_NEIGHBOR_WITH_ROI"] = True
    with pytest.raises(NotImplementedError, match="FILTER_NEIGHBOR_WITH_ROI"):
        VoxelSetAbstraction(model_cfg=AttrDict(cfg), **kw)
    cfg = V.pfe_cfg()
    cfg["SA_LAYER"]["x_conv4"]["NAME"] = "VectorPoolAggregationModuleMSG"
    with pytest.raises(NotImplementedError, match="VectorPoolAggregationModuleMSG"):
        VoxelSetAbstraction(model_cfg=AttrDict(cfg), **kw)
    # a static-capacity sparse tensor
    vsa, _ = _front()
    batch = V.batch_of(V.scene(), _t)
    batch["multi_scale_3d_features"]["x_conv4"].n_valid = torch.tensor(7)
    with V.cpu_ops(), pytest.raises(NotImplementedError, match="static-capacity.*x_conv4"):
        vsa(batch)
    # PVRCNNHead without a PFE
    full = cfg_from_yaml_file(YAML, AttrDict())
    ds = SyntheticDataset(full.DATA_CONFIG, full.CLASS_NAMES, True, cfg_id=0)
    del full.MODEL["PFE"]
    full.MODEL.POINT_HEAD = None
    with pytest.raises(NotImplementedError, match=r"PVRCNNHead.*MODEL\.PFE"):
        build_network(full.MODEL, 3, ds)
    # target options the point head does not use
    _, head = _front()
    pts, gt = torch.zeros(4, 4, dtype=torch.float64), torch.zeros(2, 1, 8, dtype=torch.float64)
    for kwargs, name in ((dict(ret_box_labels=True), "ret_box_labels"), (dict(ret_part_labels=True), "ret_part_labels"),
                         (dict(set_ignore_flag=False, use_ball_constraint=True), "use_ball_constraint")):
        with pytest.raises(NotImplementedError, match=name):
            head.assign_stack_targets(pts, gt, gt, **kwargs)


def test_shuffled_cloud_clears_the_layout_flag():
    vsa, _ = _front()
    batch = V.batch_of(V.scene(), _t)
    batch["points"] = batch["points"].flip(0).contiguous()
    with V.cpu_ops():
        out = vsa(batch)
    assert out["pfe_layout_ok"].dim() == 0 and not bool(out["pfe_layout_ok"])


def test_bev_interpolation_equals_the_reference_function_at_every_clamp_edge():
    from pcdet_amd.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    vsa, _ = _front()
    rng = np.random.default_rng(3)
    h, w, stride = 5, 7, 4
    bev = torch.from_numpy(rng.normal(size=(2, V.BEV_CHANNELS, h, w))).requires_grad_(True)
    # map coordinates: x < 0, x >= W - 1, y < 0, y >= H - 1, integers, and the interior
    xs = np.array([-1.3, -0.2, 0.0, 1.0, 2.5, 5.0, 6.0, 6.4, 7.9, 3.0, 3.3, -0.5, 6.0])
    ys = np.array([2.2, -0.7, 0.0, 3.0, -1.5, 4.0, 4.0, 4.6, 5.5, 1.0, 2.7, 4.2, -0.1])
    assert (xs < 0).any() and (xs >= w - 1).any() and (ys < 0).any() and (ys >= h - 1).any()
    assert ((xs == np.floor(xs)) & (ys == np.floor(ys))).any()
    frame = np.arange(len(xs)) % 2
    order = np.argsort(frame, kind="stable")
    xs, ys, frame = xs[order], ys[order], np.sort(frame)
    scale = np.array(V.VOXEL[:2]) * stride
    kp = np.stack([frame, xs * scale[0] + V.RANGE[0], ys * scale[1] + V.RANGE[1], np.zeros_like(xs)], 1)
    with V.cpu_ops():
        got = vsa.interpolate_from_bev_features(_t(kp), bev, 2, stride)
    got.sum().backward()
    grad = bev.grad.clone()
    bev.grad = None
    # the reference's own loop over frames
    kpt = _t(kp)
    x_idxs = (kpt[:, 1] - V.RANGE[0]) / V.VOXEL[0] / stride
    y_idxs = (kpt[:, 2] - V.RANGE[1]) / V.VOXEL[1] / stride
    want = torch.cat([vsa_mod.bilinear_interpolate_torch(bev[k].permute(1, 2, 0), x_idxs[kpt[:, 0] == k],
                                                         y_idxs[kpt[:, 0] == k]) for k in range(2)])
    want.sum().backward()
    _close(got, want.detach().numpy(), "bev")
    _close(grad, bev.grad.numpy(), "bev grad")
    assert float(got.detach().abs().max()) > 0
