"""The second stage without a GPU.  tests/golden/roi_head.npz holds what the reference's ProposalTargetLayer,
RoIHeadTemplate and SECONDHead returned in float64 (tests/golden/make_golden_roi_head.py).  Against it:
  * the numpy restatement (tests/proposal_targets_ref.py): sampled rows, assignments and labels exactly, IoUs and targets
    to 1e-10 -- the GPU tests then compare the HIP ops with this restatement on larger inputs;
  * the port's CPU composition on the same items: torch ProposalTargetLayer, assign_targets, the losses with gradients,
    generate_predicted_boxes, roi_grid_pool;
  * state_dict keys; SECONDNetIoU from second_iou.yaml; what is refused by name."""
import json
import os

import numpy as np
import pytest
import torch

import box_iou_ref as R
import proposal_targets_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd", "tools", "cfgs", "kitti_models", "second_iou.yaml")
TOL = 1e-10
EXACT = ("rois", "gt_of_rois_src", "roi_scores", "roi_labels", "reg_valid_mask")
CLOSE = ("gt_iou_of_rois", "rcnn_cls_labels", "gt_of_rois")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "roi_head.npz")))


def _names(gold):
    return [str(n) for n in gold["a/names"]]


def _case(name):
    case = P.sampling_cases()[name.replace("_clslabel", "")]
    return case, dict(case["cfg"], CLS_SCORE_TYPE="cls" if name.endswith("_clslabel") else "roi_iou")


def _cfg():
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    return cfg_from_yaml_file(YAML, AttrDict())


def _head(target_cfg=None, loss_cfg=None, pool_cfg=None):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads import SECONDHead
    head_cfg = _cfg().MODEL.ROI_HEAD
    if target_cfg is not None:
        head_cfg.TARGET_CONFIG = AttrDict(dict(target_cfg, BOX_CODER="ResidualCoder"))
    if loss_cfg is not None:
        head_cfg.LOSS_CONFIG = AttrDict(loss_cfg)
    if pool_cfg is not None:
        head_cfg.ROI_GRID_POOL = AttrDict(pool_cfg)
    if target_cfg is not None or loss_cfg is not None or pool_cfg is not None:      # the layers are not under test: small
        head_cfg.ROI_GRID_POOL.IN_CHANNEL = min(head_cfg.ROI_GRID_POOL.IN_CHANNEL, 4)
        head_cfg.SHARED_FC, head_cfg.IOU_FC = [8], [8]
    return SECONDHead(input_channels=512, model_cfg=head_cfg, num_class=1)


def _compare(got, gold, name):
    for key in EXACT:
        want = gold["a/%s/%s" % (name, key)]
        assert got[key].shape == want.shape, key
        np.testing.assert_array_equal(got[key], want, err_msg=key)
    for key in CLOSE:
        want = gold["a/%s/%s" % (name, key)]
        assert got[key].shape == want.shape, key
        assert np.abs(np.asarray(got[key], np.float64) - want).max() <= TOL, key


def test_recorded_cases_are_the_generated_ones(gold):
    names = _names(gold)
    assert sorted(n for n in names if not n.endswith("_clslabel")) == \
        sorted(n for n in P.sampling_cases() if n.startswith(("r1_", "r7_")))
    assert sum(n.endswith("_clslabel") for n in names) == 2
    seen = set()
    for name in names:        # the branches the recorded frames went through, read off the reference's own outputs
        case, cfg = _case(name)
        seen.update(P.check_input_condition(dict(case, cfg=cfg)))
    kinds = {(f > 0, h > 0, e > 0) for f, h, e in seen}
    assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, True, True)} <= kinds


def test_restatement_equals_reference(gold):
    for name in _names(gold):
        case, cfg = _case(name)
        picked = P.sample(case["rois"], case["roi_labels"], case["gt_boxes"], cfg, case["fg_keys"], case["slot_u"])
        got = P.targets(case["rois"], gold["a/%s/in_roi_scores" % name], case["roi_labels"], case["gt_boxes"], picked, cfg)
        _compare(got, gold, name)
        # the sampled rows themselves: a RoI row is unique in its frame wherever it is not the all-zero row
        for b in range(3):
            for s, row in zip(picked["sampled_inds"][b], gold["a/%s/rois" % name][b]):
                assert (case["rois"][b][s].astype(np.float64) == row).all()


def _float64_iou(a, b):
    return torch.from_numpy(R.iou3d_ref(a.numpy(), b.numpy())[0])


def _port_targets(name, gold, monkeypatch):
    from pcdet_amd.models.roi_heads.target_assigner import ProposalTargetLayer
    case, cfg = _case(name)
    monkeypatch.setattr(ProposalTargetLayer, "iou3d_fn", staticmethod(_float64_iou))
    head = _head(target_cfg=cfg)
    batch = dict(batch_size=3, rois=torch.from_numpy(case["rois"]).double(),
                 roi_scores=torch.from_numpy(gold["a/%s/in_roi_scores" % name]), roi_labels=torch.from_numpy(case["roi_labels"]),
                 gt_boxes=torch.from_numpy(case["gt_boxes"]).double(),
                 roi_sampler_rand=(torch.from_numpy(case["fg_keys"]), torch.from_numpy(case["slot_u"])))
    return head, head.assign_targets(batch)


def test_port_cpu_composition_equals_reference(gold, monkeypatch):
    for name in _names(gold):
        _, out = _port_targets(name, gold, monkeypatch)
        assert out["roi_labels"].dtype == out["reg_valid_mask"].dtype == torch.int64
        _compare({k: v.numpy() for k, v in out.items()}, gold, name)


def test_port_draws_its_own_random_numbers(monkeypatch):
    from pcdet_amd.models.roi_heads.target_assigner import ProposalTargetLayer
    case, cfg = _case("r7_m4_all_t1")
    monkeypatch.setattr(ProposalTargetLayer, "iou3d_fn", staticmethod(_float64_iou))
    head = _head(target_cfg=cfg)
    batch = dict(batch_size=3, rois=torch.from_numpy(case["rois"]).double(), roi_scores=torch.zeros(3, 7).double(),
                 roi_labels=torch.from_numpy(case["roi_labels"]), gt_boxes=torch.from_numpy(case["gt_boxes"]).double())
    torch.manual_seed(0)
    out = head.assign_targets(batch)
    assert set(out) == {"rois", "gt_of_rois", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask",
                        "rcnn_cls_labels", "gt_of_rois_src"}
    assert out["rois"].shape == (3, 4, 7) and out["gt_of_rois"].shape == (3, 4, 8)


@pytest.mark.parametrize("g", [7, 2])
def test_roi_grid_pool_restatement_and_port_equal_reference(gold, g):
    from pcdet_amd.config import AttrDict
    rois, feat, step = gold["b/rois"], gold["b/features"], gold["b/step"]
    np.testing.assert_array_equal(rois, P.pool_rois(12))
    want = gold["b/g%d/out" % g]
    assert want.shape == (24, 3, g, g) and np.abs(want).max() > 0.1
    got = P.roi_grid_pool(rois, feat, g, P.POOL["min_x"], P.POOL["min_y"], step[0], step[1])
    assert np.abs(got - want).max() <= TOL
    outside = P.taps_all_outside(rois, P.POOL["h"], P.POOL["w"], g, P.POOL["min_x"], P.POOL["min_y"], step[0], step[1])
    assert outside.any() and not outside.all() and (want[np.broadcast_to(outside[:, None], want.shape)] == 0).all()
    head = _head(pool_cfg=dict(GRID_SIZE=g, DOWNSAMPLE_RATIO=8, IN_CHANNEL=3))
    ds = AttrDict(POINT_CLOUD_RANGE=[P.POOL["min_x"], P.POOL["min_y"], -3, 2.8, 1.0, 1],
                  DATA_PROCESSOR=[dict(NAME="x", VOXEL_SIZE=[0.05, 0.1, 0.1])])
    before = torch.backends.cudnn.enabled
    out = head.roi_grid_pool(dict(batch_size=2, rois=torch.from_numpy(rois).double(),
                                  spatial_features_2d=torch.from_numpy(feat).double(), dataset_cfg=ds))
    assert torch.backends.cudnn.enabled == before
    assert out.dtype == torch.float64 and np.abs(out.numpy() - want).max() <= TOL
    cl = torch.from_numpy(feat).double().contiguous(memory_format=torch.channels_last)
    out_cl = head.roi_grid_pool(dict(batch_size=2, rois=torch.from_numpy(rois).double(), spatial_features_2d=cl,
                                     dataset_cfg=ds))
    assert np.abs(out_cl.numpy() - want).max() <= TOL


def _focal_ref(x, t, gamma=2.0, alpha=0.25):
    p = 1 / (1 + np.exp(-x))
    bce = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
    return (t * alpha + (1 - t) * (1 - alpha)) * (t * (1 - p) + (1 - t) * p) ** gamma * bce


@pytest.mark.parametrize("kind", ["BinaryCrossEntropy", "L2", "smoothL1", "focalbce"])
def test_iou_loss_kinds(gold, kind):
    head = _head(loss_cfg=dict(IOU_LOSS=kind, LOSS_WEIGHTS={"rcnn_iou_weight": 1.5, "code_weights": [1.0] * 7}))
    x = torch.from_numpy(gold["c/logits"]).requires_grad_(True)
    labels = gold["c/labels"]
    loss, tb = head.get_box_iou_layer_loss(dict(rcnn_iou=x, rcnn_cls_labels=torch.from_numpy(labels)))
    loss.backward()
    assert isinstance(tb["rcnn_loss_iou"], torch.Tensor) and tb["rcnn_loss_iou"].dim() == 0
    if kind == "focalbce":      # not defined by the reference: the sigmoid focal loss, gamma 2, alpha 0.25
        want = 1.5 * _focal_ref(gold["c/logits"][:, 0], labels).mean()
        assert abs(loss.item() - want) <= TOL and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    else:
        assert abs(loss.item() - float(gold["c/%s/loss" % kind])) <= TOL
        assert np.abs(x.grad.numpy() - gold["c/%s/grad" % kind]).max() <= TOL


def _loss_head():
    weights = {"rcnn_cls_weight": 1.25, "rcnn_reg_weight": 0.75, "rcnn_corner_weight": 2.0, "code_weights": [1.0] * 7}
    return _head(loss_cfg=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
                               LOSS_WEIGHTS=weights))


def _recorded_targets(gold, name):
    return {k: torch.from_numpy(gold["a/%s/%s" % (name, k)]) for k in EXACT + CLOSE}


def test_box_losses_and_decoding_equal_reference(gold):
    head = _loss_head()
    tgt = _recorded_targets(gold, str(gold["d/case"]))
    assert 0 < tgt["reg_valid_mask"].sum() < tgt["reg_valid_mask"].numel()      # fg rows and masked rows
    x = torch.from_numpy(gold["d/rcnn_reg"]).requires_grad_(True)
    loss, tb = head.get_box_reg_layer_loss(dict(tgt, rcnn_reg=x))
    loss.backward()
    assert abs(loss.item() - float(gold["d/reg/loss"])) <= TOL
    assert abs(tb["rcnn_loss_corner"].item() - float(gold["d/reg/corner"])) <= TOL
    assert np.abs(x.grad.numpy() - gold["d/reg/grad"]).max() <= TOL
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in tb.values())
    x = torch.from_numpy(gold["d/rcnn_cls"]).requires_grad_(True)
    loss, _ = head.get_box_cls_layer_loss(dict(tgt, rcnn_cls=x))
    loss.backward()
    assert abs(loss.item() - float(gold["d/cls_bce/loss"])) <= TOL
    assert np.abs(x.grad.numpy() - gold["d/cls_bce/grad"]).max() <= TOL
    head.model_cfg.LOSS_CONFIG.CLS_LOSS = "CrossEntropy"
    hard = torch.from_numpy(gold["a/r7_m4_cls_t1_clslabel/rcnn_cls_labels"]).view(-1)
    assert set(hard.tolist()) >= {0, 1}
    x = torch.from_numpy(gold["d/rcnn_cls3"][:hard.numel()]).requires_grad_(True)
    loss, _ = head.get_box_cls_layer_loss(dict(rcnn_cls=x, rcnn_cls_labels=hard))
    loss.backward()
    assert abs(loss.item() - float(gold["d/cls_ce/loss"])) <= TOL
    assert np.abs(x.grad.numpy() - gold["d/cls_ce/grad"]).max() <= TOL
    cls_out, box_out = head.generate_predicted_boxes(batch_size=3, rois=tgt["rois"], cls_preds=torch.from_numpy(gold["d/rcnn_cls"]),
                                                     box_preds=torch.from_numpy(gold["d/rcnn_reg"]))
    np.testing.assert_array_equal(cls_out.numpy(), gold["d/decode/cls"])
    assert np.abs(box_out.numpy() - gold["d/decode/boxes"]).max() <= TOL


def test_corner_loss_without_fg_rows_is_zero_with_finite_gradients(gold):
    head = _loss_head()
    tgt = _recorded_targets(gold, str(gold["d/case"]))
    tgt["reg_valid_mask"] = torch.zeros_like(tgt["reg_valid_mask"])
    x = (torch.from_numpy(gold["d/rcnn_reg"]) * 500).requires_grad_(True)      # exp(100) in the size decode of a masked row
    loss, tb = head.get_box_reg_layer_loss(dict(tgt, rcnn_reg=x))
    loss.backward()
    assert loss.item() == 0 and tb["rcnn_loss_corner"].item() == 0 and torch.isfinite(x.grad).all()


def test_state_dict_keys_equal_reference():
    want = json.load(open(os.path.join(GOLDEN, "roi_head_state_keys.json")))["second_iou"]
    head = _head()
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == want
    assert want[0] == ["shared_fc_layer.0.weight", [256, 512 * 49, 1]]


def _dataset(cfg):
    from pcdet_amd.datasets import SyntheticDataset
    return SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=0)


def test_second_iou_builds_from_yaml():
    from pcdet_amd.models import build_network
    from pcdet_amd.models.detectors import SECONDNetIoU
    from pcdet_amd.models.roi_heads import SECONDHead
    cfg = _cfg()
    ds = _dataset(cfg)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    assert isinstance(model, SECONDNetIoU) and isinstance(model.roi_head, SECONDHead)
    assert model.module_list[-1] is model.roi_head and model.dense_head.predict_boxes_when_training
    assert model.roi_head.num_class == 1                      # CLASS_AGNOSTIC
    # the dataset_cfg the head reads is the geometry the model is built on, not the yaml's KITTI range
    assert ds.dataset_cfg.POINT_CLOUD_RANGE[:2] == [0.0, -8.0] and ds.dataset_cfg.DATA_PROCESSOR[-1].VOXEL_SIZE == [0.05, 0.05, 0.1]
    assert cfg.DATA_CONFIG.POINT_CLOUD_RANGE[1] == -40          # the caller's config is not written to


def test_other_roi_heads_and_options_are_refused_by_name():
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models import build_network
    cfg = _cfg()
    ds = _dataset(cfg)
    cfg.MODEL.ROI_HEAD.NAME = "PVRCNNHead"
    with pytest.raises(NotImplementedError, match="PVRCNNHead"):
        build_network(cfg.MODEL, 3, ds)
    head = _head()
    boxes = dict(batch_size=1, batch_box_preds=torch.zeros(1, 4, 7), batch_cls_preds=torch.zeros(1, 4, 3))
    nms = AttrDict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=True, NMS_PRE_MAXSIZE=4, NMS_POST_MAXSIZE=2, NMS_THRESH=0.5)
    with pytest.raises(NotImplementedError, match="MULTI_CLASSES_NMS"):
        head.proposal_layer(dict(boxes), nms)
    nms.MULTI_CLASSES_NMS, nms.NMS_POST_MAXSIZE = False, [2, 2]
    with pytest.raises(NotImplementedError, match="NMS_POST_MAXSIZE"):
        head.proposal_layer(dict(boxes), nms)
    cfg = _cfg()
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.SCORE_TYPE = "num_pts_iou_cls"
    model = build_network(cfg.MODEL, 3, ds)
    batch = dict(batch_size=1, batch_box_preds=torch.zeros(1, 4, 7), batch_cls_preds=torch.zeros(1, 4, 1),
                 roi_scores=torch.zeros(1, 4), roi_labels=torch.ones(1, 4, dtype=torch.long), has_class_labels=True,
                 cls_preds_normalized=False)
    with pytest.raises(NotImplementedError, match="num_pts_iou_cls"):
        model.post_processing(batch)


def test_score_by_class_covers_every_class():
    """A frame without class 1: the reference's range(len(unique(labels))) would leave class 3 at score 0."""
    from pcdet_amd.models import build_network
    cfg = _cfg()
    model = build_network(cfg.MODEL, 3, _dataset(cfg))
    iou, cls = torch.tensor([0.9, 0.8, 0.7]), torch.tensor([0.1, 0.2, 0.3])
    got = model.set_nms_score_by_class(iou, cls, torch.tensor([2, 3, 3]), {"Car": "iou", "Pedestrian": "cls", "Cyclist": "iou"})
    assert got.tolist() == pytest.approx([0.1, 0.8, 0.7])


def test_small_additions():
    from pcdet_amd.utils import common_utils, loss_utils
    pts = torch.tensor([[[1.0, 0.0, 5.0, 9.0]]], dtype=torch.float64)
    out = common_utils.rotate_points_along_z(pts, torch.tensor([np.pi / 2], dtype=torch.float64))
    assert out.dtype == torch.float64 and np.allclose(out.numpy(), [[[0, 1, 5, 9]]], atol=1e-7)
    box = torch.tensor([[1.0, 2.0, 3.0, 4.0, 2.0, 1.5, 0.3]], dtype=torch.float64)
    flipped = box.clone()
    flipped[:, 6] += np.pi
    assert loss_utils.get_corner_loss_lidar(box, flipped).abs().max() <= 1e-6      # a box turned by pi is the same box
    assert loss_utils.get_corner_loss_lidar(box, box + 0.5).item() > 0.1
