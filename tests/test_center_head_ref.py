"""The centre head without a GPU: the numpy restatement of the target assignment (tests/center_targets_ref.py) against
what the reference's assign_target_of_single_head returned (tests/golden/center_head.npz, recorded by
tests/golden/make_golden_center_head.py), bit for bit; state_dict keys, the heatmap decode and the two losses against
the reference's; CenterPoint from both yamls; the refusals (CPU tensors, circle_nms)."""
import json
import os

import numpy as np
import pytest
import torch

import center_targets_ref as ctr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFGS = os.path.join(ROOT, "tsm-det-pointcloud-_amd", "tools", "cfgs")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "center_head.npz")))


def _cfg(dataset):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    return cfg_from_yaml_file(os.path.join(CFGS, "%s_models" % dataset, "centerpoint.yaml"), AttrDict())


def _head(names_each_head, input_channels=512):
    from pcdet_amd.models.dense_heads import CenterHead
    cfg = _cfg("kitti")
    head_cfg = cfg.MODEL.DENSE_HEAD
    head_cfg.CLASS_NAMES_EACH_HEAD = names_each_head
    return CenterHead(model_cfg=head_cfg, input_channels=input_channels, num_class=3, class_names=list(cfg.CLASS_NAMES),
                      grid_size=np.array([192, 160, 40]), point_cloud_range=np.array(ctr.RANGE, np.float32),
                      voxel_size=list(ctr.VOXEL_SIZE), predict_boxes_when_training=False)


def test_cases_are_the_recorded_ones(gold):
    """The GPU tests run the restatement on cases(); the fixture holds the reference's answers for exactly those inputs."""
    cases = ctr.cases()
    assert sorted(cases) == list(gold["a/names"])
    for name, case in cases.items():
        np.testing.assert_array_equal(case["gt"], gold["a/%s/gt" % name])
        assert case["k"] == int(gold["a/%s/k" % name])
        assert [",".join(str(i) for i in ids) for ids in case["heads"]] == list(gold["a/%s/heads" % name])
    radii = ctr.check_radius_margin(cases)
    assert radii.min() < ctr.MIN_RADIUS and radii.max() >= 6        # min_radius decides somewhere; a radius >= 6 exists


@pytest.mark.parametrize("name", sorted(ctr.cases()))
def test_restatement_equals_reference_bit_for_bit(gold, name):
    case = ctr.cases()[name]
    got = ctr.assign(case["gt"], case["heads"], case["k"])
    live = 0
    for h in range(len(case["heads"])):
        for f in range(case["gt"].shape[0]):
            key = "a/%s/h%d/f%d/" % (name, h, f)
            for out in ("heatmap", "target_boxes", "inds", "mask"):
                want = gold[key + out]
                assert got[h][out][f].dtype == want.dtype and got[h][out][f].shape == want.shape, (key, out)
                assert got[h][out][f].tobytes() == want.tobytes(), (key, out)
            live += int(gold[key + "mask"].sum())
    assert live > 0


def test_case_properties(gold):
    """Each case does what it is there for, read off the reference's own outputs."""
    g = lambda name, out, h=0, f=0: gold["a/%s/h%d/f%d/%s" % (name, h, f, out)]   # noqa: E731
    hm = g("overlap", "heatmap")
    assert (hm[0] == 1).sum() == 2 and hm[0, 8, 11] > 0 and g("overlap", "inds")[2] == g("overlap", "inds")[3]
    assert hm[1, 5, 5] == 1 and hm[2, 5, 5] == 1
    assert list(g("outside", "inds")[:2]) == [19 * ctr.W, ctr.W - 1] and list(g("outside", "mask")[:2]) == [1, 1]
    assert g("corner", "inds")[0] == ctr.W * ctr.H - 1
    assert list(g("zero_dx", "mask")[:4]) == [1, 0, 1, 0] and not g("zero_dx", "target_boxes")[1].any()
    assert g("truncate", "mask").shape == (4,) and g("truncate", "mask").all()
    assert list(g("padding", "mask")[:4]) == [1, 1, 1, 0] and not g("padding", "heatmap", f=1).any()
    np.testing.assert_array_equal(g("velocity", "target_boxes")[:2, 8:10], [[1.25, -0.5], [-3.0, 0.75]])
    assert list(g("two_heads", "mask", h=0)[:3]) == [1, 1, 0] and list(g("two_heads", "mask", h=1)[:4]) == [1, 1, 1, 0]


@pytest.mark.parametrize("config", ["one_head", "two_heads"])
def test_state_dict_keys_and_shapes(config):
    from pcdet_amd.models.dense_heads import center_head
    want = json.load(open(os.path.join(GOLDEN, "center_head_state_keys.json")))[config]
    names = {"one_head": [["Car", "Pedestrian", "Cyclist"]], "two_heads": [["Car"], ["Pedestrian", "Cyclist"]]}[config]
    head = _head(names)
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == want
    for sep in head.heads_list:
        assert isinstance(sep, center_head.SeparateHead)
        assert torch.all(sep.hm[-1].bias == -2.19) and not sep.center[-1].bias.any()
    assert [m.tolist() for m in head.class_id_mapping_each_head] == ([[0, 1, 2]] if config == "one_head" else [[0], [1, 2]])
    np.testing.assert_array_equal(head.class_to_head_slot.numpy(),
                                  ctr.table_of(ctr.ONE_HEAD if config == "one_head" else ctr.TWO_HEADS, 3))


def test_decode_bbox_from_heatmap(gold):
    from pcdet_amd.models.model_utils import centernet_utils
    parts = {k[len("b/in/"):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("b/in/")}
    out = centernet_utils.decode_bbox_from_heatmap(
        point_cloud_range=np.array(ctr.RANGE, np.float32), voxel_size=list(ctr.VOXEL_SIZE), feature_map_stride=ctr.STRIDE,
        K=int(gold["b/k"]), circle_nms=False, score_thresh=float(gold["b/score_thresh"]),
        post_center_limit_range=torch.from_numpy(gold["b/limit"]), **parts)
    assert len(out) == 2
    kept = 0
    for f, d in enumerate(out):
        want = {k: gold["b/out/f%d/%s" % (f, k)] for k in ("pred_boxes", "pred_scores", "pred_labels")}
        assert d["pred_boxes"].shape == want["pred_boxes"].shape and d["pred_boxes"].shape[1] == 7
        np.testing.assert_allclose(d["pred_boxes"].numpy(), want["pred_boxes"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(d["pred_scores"].numpy(), want["pred_scores"], rtol=0, atol=1e-6)
        np.testing.assert_array_equal(d["pred_labels"].numpy(), want["pred_labels"])
        kept += len(want["pred_scores"])
    assert 8 <= kept <= 24          # "about half" of 2 x 16


def test_circle_nms_raises_by_name(gold):
    from pcdet_amd.models.model_utils import centernet_utils
    parts = {k[len("b/in/"):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("b/in/")}
    with pytest.raises(NotImplementedError, match="circle_nms"):
        centernet_utils.decode_bbox_from_heatmap(K=4, circle_nms=True, post_center_limit_range=torch.zeros(6), **parts)


def _loss_targets(gold):
    keys = [k[:-len("heatmap")] for name in ctr.LOSS_CASES for k in sorted(gold)
            if k.startswith("a/%s/h0/" % name) and k.endswith("heatmap")]
    stack = lambda out: torch.from_numpy(np.stack([gold[k + out] for k in keys]))   # noqa: E731
    return stack("heatmap").double(), stack("target_boxes").double(), stack("inds"), stack("mask")


def test_losses_match_reference_in_float64(gold):
    from pcdet_amd.utils import loss_utils
    heat, boxes, inds, mask = _loss_targets(gold)
    assert heat.shape[0] == 3 and int(mask.sum()) == 7
    logits = torch.from_numpy(gold["c/logits"]).double()
    for tag, target in (("hm", heat), ("hm_empty", torch.zeros_like(heat))):
        pred = torch.clamp(logits.sigmoid(), min=1e-4, max=1 - 1e-4).requires_grad_(True)
        loss = loss_utils.FocalLossCenterNet()(pred, target)
        loss.backward()
        np.testing.assert_allclose(loss.detach().numpy(), gold["c/%s/loss" % tag], rtol=1e-10, atol=0)
        np.testing.assert_allclose(pred.grad.numpy(), gold["c/%s/grad" % tag], rtol=1e-10, atol=1e-10)
    out = torch.from_numpy(gold["c/regs"]).double().requires_grad_(True)
    loss = loss_utils.RegLossCenterNet()(out, mask, inds, boxes)
    assert loss.shape == (8,)
    (loss * torch.from_numpy(gold["c/weights"])).sum().backward()
    np.testing.assert_allclose(loss.detach().numpy(), gold["c/reg/loss"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(out.grad.numpy(), gold["c/reg/grad"], rtol=1e-10, atol=1e-10)
    assert np.abs(gold["c/reg/grad"]).sum() > 0


@pytest.mark.parametrize("dataset", ["kitti", "waymo"])
def test_centerpoint_builds_from_yaml(dataset):
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    from pcdet_amd.models.dense_heads import AnchorHeadTemplate, CenterHead
    from pcdet_amd.models.detectors import CenterPoint
    cfg = _cfg(dataset)
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True)
    model = build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    assert isinstance(model, CenterPoint) and type(model.backbone_3d).__name__ == "VoxelResBackBone8x"
    assert isinstance(model.dense_head, CenterHead)
    assert not any(isinstance(m, AnchorHeadTemplate) for m in model.modules())
    assert [type(m).__name__ for m in model.module_list] == ["MeanVFE", "VoxelResBackBone8x", "HeightCompression",
                                                             "BaseBEVBackbone", "CenterHead"]
    head_cfg = cfg.MODEL.DENSE_HEAD
    assert head_cfg.CLASS_NAMES_EACH_HEAD == [list(cfg.CLASS_NAMES)]
    rng = ds.point_cloud_range
    assert list(head_cfg.POST_PROCESSING.POST_CENTER_LIMIT_RANGE) == [rng[0] - 5, rng[1] - 5, rng[2], rng[3] + 5, rng[4] + 5,
                                                                      rng[5]]


def test_assign_targets_refuses_cpu_tensors():
    from spx import _lib
    head = _head([["Car", "Pedestrian", "Cyclist"]], input_channels=32)
    gt = torch.from_numpy(ctr.cases()["overlap"]["gt"])
    with pytest.raises(_lib.SpxError):
        head.assign_targets(gt, feature_map_size=(ctr.H, ctr.W))
