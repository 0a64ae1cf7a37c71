"""tests/anchor_head_ref.py (the plain references the GPU tests of csrc/assign.hip and csrc/anchor_loss.hip compare with)
against what the reference project computed (tests/golden/anchor_head_edges.npz, tests/golden/ref_modules.npz) and against
this project's torch formulations, on the CPU.  Also: the conditions that make the edge inputs meaningful (forced
positives, ties, ignored anchors, no IoU near a threshold), and the host-side argument checks of the two entry points."""
import ctypes

import numpy as np
import pytest
import torch

import anchor_head_ref as ahr
import point_loss_ref as plr

ASSIGN_CASES = ("fixture",) + ahr.SYNTH_CASES


def _ref(name):
    return ahr.fixture_ref() if name == "fixture" else ahr.synth_ref(name)


def _torch_assigner(case):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner
    from pcdet_amd.utils.box_coder_utils import ResidualCoder
    cfg = AttrDict(ANCHOR_GENERATOR_CONFIG=[{"class_name": n, "matched_threshold": m, "unmatched_threshold": u}
                                            for n, m, u in zip(case["set_names"], case["matched"], case["unmatched"])],
                   TARGET_ASSIGNER_CONFIG=AttrDict(POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False))
    return AxisAlignedTargetAssigner(cfg, list(case["class_names"]), ResidualCoder(), match_height=False)


def _torch_assign(name, m=8):
    if name == "fixture":
        head = ahr.fixture_head()
        return head.target_assigner.assign_targets_torch(head.anchors, torch.from_numpy(ahr.fixture_edge_batch(m)))
    case = ahr.synth_case(name)
    anchors = [torch.from_numpy(a.copy())[None, None, :, None] for a in case["anchor_sets"]]
    return _torch_assigner(case).assign_targets_torch(anchors, torch.from_numpy(case["gt"].copy()))


# ---------------------------------------------------------------------------------------------------- assignment

@pytest.mark.parametrize("name", ASSIGN_CASES)
def test_assign_ref_matches_recorded_reference(name):
    g, ref = ahr.golden(), _ref(name)
    key = name if name == "fixture" else "synth_" + name
    assert np.array_equal(ref["labels"], g[key + "_labels"])
    assert np.array_equal(ref["weights"], g[key + "_weights"])
    pos = ref["targets"][ref["labels"] > 0]
    assert pos.shape == g[key + "_pos_targets"].shape
    if pos.size:
        assert np.abs(pos - g[key + "_pos_targets"]).max() < 1e-6
    assert not ref["targets"][ref["labels"] <= 0].any()


@pytest.mark.parametrize("name", ASSIGN_CASES + ("fixture_m257",))
def test_assign_ref_matches_torch_formulation(name):
    ref = ahr.fixture_ref(257) if name == "fixture_m257" else _ref(name)
    got = _torch_assign("fixture", 257) if name == "fixture_m257" else _torch_assign(name)
    assert np.array_equal(got["box_cls_labels"].numpy(), ref["labels"])
    assert np.array_equal(got["reg_weights"].numpy(), ref["weights"])
    assert np.abs(got["box_reg_targets"].numpy() - ref["targets"]).max() < 1e-6


def test_assign_ref_matches_ref_modules_labels():
    g = ahr.modules()
    ref = ahr.assign_ref(ahr.fixture_anchor_sets(), ahr.CLASS_NAMES, ahr.CLASS_NAMES, ahr.FIXTURE_MATCHED,
                         ahr.FIXTURE_UNMATCHED, g["head_gt"])
    assert np.array_equal(ref["labels"], g["head_box_cls_labels"])
    assert np.array_equal(ref["weights"], g["head_reg_weights"])
    assert np.abs(ref["targets"] - g["head_box_reg_targets"]).max() < 1e-6
    assert np.array_equal(ahr.fixture_ref()["labels"][:2], g["head_box_cls_labels"])   # padding to M = 8 changes nothing
    assert np.array_equal(ahr.fixture_ref(257)["labels"], ahr.fixture_ref()["labels"])


def test_fixture_batch_conditions():
    """What makes the five-frame batch worth running: forced positives below the matched threshold, ignored anchors,
    frames without a positive, and no decision that float32 rounding could flip."""
    ref = ahr.fixture_ref()
    labels = ref["labels"]
    matched = np.tile(np.repeat(np.array(ahr.FIXTURE_MATCHED), 2), labels.shape[1] // 6)[None, :]
    assert (ref["forced"] & (labels > 0) & (ref["max_iou"] < matched)).sum() >= 1
    assert (labels == -1).sum() >= 1
    pos = (labels > 0).sum(axis=1)
    print("positives per frame", pos, "ignored per frame", (labels == -1).sum(axis=1))
    assert (pos[:3] > 0).all() and pos[3] == 0 and pos[4] == 0
    assert not labels[3:].any()
    assert ahr.threshold_margin(ref, ahr.FIXTURE_MATCHED, ahr.FIXTURE_UNMATCHED, 3, 2) > 1e-5
    assert ref["max_iou"][2].max() == 1.0                                     # the gt equal to an anchor
    # frame 3: its box overlaps nothing, so nothing is forced although the frame has a gt of the Car set's class
    assert ref["iou"][3][0].shape[1] == 1 and ref["iou"][3][0].max() == 0 and not ref["forced"][3].any()


def test_synthetic_case_conditions():
    # M = 256: row 255 is the only gt of set 0's class and is found
    ref, case = ahr.synth_ref("last_row"), ahr.synth_case("last_row")
    lab = ref["labels"].reshape(3, -1, 2, 2)
    assert ref["iou"][0][0].shape[1] == 1 and ref["iou"][1][0].shape[1] == 1 and ref["iou"][0][1].shape[1] == 255
    assert (lab[0, :, 0] == 1).sum() >= 1 and (lab[1, :, 0] == 1).sum() >= 1 and (lab[0, :, 1] == 2).sum() >= 1
    assert not lab[2].any() and not lab[1, :, 1].any()
    # exact tie: both neighbours forced, neither reaches the matched threshold
    ref = ahr.synth_ref("tie")
    assert ref["forced_per_gt"][0][0].tolist() == [2]
    assert ref["labels"][0].tolist() == [0, 0, 1, 1, 0, 0] and ref["max_iou"][0, 2] < 0.75
    # first argmax: rows 2 and 4 have one footprint; the targets are those of row 2
    ref, case = ahr.synth_ref("first_argmax"), ahr.synth_case("first_argmax")
    iou = ref["iou"][0][0]
    assert iou.shape[1] == 2 and np.array_equal(iou[:, 0], iou[:, 1]) and ref["labels"][0, 0] == 1
    an, gt = case["anchor_sets"][0].reshape(-1, 7), case["gt"][0]
    assert np.array_equal(ref["targets"][0, 0], ahr.encode64(gt[2:3, :7], an[0:1])[0])
    assert np.abs(ref["targets"][0, 0] - ahr.encode64(gt[4:5, :7], an[0:1])[0]).max() > 0.5
    # thresholds equal to the IoU's bit pattern: >= matched holds (set 0), < unmatched does not (set 1: ignored)
    ref = ahr.synth_ref("threshold")
    lab = ref["labels"].reshape(3, 256, 2)
    f32 = ahr._iou(ahr.aligned_bev32(ahr.synth_case("threshold")["anchor_sets"][0].reshape(-1, 7)[40:42]),
                   ahr.aligned_bev32(ahr.synth_case("threshold")["gt"][0, :1, :7]), np.float32)
    assert f32[0, 0] == f32[1, 0] == ahr.IOU_THIRD
    assert not ref["forced"].reshape(3, 256, 2)[:, 40:42].any()
    assert lab[0, 40:42, 0].tolist() == [1, 1] and lab[2, 40:42, 0].tolist() == [1, 1]
    assert lab[1, 40:42, 1].tolist() == [-1, -1] and lab[2, 40:42, 1].tolist() == [-1, -1]
    assert lab[0, 200, 0] == 1 and lab[1, 200, 1] == 2
    # geometry: the zero-size box gives no positive, the cancelling last row is padding, headings next to pi/4 swap
    ref, case = ahr.synth_ref("geometry"), ahr.synth_case("geometry")
    assert case["gt"][0, 3, :7].sum() == 0 and case["gt"][0, 3, :7].any()
    assert ref["iou"][0][0].shape[1] == 2 and ref["iou"][0][0][:, 0].max() == 0
    lab = ref["labels"].reshape(3, 85, 2, 6)
    assert not lab[0, 3:6].any()                                              # kept, row 3 would match the anchors at x = 4
    iou = ref["iou"][1][0]                                                    # columns: the six class-1 boxes of frame 1
    assert iou[:, 3].max() == 1.0 and iou[:, 4].max() == 1.0 and iou[:, 5].max() == 1.0
    assert iou[:, 3].argmax() % 6 == 0 and iou[:, 4].argmax() % 6 == 1 and iou[:, 5].argmax() % 6 == 1
    assert not lab[2].any() and not ahr.synth_ref("not_owned")["labels"].any()
    for name in ahr.SYNTH_CASES:                                              # nothing within 1e-5 of a threshold, except
        if name != "threshold":                                              # where the threshold IS the IoU's value
            c = ahr.synth_case(name)
            assert ahr.threshold_margin(ahr.synth_ref(name), c["matched"], c["unmatched"], len(c["anchor_sets"]),
                                        c["per_location"]) > 1e-5, name


# --------------------------------------------------------------------------------------------------------- losses

def _close(got, want, rel):
    return np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("name", sorted(ahr.LOSS_CASES))
def test_loss_ref_matches_recorded_reference(name):
    g = ahr.golden()
    losses, dcls, dbox, ddir = ahr.loss_case_ref(name)
    assert _close(losses, g["loss_%s_losses" % name], 1e-12)
    c = ahr.loss_case(name)
    if c["labels"].size <= ahr.GOLDEN_GRAD_ROWS:
        assert _close(dcls, g["loss_%s_dcls" % name], 1e-12) and _close(dbox, g["loss_%s_dbox" % name], 1e-12)
        if ddir is not None:
            assert _close(ddir, g["loss_%s_ddir" % name], 1e-12)
    assert all(np.isfinite(x).all() for x in (losses, dcls, dbox))
    # elements the reference gives no weight: exact zeros
    assert not dcls[c["labels"] < 0].any() and not dbox[c["labels"] <= 0].any()
    assert not dbox[np.isnan(c["targets"])].any()
    assert ddir is None or not ddir[c["labels"] <= 0].any()


@pytest.mark.parametrize("name", sorted(ahr.LOSS_CASES))
def test_loss_ref_matches_torch_composition_in_float64(name):
    """The project's get_cls_layer_loss / get_box_reg_layer_loss in float64 (bound to the case's tensors the way the GPU
    test binds them in float32) give loss_ref's numbers.  The composition keeps its anchor weights (1 / #positives) in
    float32 whatever the predictions' type, one rounding of 6e-8 relative per weight, hence 5e-7."""
    c = ahr.loss_case(name)
    want = ahr.run_loss_ref(c)
    got = ahr.torch_losses(c, torch.float64, "cpu")
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert _close(a, b, 5e-7)


def test_loss_case_contents():
    g = ahr.golden()
    assert bool(g["nan_heading_reference_is_nan"])
    seen_nc, seen_nb, seen_a, seen_b, seen_beta = set(), set(), set(), set(), set()
    for name, (B, A, NC, NB, beta, weights, _off) in ahr.LOSS_CASES.items():
        c = ahr.loss_case(name)
        seen_nc.add(NC), seen_nb.add(NB), seen_a.add(A), seen_b.add(B), seen_beta.add(beta)
        assert c["labels"].min() >= -1 and c["labels"].max() <= NC
        if NB is not None and not name.startswith("boundary"):                # mid-bin: float32 and float64 bins agree
            b64 = ahr.dir_bins64(c["targets"], c["anchors"], c["dir_offset"], NB)
            assert np.array_equal(b64, ahr.dir_bins32(c["targets"], c["anchors"], c["dir_offset"], NB))
            assert set(np.unique(b64[c["labels"] > 0])) == set(range(NB)) or A == 1
            v = c["targets"][..., 6].astype(np.float64) + c["anchors"][None, :, 6] - c["dir_offset"]
            assert A == 1 or (v.min() < 0 and v.max() > 2 * np.pi)
    assert seen_nc == {1, 3, 8} and seen_nb == {None, 2, 4, 8} and seen_b == {1, 3} and seen_beta == {1.0 / 9.0, 0.0}
    assert {1, 255, 256, 258, 1026, 1028} <= seen_a
    c = ahr.loss_case("a1028")
    lab = c["labels"]
    assert set(np.unique(lab[0])) == {-1, 0, 1, 2, 3} and (lab[1] == -1).all() and (lab[2] > 0).all()
    assert (ahr.loss_case("a258_bins8")["labels"][1] <= 0).all() and (ahr.loss_case("a258_bins8")["labels"][1] == 0).any()
    assert {0.0, 20.0, -20.0, 90.0, -90.0} <= set(c["cls"][0, :2].reshape(-1).tolist())
    d = (c["box"] - c["targets"])[..., :6][lab > 0]
    d = d[~np.isnan(d)]
    assert (d == 0).any() and ((np.abs(d) > 0) & (np.abs(d) < 1 / 9)).any() and (d > 1 / 9).any() and (d < -1 / 9).any()
    assert (c["box"][..., 6] == c["targets"][..., 6])[lab > 0].any()          # heading difference exactly 0
    assert np.isnan(c["targets"][..., 4][lab > 0]).any() and not np.isnan(c["targets"][..., 6]).any()
    for name in ("nan_heading", "nan_heading_l1"):
        c = ahr.loss_case(name)
        assert np.isnan(c["targets"][..., 6][c["labels"] > 0]).sum() >= 8


@pytest.mark.parametrize("name", ("boundary_2", "boundary_4", "boundary_8"))
def test_boundary_bins(name):
    """On a bin boundary the reference's float32 bin is the definition.  One rounding per float32 operation in torch's
    order reproduces it; the cases do cross boundaries (a float32 step changes the bin) and differ from float64."""
    c, rec = ahr.loss_case(name), ahr.golden()["loss_%s_bins32" % name].astype(np.int64)
    nb = c["num_dir_bins"]
    assert np.array_equal(ahr.dir_bins32(c["targets"], c["anchors"], c["dir_offset"], nb), rec)
    assert set(np.unique(rec)) == set(range(nb))
    below, on, above = rec[0, 1::3], rec[0, 0::3], rec[0, 2::3]
    assert (below != above).sum() >= nb
    assert ((on == below) | (on == above)).all()
    v = c["targets"][0, :, 6].astype(np.float64) + c["anchors"][:, 6] - c["dir_offset"]
    assert (np.abs(v) > 6 * np.pi).sum() >= 3 * nb             # periods in which floor(v / 2 pi) * 2 pi is inexact
    assert (ahr.dir_bins64(c["targets"], c["anchors"], c["dir_offset"], nb) != rec).any()


def test_head_get_loss_torch_float32_within_floor():
    """head.get_loss_torch() in float32 on the CPU against loss_ref on the same predictions, labels and targets, within
    the floor of point_loss_ref.measured_bound (1e-6 of each tensor's largest magnitude)."""
    g = ahr.modules()
    head = ahr.fixture_head()
    head({"spatial_features_2d": torch.from_numpy(g["head_feat"]), "gt_boxes": torch.from_numpy(g["head_gt"]),
          "batch_size": 2})
    fr = head.forward_ret_dict
    preds = [fr[k] for k in ("cls_preds", "box_preds", "dir_cls_preds")]
    for p in preds:
        p.retain_grad()
    loss, tb = head.get_loss_torch()
    loss.backward()
    cfg = head.model_cfg
    w = cfg.LOSS_CONFIG.LOSS_WEIGHTS
    view = lambda p, n: p.detach().numpy().reshape(2, -1, n)
    want = ahr.loss_ref(view(preds[0], 3), view(preds[1], 7), view(preds[2], 2), fr["box_cls_labels"].numpy(),
                        fr["box_reg_targets"].numpy(), head._flat_anchors().reshape(-1, 7).numpy(), cfg.DIR_OFFSET,
                        w["cls_weight"], w["loc_weight"], w["dir_weight"], head.reg_loss_func.beta,
                        head.cls_loss_func.alpha, cfg.NUM_DIR_BINS)
    got = [np.array([float(tb["rpn_loss_cls"]), float(tb["rpn_loss_loc"]), float(tb["rpn_loss_dir"])])]
    got += [view(p.grad, n).astype(np.float64) for p, n in zip(preds, (3, 7, 2))]
    for name, a, b in zip(("losses", "dcls", "dbox", "ddir"), got, want):
        err, floor = float(np.abs(a - b).max()), plr.measured_bound(0.0, b)
        print("%-7s e_float32 %.3e  floor %.3e" % (name, err, floor))
        assert err <= floor, (name, err, floor)


# ------------------------------------------------------------------------------------------- argument validation

INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -3


def _fake(n):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def _assign(lib, n_sets=3, a=2560, per_loc=2, b=2, m=8, n_classes=3, null=None, ws_bytes=None):
    anchors, gt, set_cls, mt, um, labels, targets, weights, ws = ptrs = _fake(9)
    if null is not None:
        ptrs[null] = None
        anchors, gt, set_cls, mt, um, labels, targets, weights, ws = ptrs
    if ws_bytes is None:
        ws_bytes = lib.spx_assign_targets_ws_bytes(b, n_sets, m)
    return lib.spx_assign_targets(anchors, n_sets, a, per_loc, gt, b, m, set_cls, n_classes, mt, um, labels, targets,
                                  weights, ws, ws_bytes, None)


def _loss(lib, b=2, a=7680, nc=3, nb=2, null=None, ws_bytes=None):
    ptrs = _fake(11)
    if null is not None:
        ptrs[null] = None
    cls, box, dirp, labels, targets, anchors, losses, dcls, dbox, ddir, ws = ptrs
    if ws_bytes is None:
        ws_bytes = lib.spx_anchor_loss_ws_bytes(b, a)
    return lib.spx_anchor_loss(cls, box, dirp, labels, targets, anchors, b, a, nc, nb, 0.78539, 1.0, 2.0, 0.2, 1.0 / 9.0,
                               0.25, losses, dcls, dbox, ddir, ws, ws_bytes, None)


def test_assign_targets_argument_validation():
    from spx import _lib
    lib = _lib.load()
    assert lib.spx_strerror(INVALID) and lib.spx_strerror(WORKSPACE) and lib.spx_strerror(UNSUPPORTED)
    for null in range(8):                                   # every input and output pointer
        assert _assign(lib, null=null) == INVALID, null
    assert _assign(lib, a=2561) == INVALID                  # anchors_per_set % per_location != 0
    assert _assign(lib, a=6, per_loc=4) == INVALID
    for kw in ({"n_sets": 0}, {"a": 0}, {"per_loc": 0}, {"b": 0}, {"m": 0}, {"n_classes": 0}, {"b": -1}):
        assert _assign(lib, **kw) == INVALID, kw
    assert _assign(lib, m=257) == UNSUPPORTED
    assert _assign(lib, m=1 << 20) == UNSUPPORTED
    assert _assign(lib, null=8) == WORKSPACE                # no workspace
    assert _assign(lib, ws_bytes=lib.spx_assign_targets_ws_bytes(2, 3, 8) - 1) == WORKSPACE
    assert _assign(lib, m=256, ws_bytes=lib.spx_assign_targets_ws_bytes(2, 3, 128)) == WORKSPACE
    assert lib.spx_assign_targets_ws_bytes(2, 3, 8) >= 2 * 3 * 8 * 4 + 2 * 4


def test_anchor_loss_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for null in (0, 1, 3, 4, 5, 6, 7, 8):                   # every pointer that is not optional
        assert _loss(lib, null=null) == INVALID, null
    assert _loss(lib, null=9) == INVALID                    # direction logits without a gradient buffer
    assert _loss(lib, nc=9) == INVALID and _loss(lib, nc=0) == INVALID
    assert _loss(lib, nb=9) == INVALID and _loss(lib, nb=0) == INVALID
    assert _loss(lib, b=0) == INVALID and _loss(lib, a=0) == INVALID
    assert _loss(lib, null=10) == WORKSPACE                 # no workspace
    assert _loss(lib, ws_bytes=lib.spx_anchor_loss_ws_bytes(2, 7680) - 1) == WORKSPACE
    assert _loss(lib, a=76800, ws_bytes=lib.spx_anchor_loss_ws_bytes(2, 7680)) == WORKSPACE
    assert lib.spx_anchor_loss_ws_bytes(2, 7680) >= 2 * 30 * 3 * 4 + 2 * 4


def test_ops_refuse_cpu_tensors():
    from spx import _lib, ops
    c = ahr.loss_case("one_anchor")
    t = torch.from_numpy
    with pytest.raises(_lib.SpxError):
        ops.anchor_loss(t(c["cls"]), t(c["box"]), t(c["dir"]), t(c["labels"]), t(c["targets"]), t(c["anchors"]),
                        c["dir_offset"], *c["weights"])
    case = ahr.synth_case("tie")
    with pytest.raises(_lib.SpxError):
        ops.assign_targets(t(case["anchor_sets"][0].reshape(1, -1, 7)), 1, t(case["gt"]),
                           torch.zeros(1, dtype=torch.int32), 3, torch.tensor([0.75]), torch.tensor([0.5]))
