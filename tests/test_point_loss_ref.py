"""The point-head losses without a GPU: the torch compositions (point_losses.head_loss_torch,
PointSASALoss.loss_forward(fused=False), WeightedBinaryCrossEntropyLoss.forward) in float64 against what the reference
computes (tests/golden/point_head_losses.npz), the host-side argument checks of the new libspx entry points
(include/spx.h §17), and what must raise."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_loss_ref as plr

TOL = dict(rtol=1e-10, atol=1e-10)      # the bound tests/test_point_head_cpu.py uses for float64 restatements


@pytest.mark.parametrize("case", plr.CASES)
def test_head_loss_torch_matches_reference(case):
    from pcdet_amd.models.dense_heads import point_losses
    h = plr.head()
    rd = plr.ret_dict(case, torch.float64)
    total, parts = point_losses.head_loss_torch(rd, *plr.head_loss_args(h))
    want = plr.load(case)["losses"]
    assert parts.dtype == torch.float64 and not parts.requires_grad
    np.testing.assert_allclose(parts.numpy(), want, **TOL)
    np.testing.assert_allclose(float(total.detach()), want.sum(), **TOL)
    leaves = [rd[plr.LEAF_KEYS[k]] for k in plr.LEAVES]
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    for name, leaf, g in zip(plr.LEAVES, leaves, grads):
        g = np.zeros(leaf.shape) if g is None else g.numpy()
        np.testing.assert_allclose(g, plr.grad(case, "sum", name), err_msg=name, **TOL)
    if case == "c":
        assert want[0] == 0 and want[2] == 0 and want[1] > 0


@pytest.mark.parametrize("case", plr.CASES)
def test_head_loss_torch_components_match_reference(case):
    """Per component, so that the path from the cls loss into box_preds (through the soft target) is checked on its
    own: the torch composition is split by switching loss weights off."""
    from pcdet_amd.models.dense_heads import point_losses
    h = plr.head()
    members = {0: ("vote_reg_weight",), 1: ("point_cls_weight",),
               2: ("point_offset_reg_weight", "point_angle_cls_weight", "point_angle_reg_weight", "point_iou_weight",
                   "point_corner_weight")}
    for comp, keep in members.items():
        cfg = copy.deepcopy(h.model_cfg)
        for k in cfg.LOSS_CONFIG.LOSS_WEIGHTS:
            if k not in keep:
                cfg.LOSS_CONFIG.LOSS_WEIGHTS[k] = 0.0
        rd = plr.ret_dict(case, torch.float64)
        total, parts = point_losses.head_loss_torch(rd, cfg, h.box_coder, h.reg_loss_func, h.cls_loss_func)
        np.testing.assert_allclose(parts.numpy()[comp], plr.load(case)["losses"][comp], **TOL)
        leaves = [rd[plr.LEAF_KEYS[k]] for k in plr.LEAVES]
        grads = torch.autograd.grad(total, leaves, allow_unused=True)
        for name, leaf, g in zip(plr.LEAVES, leaves, grads):
            g = np.zeros(leaf.shape) if g is None else g.numpy()
            np.testing.assert_allclose(g, plr.grad(case, comp, name), err_msg="%d %s" % (comp, name), **TOL)
    if case != "c":
        assert np.abs(plr.grad(case, 1, "box")).max() > 0          # the cls loss does reach box_preds


@pytest.mark.parametrize("case", plr.CASES)
@pytest.mark.parametrize("func,s", plr.SEG_COMBOS)
def test_sasa_loss_forward_torch_matches_reference(case, func, s):
    from pcdet_amd.utils import loss_utils
    g = plr.load(case)
    sasa = loss_utils.PointSASALoss(func=func, layer_weights=[plr.SEG_LAYER_WEIGHT, 0.3, 0.2], extra_width=[1.0, 1.0, 1.0],
                                    set_ignore_flag=True, num_class=plr.NUM_CLASS)
    scores = torch.from_numpy(g["seg_scores%d" % s]).double().requires_grad_(True)
    labels = torch.from_numpy(g["seg_labels"])
    out = sasa.loss_forward([scores, None, scores], [labels, labels, None], [None] * 3, [None] * 3, [None] * 3, fused=False)
    assert out[1] is None and out[2] is None and out[0].dim() == 0
    np.testing.assert_allclose(float(out[0].detach()), g["seg_%s_s%d" % (func, s)], **TOL)
    grad, = torch.autograd.grad(out[0].sum(), scores)
    np.testing.assert_allclose(grad.numpy(), g["seg_%s_s%d_grad" % (func, s)], **TOL)


def test_sasa_bce_broadcasts_one_column_over_the_classes():
    """The combination the reference's BCE cannot evaluate with today's torch (it refuses a (N, 1) input against a
    (N, 3) target): a one-column score meets each of the num_class target columns, mean over them."""
    from pcdet_amd.utils import loss_utils
    g = plr.load("a")
    sasa = loss_utils.PointSASALoss(func="BCE", layer_weights=[0.1], num_class=3)
    x, labels = torch.from_numpy(g["seg_scores1"]).double(), torch.from_numpy(g["seg_labels"])
    out, = sasa.loss_forward([x], [labels], [None], [None], [None], fused=False)
    keep = labels >= 0
    tgt = torch.stack([(labels == c + 1).double() for c in range(3)], dim=1)
    want = F.binary_cross_entropy_with_logits(x.expand(-1, 3), tgt, reduction="none").mean(dim=1)[keep].sum() \
        * 0.1 / max(int(keep.sum()), 1)
    np.testing.assert_allclose(float(out), float(want), **TOL)


def test_weighted_bce_forward():
    from pcdet_amd.utils import loss_utils
    gen = torch.Generator().manual_seed(3)
    x, t = torch.randn(2, 9, 3, generator=gen, dtype=torch.float64), torch.rand(2, 9, 3, generator=gen, dtype=torch.float64)
    w = torch.rand(2, 9, generator=gen, dtype=torch.float64)
    got = loss_utils.WeightedBinaryCrossEntropyLoss()(x, t, w)
    want = F.binary_cross_entropy_with_logits(x, t, reduction="none").mean(dim=-1) * w
    assert got.shape == (2, 9) and torch.equal(got, want)


# ------------------------------------------------------------------------------------- host-side argument checks (§17)

def _fake(n):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def _head(lib, _lib, n=74, c=3, k=12, null=None, params=True, ws=True, ws_bytes=None):
    ptrs = _fake(18)
    if null is not None:
        ptrs[null] = None
    par = _lib.f_arr([1.0] * 11) if params else None
    wsb = lib.spx_point_head_loss_ws_bytes(n) if ws_bytes is None else ws_bytes
    return lib.spx_point_head_loss(*ptrs[:12], n, c, k, par, 1, 1, 1, *ptrs[12:17], ptrs[17] if ws else None, wsb, None)


def _seg(lib, n=74, s=1, num_class=3, func=1, null=None, ws=True, ws_bytes=None):
    ptrs = _fake(5)
    if null is not None:
        ptrs[null] = None
    scores, labels, loss, d_scores, wsp = ptrs
    wsb = lib.spx_point_seg_loss_ws_bytes(n) if ws_bytes is None else ws_bytes
    return lib.spx_point_seg_loss(scores, labels, n, s, num_class, func, 0.1, loss, d_scores, wsp if ws else None, wsb, None)


def test_point_head_loss_argument_validation():
    from spx import _lib
    lib = _lib.load()
    assert lib.spx_abi_version() == 3
    for null in range(17):                      # every input and output pointer
        assert _head(lib, _lib, null=null) == -1, null
    assert _head(lib, _lib, params=False) == -1
    assert _head(lib, _lib, n=-1) == -1 and _head(lib, _lib, c=0) == -1 and _head(lib, _lib, k=0) == -1
    assert _head(lib, _lib, c=9) == -3
    assert _head(lib, _lib, k=33) == -3
    assert _head(lib, _lib, c=8, k=32, ws=False) == -2          # the limits themselves pass the checks
    assert _head(lib, _lib, n=0) == 0                           # nothing to do, nothing launched
    assert _head(lib, _lib, ws=False) == -2
    assert _head(lib, _lib, ws_bytes=lib.spx_point_head_loss_ws_bytes(74) - 1) == -2
    sizes = [lib.spx_point_head_loss_ws_bytes(n) for n in (1, 74, 513, 2048, 12288)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]


def test_point_seg_loss_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for null in range(4):
        assert _seg(lib, null=null) == -1, null
    assert _seg(lib, n=-1) == -1 and _seg(lib, num_class=0) == -1 and _seg(lib, func=2) == -1
    assert _seg(lib, s=2) == -1                                 # scores are one column or num_class columns
    assert _seg(lib, num_class=9, s=9) == -3
    assert _seg(lib, n=0) == 0
    assert _seg(lib, ws=False) == -2
    assert _seg(lib, ws_bytes=lib.spx_point_seg_loss_ws_bytes(74) - 1) == -2
    sizes = [lib.spx_point_seg_loss_ws_bytes(n) for n in (1, 74, 513, 12288, 1 << 20)]      # 4 bytes per 256 rows
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]


# ---------------------------------------------------------------------------------------------------- what must raise

def test_ops_and_fused_loss_refuse_cpu_tensors():
    from spx import _lib, ops
    h = plr.head()
    rd = plr.ret_dict("a", torch.float32)
    with pytest.raises(_lib.SpxError):
        ops.point_head_loss(rd["s_point_vote_coords"], rd["s_point_cls_preds"], rd["s_point_reg_preds"],
                            rd["s_point_box_preds"], rd["point_cls_preds"], rd["point_reg_preds"], rd["point_box_preds"],
                            rd["vote_cls_labels"], rd["vote_reg_labels"], rd["s_point_cls_labels"],
                            rd["s_point_reg_labels"], rd["s_point_box_labels"], loss_weights=[1.0] * 8)
    with pytest.raises(_lib.SpxError):
        ops.point_seg_loss(torch.zeros(8, 1), torch.zeros(8, dtype=torch.int64), 3, 1, 0.1)
    with pytest.raises(_lib.SpxError):
        h.get_loss_fused(rd)
    sasa = h.loss_point_sasa
    with pytest.raises(_lib.SpxError):
        sasa.loss_forward([torch.zeros(8, 1)] * 3, [torch.zeros(8, dtype=torch.int64)] * 3, [None] * 3, [None] * 3,
                          [None] * 3)


def test_unsupported_settings_are_named():
    from pcdet_amd.models.dense_heads import point_losses
    from pcdet_amd.utils import box_coder_utils, loss_utils
    h = plr.head()
    rd = plr.ret_dict("a", torch.float32)
    args = dict(zip(("model_cfg", "box_coder", "reg_loss_func", "cls_loss_func"), plr.head_loss_args(h)))

    def raises(match, **change):
        with pytest.raises(NotImplementedError, match=match):
            point_losses.head_loss_fused(rd, **dict(args, **change))

    cfg = copy.deepcopy(h.model_cfg)
    cfg.LOSS_CONFIG["AXIS_ALIGNED_IOU_LOSS_REGULARIZATION"] = True
    raises("AXIS_ALIGNED_IOU_LOSS_REGULARIZATION", model_cfg=cfg)
    raises("pred_velo", box_coder=box_coder_utils.PointBinResidualCoder(use_mean_size=False, angle_bin_num=12,
                                                                        pred_velo=True))
    raises("use_mean_size", box_coder=box_coder_utils.PointBinResidualCoder(
        use_mean_size=True, angle_bin_num=12, mean_size=[[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]))
    raises("LOSS_CLS", cls_loss_func=loss_utils.SigmoidFocalClassificationLoss())
    raises("code_weights", reg_loss_func=loss_utils.WeightedSmoothL1Loss(code_weights=[1.0] * 30))


def test_get_loss_and_train_forward_still_raise():
    h = plr.head()
    with pytest.raises(NotImplementedError):
        h.get_loss()
    h.train()
    with pytest.raises(NotImplementedError, match="training"):
        h.forward({})
    with pytest.raises(ValueError):
        h.get_loss_torch()                       # no ret_dict and no forward yet


def test_get_loss_torch_on_the_cpu_has_the_reference_keys():
    h = plr.head()
    rd = plr.ret_dict("a", torch.float64)
    g = plr.load("a")
    scores, labels = torch.from_numpy(g["seg_scores1"]).double(), torch.from_numpy(g["seg_labels"])
    rd.update(point_sasa_preds=[scores, None, scores], point_sasa_labels=[labels, None, labels],
              point_sasa=[None] * 3, point_sasa_boxes=[None] * 3, point_sasa_parts=[None] * 3)
    loss, tb = h.get_loss_torch(rd)
    assert sorted(tb) == ["point_loss_box", "point_loss_cls", "point_loss_sasa", "point_loss_sasa_layer_0",
                          "point_loss_sasa_layer_2", "point_loss_vote", "point_pos_num", "vote_loss_reg"]
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and not v.requires_grad for v in tb.values())
    assert int(tb["point_pos_num"]) == int((g["cls_labels"] > 0).sum())
    want = g["losses"].sum() + 2 * float(g["seg_Focal_s1"])
    np.testing.assert_allclose(float(loss.detach()), want, **TOL)
