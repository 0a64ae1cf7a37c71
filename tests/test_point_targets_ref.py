"""Point-head target assignment without a GPU: the float32 restatement (tests/point_targets_ref.py) against the values
recorded from the reference coder and against an eager CPU composition of points-in-boxes, masks and
PointBinResidualCoder.encode_torch; the host-side argument checks of spx_point_assign_targets; and the refusal of CPU
tensors by every layer above it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import point_head_configs as phc
import point_targets_ref as ref
import roiaware_ref as rr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
LOG_ULP = 4     # OpenCL's bound for log is 3 ulp, plus 1 for rounding the value it is compared with


def test_restated_encode_matches_recorded_reference_values():
    z = np.load(os.path.join(GOLDEN, "point_bin_coder.npz"))
    want = z["encode_plain"]
    got = ref.encode(z["boxes"][:, :7], z["points"], 12)
    assert got.shape == want.shape[:1] + (30,)
    np.testing.assert_array_equal(got[:, 0:3], want[:, 0:3])
    np.testing.assert_array_equal(got[:, 6:30], want[:, 6:30])
    assert (want[:, 6:18].sum(axis=1) == 1).all()
    d = ref.ulp_distance(got[:, 3:6], want[:, 3:6])
    print("log columns: max ulp distance %d" % d.max())
    assert d.max() <= LOG_ULP


def _compose(points, gt_boxes, mode, extra_width, radius, num_class, bins):
    """The per-frame pattern the fused op replaces, on the CPU: points in boxes once or twice, boolean masks, the
    coder on the compacted rows, a scatter back.  Rows are filled where the label is > 0."""
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    coder = PointBinResidualCoder(use_mean_size=False, angle_bin_num=max(bins, 1))
    b, n = points.shape[:2]
    cls = torch.zeros(b * n, dtype=torch.int64)
    idx = torch.zeros(b * n, dtype=torch.int32)
    box, ctr, reg = torch.zeros(b * n, 7), torch.zeros(b * n, 3), torch.zeros(b * n, coder.code_size)
    for k in range(b):
        pts = torch.from_numpy(points[k])
        gt = torch.from_numpy(gt_boxes[k])
        ext = gt[:, :7].clone()
        ext[:, 3:6] += torch.tensor(extra_width, dtype=torch.float32)[None, :]
        in_gt = torch.from_numpy(rr.points_in_boxes(points[k:k + 1], gt[None, :, :7].numpy())[0]).long()
        in_ext = torch.from_numpy(rr.points_in_boxes(points[k:k + 1], ext[None].numpy())[0]).long()
        single = torch.zeros(n, dtype=torch.int64)
        hit = in_ext if mode == ref.PLAIN else in_gt
        flag = hit >= 0
        if mode == ref.IGNORE_RING:
            single[flag ^ (in_ext >= 0)] = -1
        elif mode == ref.BALL:
            centers = gt[hit.clamp(min=0)][:, 0:3] if gt.shape[0] else torch.zeros(n, 3)
            ball = (centers - pts).norm(dim=1) < radius
            single[flag & ~ball] = -1
            flag = flag & ball
        of_fg = gt[hit[flag]]
        single[flag] = 1 if num_class == 1 else of_fg[:, 7].long()
        fill = single > 0
        of_fg = gt[hit[fill]]
        sl = slice(k * n, (k + 1) * n)
        cls[sl], idx[sl] = single, hit.int()
        box[sl][fill] = of_fg[:, :7]
        ctr[sl][fill] = of_fg[:, 0:3]
        if bins > 0 and of_fg.shape[0] > 0:
            reg[sl][fill] = coder.encode_torch(of_fg[:, :7].clone(), pts[fill])
    return cls.numpy(), idx.numpy(), box.numpy(), ctr.numpy(), reg.numpy()


@pytest.mark.parametrize("mode", [ref.PLAIN, ref.IGNORE_RING, ref.BALL])
@pytest.mark.parametrize("m,ld", ref.CASES)
@pytest.mark.parametrize("num_class,bins", [(1, 12), (3, 12)])
def test_restatement_matches_eager_cpu_composition(m, ld, mode, num_class, bins):
    pts, gt, loc = ref.make_case(m, ld)
    got = ref.assign(pts, gt, mode, ref.EXTRA_WIDTH, ref.RADIUS, num_class, bins)
    cls, idx, box, ctr, reg = _compose(pts, gt, mode, ref.EXTRA_WIDTH, ref.RADIUS, num_class, bins)
    np.testing.assert_array_equal(got["cls_labels"], cls)
    np.testing.assert_array_equal(got["box_idx"], idx)
    np.testing.assert_array_equal(got["box_labels"], box)
    np.testing.assert_array_equal(got["center_labels"], ctr)
    np.testing.assert_array_equal(got["reg_labels"][:, 0:3], reg[:, 0:3])
    np.testing.assert_array_equal(got["reg_labels"][:, 6:], reg[:, 6:])
    assert ref.ulp_distance(got["reg_labels"][:, 3:6], reg[:, 3:6]).max() <= LOG_ULP
    if m >= 5:                                   # the inputs reach every label and the rows placed on purpose
        assert (cls == 0).any() and (cls > 0).sum() >= 50
        assert (cls == -1).sum() >= (0 if mode == ref.PLAIN else 20)     # the ring of mode 1, the corners of mode 2
    if m == 5:
        n = pts.shape[1]
        assert (got["box_idx"][loc["z_face"]::n] == 0).all()             # on the top face of box 0: inside
        if mode != ref.PLAIN:
            assert (got["box_idx"][loc["thin"]::n] == 2).all()           # the centre of the box with dx < 1e-5
            assert (got["box_idx"][loc["origin"]::n] == m - 1).all()     # the origin lies in the zero-padded row
        if num_class == 1 and mode != ref.PLAIN:
            assert (cls[loc["origin"]::n] == 1).all() and (got["reg_labels"][loc["origin"]::n, 3] < -11).all()
        if num_class == 3:
            assert (cls[loc["origin"]::n] == 0).all() and not got["reg_labels"][loc["origin"]::n].any()
            assert len(set(np.unique(cls)) & {1, 2, 3}) == 3
        both = rr.in_box(pts[0], gt[0, :2, :7])[0]
        assert (both[0] & both[1]).sum() >= 5                            # overlapping boxes: the first one wins
    rows, nearest = ref.centerness_rows(pts, loc, got)
    if m >= 1:
        assert rows.size >= 50 and nearest >= 0.05
        want = ref.centerness(got["box_labels"][rows], pts.reshape(-1, 3)[rows], np.float64)
        np.testing.assert_allclose(got["centerness"][rows], want, rtol=5e-5)
    assert not got["centerness"][~got["fg"]].any()


def test_inputs_reach_every_branch():
    """What the inputs shared with the GPU tests must contain, checked on the restatement's results."""
    pts, gt, loc = ref.make_case(5, 10)
    b, n = pts.shape[:2]
    assert n % 256 != 0 and n > 256                                       # a second, partly filled workgroup
    assert (np.abs(gt[:, :, 6]) > 2 * np.pi).any() and (gt[:, :, 6] < 0).any() and (gt[:, :, 6] > 0).any()
    assert ((gt[:, :, 3] < 1e-5) & (gt[:, :, 4] > 0)).any()               # a box with a size below 1e-5
    assert not gt[:, -1].any() and not pts[:, 0].any()                    # a zero-padded row, a point at the origin
    ring = ref.assign(pts, gt, ref.IGNORE_RING, ref.EXTRA_WIDTH, ref.RADIUS, 3, 12)
    ball = ref.assign(pts, gt, ref.BALL, ref.EXTRA_WIDTH, ref.RADIUS, 3, 12)
    assert (ring["cls_labels"] == -1).sum() >= 20                         # points in the grown-only ring
    assert (ball["cls_labels"] == -1).sum() >= 20                         # in a box, outside the ball
    half_diag = np.sqrt((gt[:, :4, 3:6].astype(np.float64) ** 2).sum(axis=2)) / 2
    assert (half_diag > ref.RADIUS).any()
    assert (ring["box_idx"][loc["z_face"]::n] == 0).all()                 # a point on a z face is inside
    assert (ring["box_idx"][loc["thin"]::n] == 2).all()
    assert (ring["box_idx"][loc["origin"]::n] == gt.shape[1] - 1).all()
    pts, gt, _ = ref.make_case(300, 8)
    assert (ref.assign(pts, gt, ref.BALL, ref.EXTRA_WIDTH, ref.RADIUS, 3, 12)["box_idx"] >= 256).any()   # second LDS chunk


def _fake(n):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def test_argument_validation_without_gpu():
    from spx import _lib
    lib = _lib.load()
    ew = _lib.f_arr([0.1, 0.1, 0.1])

    def call(null=None, b=2, n=64, m=4, ld=8, ew=ew, mode=0, num_class=3, bins=12):
        ptrs = _fake(8)
        if null is not None:
            ptrs[null] = None
        pts, gt, cls, idx, box, ctr, reg, cen = ptrs
        return lib.spx_point_assign_targets(pts, gt, b, n, m, ld, ew, mode, 2.0, num_class, bins, cls, idx, box, ctr, reg,
                                            cen, None)

    for null in range(4):                       # points, gt_boxes, cls_labels, box_idx
        assert call(null=null) == -1, null
    assert call(ew=None) == -1
    assert call(b=-1) == -1 and call(n=-1) == -1 and call(m=-1) == -1
    assert call(ld=7) == -1
    assert call(bins=33) == -3 and call(bins=-1) == -3
    assert call(mode=3) == -3 and call(mode=-1) == -3
    assert call(b=0) == 0 and call(n=0) == 0    # nothing to do, nothing launched
    assert call(b=70000) == -5


def _cpu_inputs():
    pts, gt, _ = ref.make_case(5, 8)
    b, n = pts.shape[:2]
    bs = np.repeat(np.arange(b, dtype=F32), n)[:, None]
    return torch.from_numpy(np.concatenate([bs, pts.reshape(-1, 3)], axis=1)), torch.from_numpy(gt)


def test_every_layer_refuses_cpu_tensors():
    """No CPU fallback: the op, the functional module, the head's methods and PointSASALoss.forward raise SpxError (not
    NotImplementedError: they are ported).  The head's forward in train mode still raises NotImplementedError."""
    from pcdet_amd.models import dense_heads
    from pcdet_amd.models.dense_heads import point_targets
    from pcdet_amd.utils import loss_utils
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    from spx import _lib, ops
    points, gt = _cpu_inputs()
    with pytest.raises(_lib.SpxError):
        ops.point_assign_targets(points[:, 1:4].reshape(3, -1, 3), gt, ops.TARGET_PLAIN)
    coder = PointBinResidualCoder(use_mean_size=False, angle_bin_num=12)
    with pytest.raises(_lib.SpxError):
        point_targets.assign_stack_targets_mask(points, gt, coder, 3, 10.0)
    with pytest.raises(_lib.SpxError):
        point_targets.assign_targets_simple(points, gt, [0.1, 0.1, 0.1], set_ignore_flag=False)
    with pytest.raises(_lib.SpxError):
        point_targets.centerness_label(points, gt, 3, 10.0)
    sasa = loss_utils.PointSASALoss(**phc.head_dict()["LOSS_CONFIG"]["LOSS_SASA_CONFIG"])
    with pytest.raises(_lib.SpxError):
        sasa([points, points, points], [None, torch.zeros(points.shape[0], 1), None], gt)
    torch.manual_seed(0)
    head = dense_heads.__all__["PointHeadVoteSASAStatisticDistillation"](model_cfg=phc.head_cfg(), **phc.head_kwargs())
    with pytest.raises(_lib.SpxError):
        head.assign_targets({"point_vote_coords": points, "gt_boxes": gt})
    with pytest.raises(_lib.SpxError):
        head.assign_stu_targets({"s_point_vote_coords": points, "gt_boxes": gt})
    with pytest.raises(_lib.SpxError):
        head.assign_targets_simple(points, gt, extra_width=[0.1, 0.1, 0.1], set_ignore_flag=False)
    head.train()
    with pytest.raises(NotImplementedError, match="training"):
        head({"batch_size": 1})
    with pytest.raises(NotImplementedError):
        head.get_loss()


def test_unsupported_settings_and_bad_shapes_raise():
    from pcdet_amd.models import dense_heads
    from pcdet_amd.models.dense_heads import point_targets
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    points, gt = _cpu_inputs()
    mean = PointBinResidualCoder(use_mean_size=True, angle_bin_num=12, mean_size=[[3.9, 1.6, 1.56]])
    with pytest.raises(NotImplementedError):
        point_targets.assign_stack_targets_mask(points, gt, mean, 3, 10.0)
    velo = PointBinResidualCoder(use_mean_size=False, angle_bin_num=12, pred_velo=True)
    with pytest.raises(NotImplementedError):
        point_targets.assign_stack_targets_mask(points, gt, velo, 3, 10.0)
    with pytest.raises(ValueError):                                 # 899 points do not make 3 equal frames
        point_targets.assign_targets_simple(points[:-1], gt, None, set_ignore_flag=False)
    cfg = phc.head_cfg()
    cfg.TARGET_CONFIG["ASSIGN_METHOD"] = "iou"
    torch.manual_seed(0)
    head = dense_heads.__all__["PointHeadVoteSASAStatisticDistillation"](model_cfg=cfg, **phc.head_kwargs())
    with pytest.raises(NotImplementedError, match="iou"):
        head.assign_targets({"point_vote_coords": points, "gt_boxes": gt})
