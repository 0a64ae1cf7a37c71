"""Point-head target assignment on the GPU (csrc/point_targets.hip, include/spx.h §16) against the float32 numpy
restatement (tests/point_targets_ref.py): labels, box indices, box / centre rows, code offsets, bin one-hot and bin
residual equal, the log columns within 4 ulp, centerness within rtol 5e-5 of a float64 evaluation on rows that are
>= 0.05 m from every face; null outputs and canaries; the functional wrappers, the head's methods and
PointSASALoss.forward; graph capture (which fails on any host read)."""
import functools

import numpy as np
import pytest
import torch

import point_head_configs as phc
import point_targets_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = np.float32
LOG_ULP = 4          # OpenCL's bound for log is 3 ulp, plus 1 for rounding the value it is compared with
CANARY = 12345.5
FLOATS = ("box_labels", "center_labels", "reg_labels", "centerness")


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(m, ld):
    return ref.make_case(m, ld)


@functools.lru_cache(maxsize=None)
def _want(m, ld, mode, num_class, bins):
    pts, gt, _ = _case(m, ld)
    return ref.assign(pts, gt, mode, ref.EXTRA_WIDTH, ref.RADIUS, num_class, bins)


def _stacked(pts):
    """(B, N, 3) -> (B * N, 4) [bs_idx, x, y, z], the layout the heads pass around."""
    b, n = pts.shape[:2]
    bs = np.repeat(np.arange(b, dtype=F32), n)[:, None]
    return _g(np.concatenate([bs, pts.reshape(-1, 3)], axis=1))


def _check(got, want, bins, pts=None, loc=None, need_rows=0):
    """got: dict of tensors (the op's keys), want: the restatement's dict."""
    assert got["cls_labels"].dtype == torch.int64
    np.testing.assert_array_equal(got["cls_labels"].cpu().numpy(), want["cls_labels"])
    if "box_idx" in got:
        assert got["box_idx"].dtype == torch.int32
        np.testing.assert_array_equal(got["box_idx"].cpu().numpy(), want["box_idx"])
    if "box_labels" in got:
        np.testing.assert_array_equal(got["box_labels"].cpu().numpy(), want["box_labels"])
    if "center_labels" in got:
        np.testing.assert_array_equal(got["center_labels"].cpu().numpy(), want["center_labels"])
    if "reg_labels" in got:
        reg = got["reg_labels"].cpu().numpy()
        assert reg.shape == (want["cls_labels"].shape[0], 6 + 2 * bins)
        np.testing.assert_array_equal(reg[:, 0:3], want["reg_labels"][:, 0:3])
        np.testing.assert_array_equal(reg[:, 6:6 + bins], want["reg_labels"][:, 6:6 + bins])
        np.testing.assert_array_equal(reg[:, 6 + bins:], want["reg_labels"][:, 6 + bins:])
        d = ref.ulp_distance(reg[:, 3:6], want["reg_labels"][:, 3:6])
        print("log columns: max ulp distance %d" % d.max())
        assert d.max() <= LOG_ULP
    if "centerness" in got:
        cen = got["centerness"].cpu().numpy()
        assert not cen[~want["fg"]].any()
        if pts is not None:
            rows, nearest = ref.centerness_rows(pts, loc, want)
            print("centerness rows %d, nearest face %.4f m" % (rows.size, nearest))
            assert rows.size >= need_rows and nearest >= 0.05
            exact = ref.centerness(want["box_labels"][rows], pts.reshape(-1, 3)[rows], np.float64)
            if rows.size:
                print("centerness: max relative error %.3g" % np.abs(cen[rows] / exact - 1).max())
            np.testing.assert_allclose(cen[rows], exact, rtol=5e-5)


@pytest.mark.parametrize("mode", [ref.PLAIN, ref.IGNORE_RING, ref.BALL])
@pytest.mark.parametrize("m,ld", ref.CASES)
@pytest.mark.parametrize("num_class,bins", [(1, 12), (3, 12), (3, 0)])
def test_op_matches_restatement(m, ld, mode, num_class, bins):
    from spx import ops
    pts, gt, loc = _case(m, ld)
    want_keys = tuple(k for k in FLOATS if bins > 0 or k != "reg_labels")
    got = ops.point_assign_targets(_g(pts), _g(gt), mode, extra_width=ref.EXTRA_WIDTH, central_radius=ref.RADIUS,
                                   num_class=num_class, angle_bin_num=bins, want=want_keys)
    assert sorted(got) == sorted(("cls_labels", "box_idx") + want_keys)
    _check(got, _want(m, ld, mode, num_class, bins), bins, pts, loc, need_rows=50 if m >= 1 else 0)


def test_null_outputs_and_canaries():
    """The float outputs are optional; what is written stays inside its buffer."""
    from spx import _lib, ops
    lib = _lib.load()
    pts, gt, _ = _case(5, 10)
    b, n = pts.shape[:2]
    rows, bins, pad = b * n, 12, 64
    want = _want(5, 10, ref.BALL, 3, bins)
    d_pts, d_gt = _g(pts), _g(gt)
    widths = {"box_labels": 7, "center_labels": 3, "reg_labels": 6 + 2 * bins, "centerness": 1}
    ew = _lib.f_arr(ref.EXTRA_WIDTH)

    def run(keys):
        cls = torch.full((rows + 2 * pad,), -77, dtype=torch.int64, device=DEV)
        idx = torch.full((rows + 2 * pad,), -77, dtype=torch.int32, device=DEV)
        bufs = {k: torch.full((rows * widths[k] + 2 * pad,), CANARY, dtype=torch.float32, device=DEV) for k in keys}

        def p(k):
            return ops._ptr(bufs[k][pad:]) if k in bufs else None

        rc = lib.spx_point_assign_targets(ops._ptr(d_pts), ops._ptr(d_gt), b, n, gt.shape[1], gt.shape[2], ew, ref.BALL,
                                          ref.RADIUS, 3, bins, ops._ptr(cls[pad:]), ops._ptr(idx[pad:]), p("box_labels"),
                                          p("center_labels"), p("reg_labels"), p("centerness"), ops._stream(d_pts))
        assert rc == 0
        torch.cuda.synchronize()
        for t, guard in [(cls, -77), (idx, -77)] + [(bufs[k], CANARY) for k in keys]:
            assert (t[:pad] == guard).all() and (t[-pad:] == guard).all()
        got = {"cls_labels": cls[pad:-pad], "box_idx": idx[pad:-pad]}
        for k in keys:
            body = bufs[k][pad:-pad]
            got[k] = body if widths[k] == 1 else body.view(rows, widths[k])
        return got

    _check(run(()), want, bins)
    _check(run(("centerness",)), want, bins)
    _check(run(("reg_labels", "box_labels")), want, bins)
    _check(run(FLOATS), want, bins)
    with pytest.raises(_lib.SpxError):                                    # reg_labels without bins
        ops.point_assign_targets(d_pts, d_gt, ref.BALL, want=("reg_labels",))
    with pytest.raises(_lib.SpxError):
        ops.point_assign_targets(d_pts, d_gt[:, :, :7], ref.BALL, want=())


@pytest.mark.parametrize("m,ld", [(0, 8), (5, 10)])
def test_functional_wrappers_and_sasa_loss(m, ld):
    from pcdet_amd.models.dense_heads import point_targets
    from pcdet_amd.utils import loss_utils
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    pts, gt, loc = _case(m, ld)
    rows = pts.shape[0] * pts.shape[1]
    points, d_gt = _stacked(pts), _g(gt)
    coder = PointBinResidualCoder(use_mean_size=False, angle_bin_num=12)

    t = point_targets.assign_stack_targets_mask(points, d_gt, coder, 3, ref.RADIUS, with_centerness=True)
    assert sorted(t) == ["point_box_labels", "point_centerness_labels", "point_cls_labels", "point_reg_labels"]
    assert t["point_cls_labels"].dtype == torch.int64 and tuple(t["point_cls_labels"].shape) == (rows,)
    assert tuple(t["point_reg_labels"].shape) == (rows, coder.code_size) and tuple(t["point_box_labels"].shape) == (rows, 7)
    want = _want(m, ld, ref.BALL, 3, 12)
    got = {"cls_labels": t["point_cls_labels"], "box_labels": t["point_box_labels"],
           "reg_labels": t["point_reg_labels"], "centerness": t["point_centerness_labels"]}
    _check(got, want, 12, pts, loc)
    assert sorted(point_targets.assign_stack_targets_mask(points, d_gt, coder, 3, ref.RADIUS)) == \
        ["point_box_labels", "point_cls_labels", "point_reg_labels"]
    cen = point_targets.centerness_label(points, d_gt, 3, ref.RADIUS)
    assert torch.equal(torch.nan_to_num(cen, nan=-1.0), torch.nan_to_num(t["point_centerness_labels"], nan=-1.0))

    for ignore, mode in ((False, ref.PLAIN), (True, ref.IGNORE_RING)):
        t = point_targets.assign_targets_simple(points, d_gt, ref.EXTRA_WIDTH, set_ignore_flag=ignore)
        assert sorted(t) == ["point_cls_labels", "point_reg_labels"]
        assert t["point_cls_labels"].dtype == torch.int64 and tuple(t["point_reg_labels"].shape) == (rows, 3)
        want = _want(m, ld, mode, 1, 12)
        _check({"cls_labels": t["point_cls_labels"], "center_labels": t["point_reg_labels"]}, want, 12)

        sasa = loss_utils.PointSASALoss(func="Focal", layer_weights=[0.1, 0, 0.1, 0.1], extra_width=ref.EXTRA_WIDTH,
                                        set_ignore_flag=ignore, num_class=3)
        scores = torch.zeros(rows, 1, device=DEV)
        l_labels, l_boxes, l_parts = sasa([points] * 4, [scores, scores, None, scores], d_gt)
        assert [x is None for x in l_labels] == [False, True, True, False]     # None goes to l_labels only
        assert len(l_boxes) == 2 and len(l_parts) == 2
        want = _want(m, ld, mode, 3, 12)
        for lab, box, part in zip([l_labels[0], l_labels[3]], l_boxes, l_parts):
            assert lab.dtype == torch.int64 and tuple(lab.shape) == (rows,)
            assert tuple(box.shape) == (rows, 7) and tuple(part.shape) == (rows, 3)
            _check({"cls_labels": lab, "box_labels": box, "center_labels": part}, want, 12)
        lab, box, part = point_targets.sasa_assign_target(points, d_gt, ref.EXTRA_WIDTH, ignore)    # num_class None
        _check({"cls_labels": lab, "box_labels": box, "center_labels": part}, want, 12)


def test_head_methods():
    from pcdet_amd.models import dense_heads
    torch.manual_seed(0)
    cfg = phc.head_cfg()
    cfg.TARGET_CONFIG["GT_CENTRAL_RADIUS"] = ref.RADIUS
    head = dense_heads.__all__["PointHeadVoteSASAStatisticDistillation"](model_cfg=cfg, **phc.head_kwargs())
    pts, gt, loc = _case(5, 10)
    points, d_gt = _stacked(pts), _g(gt)
    want = _want(5, 10, ref.BALL, 3, 12)
    for t in (head.assign_targets({"point_vote_coords": points, "gt_boxes": d_gt}),
              head.assign_stu_targets({"s_point_vote_coords": points, "gt_boxes": d_gt})):
        assert sorted(t) == ["point_box_labels", "point_cls_labels", "point_reg_labels"]
        _check({"cls_labels": t["point_cls_labels"], "box_labels": t["point_box_labels"],
                "reg_labels": t["point_reg_labels"]}, want, 12)
    t = head.assign_targets_simple(points, d_gt, extra_width=ref.EXTRA_WIDTH, set_ignore_flag=False)
    want = _want(5, 10, ref.PLAIN, 1, 12)
    _check({"cls_labels": t["point_cls_labels"], "center_labels": t["point_reg_labels"]},
           want, 12)
    sasa = head.loss_point_sasa                                           # the config's: ignore ring of 1 m, 3 classes
    lab, box, part = sasa.assign_target(points, d_gt)
    want = ref.assign(pts, gt, ref.IGNORE_RING, sasa.extra_width, 0.0, sasa.num_class, 12)
    _check({"cls_labels": lab, "box_labels": box, "center_labels": part}, want, 12)


def test_graph_capture_and_replay_on_new_inputs():
    """Capture fails on any host read, so this is the no-sync check; the replay runs on inputs copied into the captured
    tensors afterwards."""
    from pcdet_amd.models.dense_heads import point_targets
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    coder = PointBinResidualCoder(use_mean_size=False, angle_bin_num=12)
    pts, gt, _ = _case(5, 10)
    pts2, gt2, _ = ref.make_case(5, 10, seed=7)
    assert not np.array_equal(gt, gt2)
    points, d_gt = _stacked(pts), _g(gt)

    def step():
        return point_targets.assign_stack_targets_mask(points, d_gt, coder, 3, ref.RADIUS)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    points.copy_(_stacked(pts2))
    d_gt.copy_(_g(gt2))
    for t in outs.values():
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    want = ref.assign(pts2, gt2, ref.BALL, (0.0, 0.0, 0.0), ref.RADIUS, 3, 12)
    _check({"cls_labels": outs["point_cls_labels"], "box_labels": outs["point_box_labels"], "reg_labels": outs["point_reg_labels"]}, want, 12)
    assert (want["cls_labels"] > 0).sum() >= 50 and (want["cls_labels"] == -1).sum() >= 20
