"""The rotated-BEV pair test (csrc/box_iou.h) and every NMS built on it, on the GPU, against the float64 references of
tests/box_iou_ref.py: spx_boxes_iou_bev by value within the measured per-family tolerance (box_iou_ref.TOL) on
margin-stable pairs; spx_nms_bev, the host greedy over the device's own IoU matrix and spx_point_post_process against
each other exactly (one decision per pair, whoever asks) and against the float64 greedy at thresholds that sit in wide
gaps of the reference IoUs; structures with a known keep list across the 64-box chunk boundaries.
Run with -s to see the observed errors (profiles/box_iou_accuracy.log)."""
import numpy as np
import pytest
import torch

import box_iou_ref as R
from test_box_iou_ref import family, nms_case, NMS_LO, NMS_HI

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
STRUCT_SIZES = (1, 2, 63, 64, 65, 128, 129, 193)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _nms(boxes, thresh, axis_aligned=False):
    """Kept positions of ops.nms_bev over boxes in score order."""
    from spx import ops
    keep, cnt = ops.nms_bev(_dev(boxes), thresh, axis_aligned=axis_aligned)
    k = int(cnt.item())
    assert 0 <= k <= len(boxes)
    return keep[:k].cpu().numpy()


def _post(boxes, thresh, axis_aligned=False):
    """Kept positions (in score order) of class-agnostic ops.point_post_process: one frame, one score threshold below
    every score, pre_max = post_max = n.  The rows go in shuffled, so the op's own ordering is part of what is checked."""
    from spx import ops
    n = len(boxes)
    perm = np.random.default_rng(n).permutation(n)                  # row r holds the box of score rank perm[r]
    scores = np.linspace(0.95, 0.05, n).astype(np.float32)
    assert n < 2 or np.all(np.diff(scores) < 0)
    out = ops.point_post_process(_dev(scores[perm]), torch.ones(n, dtype=torch.int64, device=DEV), _dev(boxes[perm]), 1,
                                 [0.01], thresh, n, n, axis_aligned=axis_aligned, per_class=False)
    k = int(out["count"][0])
    sel = out["sel"][0].cpu().numpy()
    assert tuple(out["sel"].shape) == (1, n) and (sel[k:] == -1).all()
    return perm[sel[:k]]


def _host_greedy(matrix, thresh):
    """The greedy over a device fp32 matrix read as [earlier, later], with the kernels' comparison: fp32 v > fp32 thresh."""
    return R.greedy_ref(matrix, np.float32(thresh))


# ----------------------------------------------------------------------------------------- pair test against float64
@pytest.mark.parametrize("name", list(R.FAMILIES))
def test_pair_test_matches_float64_reference(name):
    from spx import ops
    a, b, iou, overlap, clear = family(name)
    ok = R.stable(clear)
    key = R.family_key(name)
    got_iou = ops.boxes_iou_bev(_dev(a), _dev(b)).cpu().numpy().astype(np.float64)
    got_ov = ops.boxes_iou_bev(_dev(a), _dev(b), overlap_only=True).cpu().numpy().astype(np.float64)
    assert got_iou.shape == got_ov.shape == iou.shape
    e_iou, e_ov = np.abs(got_iou - iou)[ok].max(), np.abs(got_ov - overlap)[ok].max()
    print("device vs float64 reference, %-22s max err iou %.3e (TOL %.1e)  overlap %.3e (TOL %.1e)  unstable pairs %d"
          % (name, e_iou, R.TOL[key]["iou"], e_ov, R.TOL[key]["overlap"], int((~ok).sum())))
    # every pair, stable or not: finite, an IoU in [0, 1], an area that is not negative
    assert np.isfinite(got_iou).all() and got_iou.min() >= 0 and got_iou.max() <= 1
    assert np.isfinite(got_ov).all() and got_ov.min() >= 0
    assert e_iou <= R.TOL[key]["iou"]
    assert e_ov <= R.TOL[key]["overlap"]
    cf = R.closed_form(name)
    if cf is not None:
        known, area = cf
        input_err = R.CLOSED_FORM_INPUT_ERR[key]
        sa, sb = (a[:, 3].astype(np.float64) * a[:, 4])[:, None], (b[:, 3].astype(np.float64) * b[:, 4])[None]
        c_iou = np.abs(got_iou - area / (sa + sb - area))[known].max()
        print("device vs closed form,       %-22s max err iou %.3e (TOL + input error %.1e)"
              % (name, c_iou, R.TOL[key]["iou"] + input_err))
        assert c_iou <= R.TOL[key]["iou"] + input_err
        if input_err <= 1e-12:                 # the fp32 boxes are the ideal ones: the area has its closed form too
            assert np.abs(got_ov - area)[known].max() <= R.TOL[key]["overlap"] + input_err


def test_empty_operands_give_empty_matrices():
    from spx import ops
    a, b = (_dev(x) for x in R.grid_axis())
    none = torch.zeros((0, 7), device=DEV)
    for overlap_only in (False, True):
        left = ops.boxes_iou_bev(none, b, overlap_only=overlap_only)
        right = ops.boxes_iou_bev(a, none, overlap_only=overlap_only)
        both = ops.boxes_iou_bev(none, none, overlap_only=overlap_only)
        assert tuple(left.shape) == (0, b.shape[0]) and tuple(right.shape) == (a.shape[0], 0) and tuple(both.shape) == (0, 0)
        assert left.dtype == right.dtype == torch.float32


@pytest.mark.parametrize("name", ["clustered", "grid_axis"])
def test_iou3d_matches_float64_reference(name):
    """boxes_iou3d_gpu = BEV overlap x height overlap / union volume.  With O the 3-D overlap and U the union,
    d IoU / d O = (Va + Vb) / U^2 <= 2 / U, d O = h d(overlap) and U >= max(Va, Vb) >= h max(area): an error of
    TOL["overlap"] in the BEV overlap moves the IoU by at most 2 TOL / (smallest BEV area); the tensor expression's own
    fp32 roundings (five operations on values up to 1) add under 1e-6."""
    from pcdet_amd.ops.iou3d_nms import iou3d_nms_utils
    a, b = (x.copy() for x in R.FAMILIES[name]())
    rng = np.random.default_rng(7)
    for x in (a, b):                      # z and dz on multiples of 1/8: touching in height is exact
        x[:, 2] = rng.integers(-8, 9, len(x)) / 8.0
        x[:, 5] = rng.integers(1, 13, len(x)) / 8.0
    want, clear = R.iou3d_ref(a, b)
    ok = R.stable(clear)
    bev = R.overlap_ref(a, b)[0] > 0
    top = np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None])
    bot = np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None])
    assert (bev & (top == bot)).sum() > 10 and (bev & (top < bot)).sum() > 10 and (bev & (top > bot)).sum() > 100
    got = iou3d_nms_utils.boxes_iou3d_gpu(_dev(a), _dev(b)).cpu().numpy().astype(np.float64)
    tol = 2 * R.TOL[name]["overlap"] / float(min((a[:, 3] * a[:, 4]).min(), (b[:, 3] * b[:, 4]).min())) + 1e-6
    err = np.abs(got - want)[ok].max()
    print("3-D IoU, device vs float64 reference, %-12s max err %.3e (bound %.1e)" % (name, err, tol))
    assert err <= tol
    assert (got[bev & (top <= bot)] == 0).all()                    # disjoint or touching in height: exactly 0
    assert np.isfinite(got).all() and got.min() >= 0


# --------------------------------------------------------------------------------------- one decision per pair (exact)
@pytest.mark.parametrize("n", R.NMS_SIZES)
def test_rotated_nms_paths_take_the_same_decisions_and_match_float64(n):
    """ops.nms_bev, the host greedy over the device matrix ops.boxes_iou_bev(x, x) read as [earlier, later], and
    class-agnostic ops.point_post_process: three callers of box_iou.h, one keep list.  At the gap threshold (no reference
    IoU within 10 TOL of it: tests/test_box_iou_ref.py) the list is also the float64 greedy's; at thresholds that ARE
    entries of the device matrix the three must still agree, which they do only if the pair test gives every caller the
    same bits (v > thresh is false for the pair the threshold was taken from, true one ulp above)."""
    from spx import ops
    x, iou, _, thresh, half = nms_case(n)
    matrix = ops.boxes_iou_bev(_dev(x), _dev(x)).cpu().numpy()
    want = R.greedy_ref(iou, thresh)
    for got in (_nms(x, thresh), _host_greedy(matrix, thresh), _post(x, thresh)):
        assert np.array_equal(got, want)
    upper = matrix[np.triu_indices(n, 1)]
    live = np.sort(upper[(upper > NMS_LO) & (upper < NMS_HI)])
    assert len(live) >= 8
    for q in ((0.1, 0.35, 0.6, 0.85) if n < 1000 else (0.3, 0.7)):
        on_entry = float(live[int(q * (len(live) - 1))])
        host = _host_greedy(matrix, on_entry)
        assert len(host) < n
        assert np.array_equal(_nms(x, on_entry), host), on_entry
        assert np.array_equal(_post(x, on_entry), host), on_entry


@pytest.mark.parametrize("n", R.NMS_SIZES)
def test_axis_aligned_nms_paths_take_the_same_decisions_and_match_float64(n):
    """Exact-grid boxes (centres and sizes on multiples of 1/64): the axis-aligned IoU is exact up to its division, the
    threshold sits in a gap of at least 1e-4 (tests/test_box_iou_ref.py), so the float64 greedy is the answer."""
    g = R.nms_boxes(n, grid=True)
    ion = R.iou_normal_ref(g, g)
    thresh, half = R.gap_threshold(ion, NMS_LO, NMS_HI)
    assert half >= 1e-4
    want = R.greedy_ref(ion, thresh)
    assert np.array_equal(_nms(g, thresh, axis_aligned=True), want)
    assert np.array_equal(_post(g, thresh, axis_aligned=True), want)


# ------------------------------------------------------------------------------------------ known-answer structures
def _both_paths(boxes, thresh, axis_aligned):
    got = _nms(boxes, thresh, axis_aligned)
    assert np.array_equal(_post(boxes, thresh, axis_aligned), got)
    return got.tolist()


@pytest.mark.parametrize("axis_aligned", [False, True])
@pytest.mark.parametrize("n", STRUCT_SIZES)
def test_known_answer_structures(n, axis_aligned):
    """Exact-grid boxes at heading 0 (exact in both modes); thresholds far from every IoU of the structure."""
    # chain: neighbours 1/3, second neighbours touch -> a suppressed box suppresses nothing, across 63|64 and 127|128
    assert _both_paths(R.chain(n), 0.2, axis_aligned) == list(range(0, n, 2))
    # star: box 0 covers the others with IoU 1 / area(0); above that IoU nothing goes
    star = R.star(n)
    low = 1.0 / float(star[0, 3] * star[0, 4])
    assert _both_paths(star, low / 2, axis_aligned) == [0]
    assert _both_paths(star, min(2 * low, 0.9), axis_aligned) == list(range(n))
    assert _both_paths(R.all_identical(n), 0.9, axis_aligned) == [0]
    assert _both_paths(R.all_disjoint(n), 0.0, axis_aligned) == list(range(n))
    if n > 1:       # only the last box of the last chunk overlaps box 0
        assert _both_paths(R.late_hit(n), 0.2, axis_aligned) == list(range(n - 1))


def test_strictly_above_the_threshold_suppresses():
    """A 1 x 1 box flush inside a 2 x 1 box: axis-aligned IoU exactly 0.5 in fp32."""
    flush = R.nested_flush()
    assert _both_paths(flush, 0.5, True) == [0, 1]
    assert _both_paths(flush, float(np.nextafter(np.float32(0.5), np.float32(0))), True) == [0]


def test_no_boxes_no_keeps():
    from pcdet_amd.ops.iou3d_nms import iou3d_nms_utils
    from spx import ops
    none = torch.zeros((0, 7), device=DEV)
    for axis_aligned in (False, True):
        keep, cnt = ops.nms_bev(none, 0.1, axis_aligned=axis_aligned)
        assert int(cnt.item()) == 0 and keep[:0].numel() == 0 and cnt.dtype == torch.int64
    sel, _ = iou3d_nms_utils.nms_gpu(none, torch.zeros(0, device=DEV), 0.1)
    assert sel.numel() == 0 and sel.dtype == torch.int64


@pytest.mark.parametrize("n", [65, 129])
def test_decisions_survive_a_rigid_motion(n):
    """Chain and star turned together by pi / 4 and moved to (75, -75), rotated mode: IoUs stay 1/3, ~0 and 1 / area(0)
    up to fp32 rounding at Waymo range, far from the thresholds."""
    moved = lambda boxes: R._f32(R.rotate_about_origin(boxes.astype(np.float64), np.pi / 4, (75.0, -75.0)))   # noqa: E731
    assert _both_paths(moved(R.chain(n)), 0.2, False) == list(range(0, n, 2))
    star = R.star(n)
    low = 1.0 / float(star[0, 3] * star[0, 4])
    assert _both_paths(moved(star), low / 2, False) == [0]
    assert _both_paths(moved(star), min(2 * low, 0.9), False) == list(range(n))
    assert _both_paths(moved(R.late_hit(n)), 0.2, False) == list(range(n - 1))
