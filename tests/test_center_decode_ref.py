"""The centre-head decode without a GPU: the numpy restatement of spx_center_decode (tests/center_decode_ref.py) against
the reference's recorded decode_bbox_from_heatmap output (tests/golden/center_head.npz, b/*) with raw=0 and against this
tree's decode_bbox_from_heatmap on sigmoid / exp inputs with raw=1; the margins of the case table; the C ABI's symbols
and host-side argument checks; the operator layer's refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import center_decode_ref as cdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cdr.cases()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "center_head.npz")))


def golden_case(gold):
    """The recorded b/* inputs as a case of the restatement (raw=0: probabilities and sizes as given)."""
    g = lambda k: gold["b/in/" + k]                                              # noqa: E731
    return dict(hm=g("heatmap"), center=g("center"), center_z=g("center_z"), dim=g("dim"),
                rot=np.concatenate([g("rot_cos"), g("rot_sin")], axis=1), vel=None, k=int(gold["b/k"]),
                score_thresh=float(gold["b/score_thresh"]), limit=[float(v) for v in gold["b/limit"]], raw=False)


def test_restatement_equals_recorded_reference_output(gold):
    case = golden_case(gold)
    assert case["hm"].shape == (2, 3, 20, 24) and case["k"] == 16
    got = cdr.decode_case(case)
    kept = 0
    for f in range(2):
        want = {k: gold["b/out/f%d/%s" % (f, k)] for k in ("pred_boxes", "pred_scores", "pred_labels")}
        m = got["keep"][f].astype(bool)
        assert int(got["count"][f]) == m.sum() == len(want["pred_scores"])
        np.testing.assert_array_equal(got["labels"][f][m], want["pred_labels"])
        np.testing.assert_allclose(got["boxes"][f][m], want["pred_boxes"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["scores"][f][m], want["pred_scores"], rtol=0, atol=1e-6)
        kept += int(m.sum())
    assert 8 <= kept <= 24


def test_margins_hold_on_the_restatement_alone():
    worst_score, worst_xy = cdr.check_margins(CASES)
    print("smallest relative score margin %.3g, smallest x / y margin %.3g m" % (worst_score, worst_xy))
    assert worst_score >= cdr.SCORE_MARGIN and worst_xy >= cdr.XY_MARGIN


def test_distinct_flags_are_true_to_the_inputs():
    flags = {name: cdr.top_sigmoids_distinct(case) for name, case in CASES.items()}
    assert flags == {name: case["distinct"] for name, case in CASES.items()}
    assert sum(flags.values()) >= 5


def test_case_properties():
    """Each case does what it is there for, read off the restatement."""
    d = {name: cdr.decode_case(case) for name, case in CASES.items()}
    assert sorted(d["all_selected"]["cells"][0]) == list(range(16))
    assert list(d["constant"]["labels"][0]) == [0] * 100 and list(d["constant"]["cells"][0]) == list(range(100))
    t = d["tie_across_k"]
    assert list(t["cells"][0]) == [3, 4, 5, 6] + list(range(20, 38, 3)) and list(t["labels"][0]) == [0] * 10
    assert list(t["cells"][1]) == [3, 4, 5, 6] + [80 - 54 + i for i in range(6)] and list(t["labels"][1][4:]) == [1] * 6
    z = d["signed_zeros"]
    assert [int(c + 48 * lab) for c, lab in zip(z["cells"][0][:11], z["labels"][0][:11])] == list(range(5, 60, 5))
    assert (z["scores"][0][:11] == 0.5).all() and (z["scores"][0][11:] < 0.5).all()
    assert (CASES["all_negative"]["hm"] < 0).all() and 0 < d["all_negative"]["count"].min()
    s = d["saturated"]["scores"][0]
    assert (np.abs(CASES["saturated"]["hm"]) > 90).all() and (s[:24] == 1).all() and (s[24:] == 0).all()
    assert list(d["none_and_all"]["count"]) == [0, 20]
    assert list(d["z_on_limit"]["keep"][0][:4]) == [1, 0, 1, 0]
    k = d["kitti"]["count"]
    assert (k > 100).all() and (k < 450).all()
    assert {name for name, case in CASES.items() if case["vel"] is not None} >= {"odd_sizes", "kitti"}
    assert {name for name, case in CASES.items() if case["score_thresh"] is None} >= {"several_tiles", "z_on_limit"}


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["distinct"]))
def test_restatement_equals_eager_decode_on_distinct_cases(name):
    """raw=1 against decode_bbox_from_heatmap(hm.sigmoid(), dim.exp(), ...) on the CPU: with distinct sigmoids the
    two-stage topk has one answer.  Kept rows, their order and labels exact; x, y, z, vel exact; the float32
    transcendentals of torch within 1e-6 relative of the float64 ones."""
    from pcdet_amd.models.model_utils import centernet_utils
    case = CASES[name]
    got = cdr.decode_case(case)
    t = lambda a: None if a is None else torch.from_numpy(a)                     # noqa: E731
    out = centernet_utils.decode_bbox_from_heatmap(
        heatmap=t(case["hm"]).sigmoid(), rot_cos=t(case["rot"][:, 0:1]), rot_sin=t(case["rot"][:, 1:2]),
        center=t(case["center"]), center_z=t(case["center_z"]), dim=t(case["dim"]).exp(), vel=t(case["vel"]),
        point_cloud_range=np.array(cdr.RANGE_LO + [0.0] * 4, np.float32), voxel_size=list(cdr.VOXEL_SIZE),
        feature_map_stride=cdr.STRIDE, K=case["k"], circle_nms=False, score_thresh=case["score_thresh"],
        post_center_limit_range=torch.tensor(case["limit"], dtype=torch.float32))
    for f, d in enumerate(out):
        m = got["keep"][f].astype(bool)
        assert len(d["pred_scores"]) == m.sum() == got["count"][f]
        np.testing.assert_array_equal(d["pred_labels"].numpy(), got["labels"][f][m])
        boxes = d["pred_boxes"].numpy()
        np.testing.assert_array_equal(boxes[:, :3], got["boxes"][f][m][:, :3])
        np.testing.assert_array_equal(boxes[:, 7:], got["boxes"][f][m][:, 7:])
        np.testing.assert_allclose(boxes[:, 3:7], got["boxes"][f][m][:, 3:7], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(d["pred_scores"].numpy(), got["scores"][f][m], rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------------------ the ABI

def _fake(n):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def _call(lib, _lib, b=2, c=3, h=20, w=24, k=16, null=None, vel=True):
    ptrs = _fake(13)
    if null is not None:
        ptrs[null] = None
    hm, center, cz, dim, rot, v, boxes, scores, labels, cells, keep, count, ws = ptrs
    return lib.spx_center_decode(hm, center, cz, dim, rot, v if vel else None, b, c, h, w, k, 8.0,
                                 _lib.f_arr([0.05, 0.05]), _lib.f_arr([0.0, -4.0]), _lib.f_arr([0.0] * 6), 0.1, 1, 1,
                                 boxes, scores, labels, cells, keep, count, ws, 1 << 24, None)


def test_symbols_exported_and_workspace_positive():
    from spx import _lib
    lib = _lib.load()
    assert hasattr(lib, "spx_center_decode") and hasattr(lib, "spx_center_decode_ws_bytes")
    assert lib.spx_abi_version() == _lib.SPX_ABI_VERSION
    assert set(_lib.SIGNATURES) >= {"spx_center_decode", "spx_center_decode_ws_bytes"}
    small = lib.spx_center_decode_ws_bytes(2, 3, 20, 24, 16)
    kitti = lib.spx_center_decode_ws_bytes(4, 3, 200, 176, 500)
    assert small > 0 and kitti >= 4 * 13 * 500 * 8
    assert lib.spx_center_decode_ws_bytes(1, 3, 468, 468, 500) >= (81 + 6) * 500 * 8


def test_argument_validation_without_gpu():
    from spx import _lib
    lib = _lib.load()
    for null in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11):        # every required input and output pointer
        assert _call(lib, _lib, null=null) == -1, null
    assert _call(lib, _lib, k=0) == -1
    assert _call(lib, _lib, k=20 * 24 + 1) == -1                # K > H * W
    assert _call(lib, _lib, h=40, w=40, k=1025) == -5           # K > 1024: SPX_ERR_TOO_LARGE
    assert _call(lib, _lib, c=0) == -1 and _call(lib, _lib, b=-1) == -1
    assert _call(lib, _lib, c=4, h=1 << 15, w=1 << 14) == -5    # C * H * W = 2^31
    assert _call(lib, _lib, null=12, c=3, h=200, w=176, k=500) == -2    # no workspace
    assert _call(lib, _lib, b=0) == 0                           # nothing to do, nothing launched
    assert _call(lib, _lib, b=0, vel=False) == 0


def test_ops_center_decode_refuses_cpu_tensors_and_bad_shapes():
    from spx import _lib, ops
    case = CASES["odd_sizes"]
    t = lambda a: None if a is None else torch.from_numpy(a)                     # noqa: E731
    args = [t(case[k]) for k in ("hm", "center", "center_z", "dim", "rot", "vel")]
    with pytest.raises(_lib.SpxError):
        ops.center_decode(*args, case["k"], cdr.STRIDE, cdr.VOXEL_SIZE, cdr.RANGE_LO, case["limit"], 0.1)
    assert ops.CENTER_DECODE_MAX_K == 1024
