"""The roipoint_pool3d restatement (tests/roipoint_pool3d_ref.py) against a brute-force loop written straight from the
semantics, and the torch composition pcdet_amd.ops.roipoint_pool3d.roipoint_pool3d_utils.roipoint_pool3d_torch against the
restatement: exact in plain mode.  No GPU."""
import numpy as np
import pytest
import torch

import roipoint_pool3d_ref as R
import roipoint_pool_cases as K


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _torch(case, width, s):
    from pcdet_amd.ops.roipoint_pool3d.roipoint_pool3d_utils import roipoint_pool3d_torch
    out, flag = roipoint_pool3d_torch(torch.from_numpy(case["points"]), torch.from_numpy(case["feats"]),
                                      torch.from_numpy(case["boxes"]), width, s)
    return out.numpy(), flag.numpy()


def test_edge_scene_is_what_it_claims():
    case = K.edge_case()
    _, cnt = R.pooled_indices(case["points"], case["boxes"], 0.0, K.EDGE_S)
    for box, want in case["expected"].items():
        assert tuple(cnt[:, box]) == want, (box, cnt[:, box])
    assert cnt[0, 8] == cnt[0, 9] and 0 < cnt[0, 10] < 24            # +pi and -pi hold the same points; 30 degrees cuts
    _, grown = R.pooled_indices(case["points"], case["boxes"], K.ROUNDING_WIDTH, K.EDGE_S)
    assert tuple(grown[:, 11]) == (1, 1)                              # inside only through the float32 add
    exact = np.float64(1.0) + np.float64(np.float32(0.1))
    assert np.float64(K.ROUNDING_HALF) > exact / 2.0                  # a float64 add would leave the point outside


@pytest.mark.parametrize("width", [0.0, K.ROUNDING_WIDTH, [0.3, 0.0, 0.05]])
def test_restatement_equals_brute_force_on_the_edge_scene(width):
    case = K.edge_case()
    for s in (1, K.EDGE_S, 11):
        out, flag = R.roipoint_pool3d(case["points"], case["feats"], case["boxes"], width, s)
        ref, ref_flag = R.brute_force(case["points"], case["feats"], case["boxes"], width, s)
        assert _same(out, ref) and np.array_equal(flag, ref_flag)
        got, got_flag = _torch(case, width, s)
        assert _same(got, ref) and np.array_equal(got_flag, ref_flag) and got_flag.dtype == np.int32


@pytest.mark.parametrize("n", K.SWEEP_N)
@pytest.mark.parametrize("m", K.SWEEP_M)
def test_sweep(n, m):
    for ci, c in enumerate(K.SWEEP_C):
        case = K.sweep_case(n, m, c, 7 if (ci + m) % 2 else 9, seed=100 * n + 10 * m + ci)
        for s in K.SWEEP_S:
            out, flag = R.roipoint_pool3d(case["points"], case["feats"], case["boxes"], 0.0, s)
            if c == 1 or s == 8:
                ref, ref_flag = R.brute_force(case["points"], case["feats"], case["boxes"], 0.0, s)
                assert _same(out, ref) and np.array_equal(flag, ref_flag)
            got, got_flag = _torch(case, 0.0, s)
            assert _same(got, out) and np.array_equal(got_flag, flag)
            assert flag[0, 0] == 0 and (m == 1 or flag[0, 1] == 1)


def test_long_scene_and_degenerate_shapes():
    case = K.long_case()
    out, flag = R.roipoint_pool3d(case["points"], case["feats"], case["boxes"], 0.0, 600)
    _, cnt = R.pooled_indices(case["points"], case["boxes"], 0.0, 600)
    assert (cnt[:, 0] == 2500).all() and (cnt[:, 1] > 600).all() and ((cnt[:, 2] > 0) & (cnt[:, 2] < 600)).all()
    assert (cnt[:, 3] == 0).all()
    got, got_flag = _torch(case, 0.0, 600)
    assert _same(got, out) and np.array_equal(got_flag, flag)
    empty = dict(points=np.zeros((2, 0, 3), np.float32), feats=np.zeros((2, 0, 4), np.float32),
                 boxes=np.ones((2, 3, 7), np.float32))
    got, got_flag = _torch(empty, 0.0, 5)
    assert got.shape == (2, 3, 5, 7) and not got.any() and (got_flag == 1).all()
    out, flag = R.roipoint_pool3d(empty["points"], empty["feats"], empty["boxes"], 0.0, 5)
    assert _same(got, out) and np.array_equal(got_flag, flag)


def test_canonical_restatement_matches_its_definition():
    """The canonical columns, one RoI by hand: centre subtracted, rotated by -heading, depth from the untransformed
    point; empty RoIs are zero rows; score and features are copies."""
    case = K.edge_case()
    can, flag = R.canonical(case["points"], case["feats"], case["scores"], case["boxes"], 0.0, K.EDGE_S, 70.0)
    plain, flag2 = R.roipoint_pool3d(case["points"], case["feats"], case["boxes"], 0.0, K.EDGE_S)
    assert np.array_equal(flag, flag2) and can.shape == (24, K.EDGE_S, 5 + 5)
    plain = plain.reshape(24, K.EDGE_S, -1)
    assert np.array_equal(can[..., 5:], plain[..., 3:].astype(np.float64))
    r = 10                                                            # frame 0, the 30 degree box
    box = case["boxes"][0, r].astype(np.float64)
    p = plain[r, :, :3].astype(np.float64)
    h = box[6]
    back = np.stack([can[r, :, 0] * np.cos(h) - can[r, :, 1] * np.sin(h),
                     can[r, :, 0] * np.sin(h) + can[r, :, 1] * np.cos(h), can[r, :, 2]], axis=1) + box[:3]
    assert np.abs(back - p).max() < 1e-12
    assert np.abs(can[r, :, 4] - (np.linalg.norm(p, axis=1) / 70.0 - 0.5)).max() < 1e-15
    assert not can[flag.reshape(-1) == 1].any()


def test_module_on_cpu_and_width_forms():
    from pcdet_amd.ops.roipoint_pool3d.roipoint_pool3d_utils import RoIPointPool3d
    case = K.edge_case()
    args = [torch.from_numpy(case[k]) for k in ("points", "feats", "boxes")]
    a, fa = RoIPointPool3d(K.EDGE_S, 0.1)(*args)
    b, fb = RoIPointPool3d(K.EDGE_S, [0.1, 0.1, 0.1])(*args)
    assert torch.equal(a, b) and torch.equal(fa, fb) and fa.dtype == torch.int32
    ref, ref_flag = R.roipoint_pool3d(case["points"], case["feats"], case["boxes"], 0.1, K.EDGE_S)
    assert _same(a.numpy(), ref) and np.array_equal(fa.numpy(), ref_flag)
    with pytest.raises(ValueError, match="pool_extra_width"):
        RoIPointPool3d(K.EDGE_S, [0.1, 0.2])(*args)
    with pytest.raises(ValueError, match="pool_extra_width"):
        RoIPointPool3d(K.EDGE_S, -1.0)(*args)
