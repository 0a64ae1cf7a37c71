"""Stacked point ops without a GPU: the numpy restatement (tests/pointnet2_stack_ref.py) against plain-Python simulations
of the reference's per-thread scans, the modules' state_dict keys against the list recorded from the reference, and the
host-side checks of the C ABI, the operator layer and the python wrappers."""
import ctypes
import json
import os

import numpy as np
import pytest

import pointnet2_stack_ref as ref
from stack_configs import CLASS_OF, INSTANCES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack_module_state_keys.json")


def lattice(n, seed):
    """integer coordinates in [0, 3): 27 distinct positions, so almost every comparison is a tie"""
    return np.random.default_rng(seed).integers(0, 3, size=(n, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------- restatement vs simulation

@pytest.mark.parametrize("radius", [0.0, 0.5, 1.1, 1.5, 200.0])
@pytest.mark.parametrize("nsample", [1, 5])
def test_ball_query_restatement_equals_reference_scan(radius, nsample):
    xyz_cnt, new_cnt = [40, 1, 0, 29], [17, 6, 3, 0]
    xyz, new_xyz = lattice(sum(xyz_cnt), 1), lattice(sum(new_cnt), 2)
    new_xyz[::3] += np.float32(0.5)     # off-lattice centres too: balls that miss everything at small radii
    idx, empty = ref.ball_query(xyz, xyz_cnt, new_xyz, new_cnt, radius, nsample)
    idx_s, empty_s = ref.ball_query_simulate_reference(xyz, xyz_cnt, new_xyz, new_cnt, radius, nsample)
    assert np.array_equal(idx, idx_s) and np.array_equal(empty, empty_s)
    if radius == 0.0:
        assert empty.all()
    if radius == 200.0:
        assert not empty[:17].any() and empty[23:26].all()      # the frame without points has only empty balls


def test_ball_query_dead_rows():
    xyz_cnt, new_cnt = [20, 10], [5, 4]
    xyz, new_xyz = lattice(30 + 7, 3), lattice(9 + 5, 4)
    idx, empty = ref.ball_query(xyz, xyz_cnt, new_xyz, new_cnt, 1.1, 4)
    idx_l, empty_l = ref.ball_query(xyz[:30], xyz_cnt, new_xyz[:9], new_cnt, 1.1, 4)
    assert np.array_equal(idx[:9], idx_l) and np.array_equal(empty[:9], empty_l)
    assert not idx[9:].any() and empty[9:].all()


def test_stack_fps_restatement_equals_reference_threads():
    """frames smaller than the 1024 threads and larger; after 27 picks every remaining distance is 0: ties only"""
    xyz_cnt, npoint = [1, 63, 1500, 1024], [3, 40, 45, 33]
    xyz = lattice(sum(xyz_cnt), 5)
    got = ref.stack_furthest_point_sample(xyz, xyz_cnt, npoint)
    want = ref.fps_simulate_reference(xyz, xyz_cnt, npoint)
    assert got.shape == (sum(npoint),) and np.array_equal(got, want)
    starts = np.cumsum([0] + xyz_cnt)
    o = 0
    for f, m in enumerate(npoint):
        assert got[o] == starts[f] and (got[o:o + m] >= starts[f]).all() and (got[o:o + m] < starts[f + 1]).all()
        o += m


def test_stack_fps_empty_frame_picks_its_start():
    xyz = lattice(10, 6)
    got = ref.stack_furthest_point_sample(xyz, [4, 0, 6], [2, 3, 2])
    assert list(got[2:5]) == [4, 4, 4] and got[0] == 0 and got[5] == 4


def test_three_nn_and_grouping_restatement():
    unknown_cnt, known_cnt = [6, 3, 4], [5, 2, 0]
    unknown, known = lattice(13 + 2, 7), lattice(7 + 3, 8)
    d2, idx = ref.three_nn(unknown, unknown_cnt, known, known_cnt)
    for q in range(13):
        f = 0 if q < 6 else (1 if q < 9 else 2)
        s, e = [0, 5, 7][f], [5, 7, 7][f]
        best = []
        for k in range(s, e):                      # strict-< insertion in ascending k
            d = ref.sq_dist(unknown[q], known[k])
            pos = len(best)
            while pos > 0 and d < best[pos - 1][0]:
                pos -= 1
            best.insert(pos, (d, k))
        best = best[:3] + [(np.float32(np.inf), s)] * (3 - min(len(best), 3))
        assert [b[1] for b in best] == list(idx[q]) and [b[0] for b in best] == list(d2[q])
    assert np.isinf(d2[13:]).all() and not idx[13:].any()
    feats = np.random.default_rng(9).standard_normal((10, 3)).astype(np.float32)
    gidx = np.array([[0, 4, 5, -1]] * 6 + [[1, 0, 2, 0]] * 3 + [[0, 0, 0, 0]] * 4 + [[1, 1, 1, 1]] * 2, np.int32)
    out = ref.group_points(feats, known_cnt, gidx, unknown_cnt)
    assert out.shape == (15, 3, 4)
    assert np.array_equal(out[0, :, 1], feats[4]) and not out[0, :, 2].any() and not out[0, :, 3].any()
    assert np.array_equal(out[6, :, 0], feats[6]) and not out[6, :, 2].any()
    assert not out[9:].any()                        # a frame without sources, then dead rows


# ------------------------------------------------------------------------------------------- modules and names

def _module_class(name):
    from pcdet_amd.ops.pointnet2.pointnet2_stack import pointnet2_modules, voxel_pool_modules
    return getattr(pointnet2_modules, CLASS_OF[name], None) or getattr(voxel_pool_modules, CLASS_OF[name])


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_state_dict_keys_and_shapes_match_reference(name):
    want = json.load(open(GOLDEN))[name]
    got = [[k, list(v.shape)] for k, v in _module_class(name)(**INSTANCES[name]()).state_dict().items()]
    assert got == want


def test_public_names_and_pcdet_alias():
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tsm-det-pointcloud-_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as a
    from pcdet_amd.ops.pointnet2.pointnet2_stack import pointnet2_utils as b
    from pcdet_amd.ops.pointnet2.pointnet2_batch import pointnet2_utils as batch
    assert a is b
    for name in ("ball_query", "grouping_operation", "QueryAndGroup", "farthest_point_sample", "furthest_point_sample",
                 "stack_farthest_point_sample", "three_nn", "three_interpolate"):
        assert callable(getattr(a, name)), name
    assert a.farthest_point_sample is batch.furthest_point_sample is a.furthest_point_sample


def test_vector_pool_names_raise():
    from pcdet_amd.config import AttrDict as EasyDict
    from pcdet_amd.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm, pointnet2_utils as pu
    for fn in (pu.three_nn_for_vector_pool_by_two_step, pu.vector_pool_with_voxel_query_op):
        with pytest.raises(NotImplementedError, match="vector pooling"):
            fn(None, None)
    with pytest.raises(NotImplementedError, match="vector pooling"):
        pm.build_local_aggregation_module(4, EasyDict(NAME="VectorPoolAggregationModuleMSG"))
    layer, c_out = pm.build_local_aggregation_module(
        4, EasyDict(NAME="StackSAModuleMSG", MLPS=[[8, 8], [8, 16]], POOL_RADIUS=[0.4, 0.8], NSAMPLE=[4, 8]))
    assert isinstance(layer, pm.StackSAModuleMSG) and c_out == 24
    assert layer.mlps[0][0].weight.shape == (8, 7, 1, 1)


# ------------------------------------------------------------------------------------------- host-side checks

def _entry_points():
    """name -> call(b, rows, p): every new entry point with b frames, `rows` rows on both sides and p for every pointer"""
    from spx import _lib
    lib = _lib.load()
    return {
        "ball_query": lambda b, r, p: lib.spx_stack_ball_query(p, p, p, p, b, r, r, 0.5, 4, p, p, None),
        "group_points": lambda b, r, p: lib.spx_stack_group_points(p, p, p, p, b, r, r, 8, 4, p, None),
        "group_points_bwd": lambda b, r, p: lib.spx_stack_group_points_bwd(p, p, p, p, b, r, r, 8, 4, p, p, 1 << 30, None),
        "three_nn": lambda b, r, p: lib.spx_stack_three_nn(p, p, p, p, b, r, r, p, p, None),
        "three_interpolate": lambda b, r, p: lib.spx_stack_three_interpolate(p, p, p, p, b, r, r, 8, p, None),
        "three_interpolate_bwd": lambda b, r, p: lib.spx_stack_three_interpolate_bwd(p, p, p, p, b, r, r, 8, p, p, 1 << 30,
                                                                                    None),
        "furthest_point_sample": lambda b, r, p: lib.spx_stack_furthest_point_sample(p, p, p, b, r, r, p, p, 1 << 30, None),
    }


@pytest.mark.parametrize("name", ["ball_query", "group_points", "group_points_bwd", "three_nn", "three_interpolate",
                                  "three_interpolate_bwd", "furthest_point_sample"])
def test_argument_checks_return_before_any_launch(name):
    call = _entry_points()[name]
    somewhere = ctypes.c_void_p(4096)            # never dereferenced: each of these calls returns on the host
    assert call(2, 100, None) == -1              # null pointers
    assert call(257, 100, somewhere) == -3       # more than 256 frames
    assert call(257, 0, somewhere) == -3
    assert call(2, 0, somewhere) == 0            # no rows: nothing to do
    assert call(2, -1, somewhere) == -1


def test_ws_bytes():
    from spx import _lib
    lib = _lib.load()
    assert lib.spx_abi_version() == 3
    total, n, c = 1000 * 16, 500, 64
    assert lib.spx_stack_group_points_bwd_ws_bytes(n, 1000, c, 16) >= 4 * total * 4 + 2 * n * 4 + 2 * (total // 128) * c * 4
    assert lib.spx_stack_three_interpolate_bwd_ws_bytes(n, 1000, c) >= 4 * 3000 * 4 + 2 * n * 4
    assert lib.spx_stack_furthest_point_sample_ws_bytes(16384) == 0
    assert lib.spx_stack_furthest_point_sample_ws_bytes(65536) >= 65536 * 4


def test_ops_and_wrappers_refuse_cpu_tensors():
    import torch
    from spx import _lib, ops
    from pcdet_amd.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    xyz, cnt = torch.zeros((16, 3)), torch.tensor([10, 6], dtype=torch.int32)
    feats = torch.zeros((16, 4))
    idx, w = torch.zeros((16, 3), dtype=torch.int32), torch.zeros((16, 3))
    calls = [lambda: ops.stack_ball_query(xyz, cnt, xyz, cnt, 0.5, 3), lambda: ops.stack_group_points(feats, cnt, idx, cnt),
             lambda: ops.stack_group_points_bwd(torch.zeros((16, 4, 3)), cnt, idx, cnt, 16),
             lambda: ops.stack_three_nn(xyz, cnt, xyz, cnt), lambda: ops.stack_three_interpolate(feats, idx, w),
             lambda: ops.stack_three_interpolate_bwd(feats, idx, w, 16),
             lambda: ops.stack_furthest_point_sample(xyz, cnt, cnt, 16),
             lambda: pu.ball_query(0.5, 3, xyz, cnt, xyz, cnt), lambda: pu.grouping_operation(feats, cnt, idx, cnt),
             lambda: pu.QueryAndGroup(0.5, 3)(xyz, cnt, xyz, cnt, feats), lambda: pu.three_nn(xyz, cnt, xyz, cnt),
             lambda: pu.three_interpolate(feats, idx, w), lambda: pu.stack_farthest_point_sample(xyz, cnt, 4),
             lambda: pu.stack_farthest_point_sample(xyz, cnt, [4, 2]), lambda: pu.farthest_point_sample(xyz[None], 4)]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.SpxError):
            call()
