"""The static-capacity voxel-row entry points (include/spx.h §19) are exported and check their arguments on the host,
before any launch; the wrappers and the graphed runner refuse what they cannot run.  No GPU."""
import ctypes

import pytest
import torch


def _fake(n):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def _table(lib, _lib, null=None, cap=32, batch=2, shape=(4, 8, 8)):
    idx, table = _fake(2)
    shape3 = None if shape is None else _lib.i3(shape)
    if null == 0:
        idx = None
    if null == 1:
        table = None
    return lib.spx_voxel_table_build(idx, cap, None, batch, shape3, table, None, None)


def _mean(lib, _lib, null=None, batch=2, c=5, m=16, shape=(4, 8, 8), lo=(0.0, 0.0, 0.0), vs=(1.0, 1.0, 1.0), cap=32,
          ws_bytes=1 << 20):
    ptrs = _fake(5)
    if null is not None:
        ptrs[null] = None
    xyz, feats, table, out, ws = ptrs
    return lib.spx_voxel_rows_mean(xyz, feats, batch, c, m, table, None if shape is None else _lib.i3(shape),
                                   None if lo is None else _lib.f_arr(lo), None if vs is None else _lib.f_arr(vs), None,
                                   cap, out, ws, ws_bytes, None)


def test_symbols_exported():
    from spx import _lib
    lib = _lib.load()
    for name in ("spx_voxel_table_build", "spx_voxel_rows_mean", "spx_voxel_rows_mean_ws_bytes"):
        assert hasattr(lib, name), name
    assert lib.spx_voxel_rows_mean_ws_bytes(2, 4096) >= 3 * 2 * 4096 * 4
    assert lib.spx_voxel_rows_mean_ws_bytes(0, 16) == 0 and lib.spx_voxel_rows_mean_ws_bytes(2, 0) == 0
    assert len(lib.spx_strerror(-9)) > 4 and b"unknown" not in lib.spx_strerror(-9)


def test_table_build_argument_validation():
    from spx import _lib
    lib = _lib.load()
    assert _table(lib, _lib, null=0) == -1 and _table(lib, _lib, null=1) == -1 and _table(lib, _lib, shape=None) == -1
    for cap in (0, -1):
        assert _table(lib, _lib, cap=cap) == -1
    for batch in (0, -2):
        assert _table(lib, _lib, batch=batch) == -1
    for shape in ((0, 8, 8), (4, -1, 8), (4, 8, 0)):
        assert _table(lib, _lib, shape=shape) == -1
    assert _table(lib, _lib, cap=1 << 31) == -5
    assert _table(lib, _lib, batch=1 << 10, shape=(1 << 10, 1 << 10, 1 << 10)) == -5


def test_rows_mean_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for null in range(4):                                   # new_xyz, feats, table, out
        assert _mean(lib, _lib, null=null) == -1, null
    assert _mean(lib, _lib, shape=None) == -1 and _mean(lib, _lib, lo=None) == -1 and _mean(lib, _lib, vs=None) == -1
    for bad in (0, -1):
        assert _mean(lib, _lib, batch=bad) == -1 and _mean(lib, _lib, c=bad) == -1 and _mean(lib, _lib, m=bad) == -1
        assert _mean(lib, _lib, cap=bad) == -1
    assert _mean(lib, _lib, shape=(4, 0, 8)) == -1
    assert _mean(lib, _lib, vs=(1.0, 0.0, 1.0)) == -1 and _mean(lib, _lib, vs=(1.0, 1.0, -0.5)) == -1
    assert _mean(lib, _lib, m=4097) == -5                   # a frame's keys must fit in LDS
    assert _mean(lib, _lib, shape=(1 << 11, 1 << 10, 1 << 10)) == -5
    assert _mean(lib, _lib, null=4) == -2 and _mean(lib, _lib, ws_bytes=16) == -2


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from spx import _lib, ops
    idx = torch.zeros((8, 4), dtype=torch.int32)
    with pytest.raises(_lib.SpxError):
        ops.voxel_table_build(idx, 1, [2, 2, 2])
    with pytest.raises(_lib.SpxError):
        ops.voxel_rows_mean(torch.zeros(1, 4, 3), torch.zeros(1, 2, 4), torch.zeros((1, 2, 2, 2), dtype=torch.int32),
                            [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 8)
    assert ops.VOXEL_ROWS_MAX_M == 4096


def _cpu_model(train):
    import point_head_configs as phc
    from pcdet_amd.models.detectors import build_detector
    torch.manual_seed(0)
    net = build_detector(phc.model_cfg(), 3, phc.dataset())
    return net.train(train)


def test_graphed_point_detector_refuses_train_mode_and_wrong_point_count():
    from pcdet_amd.models.inference import GraphedPointDetector
    with pytest.raises(ValueError, match="eval"):
        GraphedPointDetector(_cpu_model(True), 2, 128)
    net = _cpu_model(False)
    for shape in ((2 * 128 - 1, 5), (2 * 128 + 2, 5), (2 * 128, 4)):
        with pytest.raises(ValueError, match="exactly 128 points"):
            GraphedPointDetector(net, 2, 128, example=torch.zeros(shape))


def test_static_mode_is_inference_only_by_name():
    """The static path refuses train mode and autograd before it touches a device."""
    import sa_configs
    from pcdet_amd.ops.pointnet2.pointnet2_batch import pointnet2_modules as pm
    m = pm.VoxelPointnetSAModuleFSMSGDistillation(**sa_configs.layer0())
    xyz, feats = torch.zeros(1, 64, 3), torch.zeros(1, 1, 64)
    with pytest.raises(RuntimeError, match="inference only"):
        m.train()(xyz, feats, static=True)
    with pytest.raises(RuntimeError, match="inference only"):
        m.eval()(xyz, feats, static=True)                   # grad enabled
    net = _cpu_model(False)
    with pytest.raises(RuntimeError, match="inference only"):
        net.backbone_3d({"batch_size": 1, "points": torch.zeros(64, 5), "static_caps": {}})
    with torch.no_grad(), pytest.raises(ValueError, match="equal"):
        net.backbone_3d({"batch_size": 3, "points": torch.zeros(64, 5), "static_caps": {}})
