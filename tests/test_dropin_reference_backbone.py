"""Boundary B2 drop-in: the REFERENCE's unmodified VoxelBackBone8x / VoxelResBackBone8x / UNetV2 / HeightCompression source
files, run with our `spconv` compat alias (tsm-det-pointcloud-_amd/compat) in place of the spconv wheel and loaded with our
modules' weights, build the same state_dict and produce the same outputs as our modules.  The reference side is stored in
tests/golden/ref_dropin.npz (made by tests/golden/make_golden_dropin.py from a checkout of the reference); sparse ops go
through the oracle backend (no GPU)."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL, ATOL = 1e-5, 1e-5        # oracle arithmetic is float32 numpy: bitwise here, BLAS rounding may differ on other CPUs


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "ref_dropin.npz"))


def _same(G, name, a):
    """`a` against the stored reference array `name`: exact for integers, to RTOL / ATOL for floats; arrays stored as a
    row sample are checked on those rows, on every row's projection on two fixed directions, on every column's sum, and
    on their shape."""
    a = np.asarray(a)
    if name + "_rows" not in G.files:
        if a.dtype.kind == "f":
            np.testing.assert_allclose(a, G[name], rtol=RTOL, atol=ATOL, err_msg=name)
        else:
            assert a.shape == G[name].shape and np.array_equal(a, G[name]), name
        return
    assert a.shape == tuple(G[name + "_shape"]), name
    rows = a.reshape(a.shape[0], -1)
    np.testing.assert_allclose(rows[G[name + "_rowidx"]], G[name + "_rows"], rtol=RTOL, atol=ATOL, err_msg=name)
    r = G[name + "_projmat"]
    rows64 = rows.astype(np.float64)
    err = np.abs(rows64 @ r - G[name + "_proj"])
    bound = RTOL * (np.abs(rows64) @ np.abs(r)) + ATOL * np.abs(r).sum(0)      # per row: elementwise RTOL / ATOL, summed
    assert (err <= bound).all(), "%s: %d rows differ" % (name, int((err > bound).any(1).sum()))
    np.testing.assert_allclose(rows64.sum(0), G[name + "_colsum"], rtol=RTOL, atol=ATOL * rows.shape[0],
                               err_msg=name + " column sums")


def _state_dict_matches(G, prefix, module, shapes=True):
    sd = module.state_dict()
    assert list(sd.keys()) == list(G[prefix + "keys"])
    if shapes:
        assert ["x".join(str(s) for s in v.shape) for v in sd.values()] == list(G[prefix + "shapes"])


def _vox(ds, b, bsz):
    from spx import ops
    vox = ops.voxelize(torch.from_numpy(b["points"]), ds.point_cloud_range, ds.voxel_size, 5, 16000, batch_size=bsz,
                       batch_col=0, xyz_col=1, feat_col=1, want_voxels=False)
    return vox, {"voxel_features": vox["mean"], "voxel_coords": vox["coords"].float(), "batch_size": bsz}


def test_reference_voxelbackbone8x_runs_on_spx(G):
    from oracle.cpu_backend import use_oracle_backend
    from pcdet_amd.config import AttrDict
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models.backbones_2d.map_to_bev import HeightCompression
    from pcdet_amd.models.backbones_3d import VoxelBackBone8x
    ds = SyntheticDataset(cfg_id=0)
    torch.manual_seed(0)
    ours = VoxelBackBone8x(AttrDict(), 4, ds.grid_size)
    _state_dict_matches(G, "bb8x_", ours)
    ours.eval()
    with torch.no_grad(), use_oracle_backend():
        _vox_out, bd = _vox(ds, ds.collate_batch([ds[0], ds[1]]), 2)
        out_o = HeightCompression(AttrDict(NUM_BEV_FEATURES=256))(ours(dict(bd)))
    for k in ("x_conv1", "x_conv2", "x_conv3", "x_conv4"):
        c = out_o["multi_scale_3d_features"][k]
        _same(G, "bb8x_%s_indices" % k, c.indices.numpy())
        _same(G, "bb8x_%s_features" % k, c.features.numpy())
    sf = out_o["spatial_features"].numpy()
    assert sf.shape == (2, 256, 40, 32) and sf.shape == tuple(G["bb8x_spatial_shape"])
    _same(G, "bb8x_spatial_features", sf.transpose(0, 2, 3, 1).reshape(-1, sf.shape[1]))
    assert out_o["encoded_spconv_tensor_stride"] == 8 == int(G["bb8x_stride"])


def test_reference_voxelresbackbone8x_runs_on_spx(G):
    """Row f-3: the reference's residual backbone (SparseBasicBlock, bias=True convs, 128-wide stage) on our operators."""
    from oracle.cpu_backend import use_oracle_backend
    from pcdet_amd.config import AttrDict
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models.backbones_3d import VoxelResBackBone8x
    ds = SyntheticDataset(cfg_id=0)
    torch.manual_seed(1)
    ours = VoxelResBackBone8x(AttrDict(), 4, ds.grid_size)
    _state_dict_matches(G, "res_", ours, shapes=False)
    ours.eval()
    with torch.no_grad(), use_oracle_backend():
        _vox_out, bd = _vox(ds, ds.collate_batch([ds[0]]), 1)
        o = ours(dict(bd))
    for k in ("x_conv1", "x_conv2", "x_conv3", "x_conv4"):
        _same(G, "res_%s_features" % k, o["multi_scale_3d_features"][k].features.numpy())
    _same(G, "res_encoded_features", o["encoded_spconv_tensor"].features.numpy())
    assert o["encoded_spconv_tensor"].features.shape[1] == 128


def test_reference_unetv2_runs_on_spx(G):
    """Row f-3: the reference's UNetV2 source (SparseInverseConv3d, 128->64 SubM, k=1 SparseConv3d) on our operators,
    against our own UNetV2: same state_dict, the same outputs."""
    from oracle.cpu_backend import use_oracle_backend
    from pcdet_amd.config import AttrDict
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models.backbones_3d import UNetV2
    ds = SyntheticDataset(cfg_id=0)
    torch.manual_seed(2)
    kw = dict(voxel_size=ds.voxel_size, point_cloud_range=ds.point_cloud_range)
    ours = UNetV2(AttrDict(), 4, ds.grid_size, **kw)
    _state_dict_matches(G, "unet_", ours)
    ours.eval()
    with torch.no_grad(), use_oracle_backend():
        vox, bd = _vox(ds, ds.collate_batch([ds[0]]), 1)
        o = ours(dict(bd))
    assert o["point_features"].shape == (vox["coords"].shape[0], 16)
    _same(G, "unet_point_features", o["point_features"].numpy())
    _same(G, "unet_raw_points_bxyz", o["raw_points_bxyz"].numpy())
    _same(G, "unet_encoded_features", o["encoded_spconv_tensor"].features.numpy())
    _same(G, "unet_encoded_indices", o["encoded_spconv_tensor"].indices.numpy())
