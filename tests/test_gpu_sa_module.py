"""Fused gather-project (csrc/group_project.hip) and the voxel-point SA modules built on it, on the GPU.

Op: forward and all three gradients against the float64 restatement (tests/group_project_ref.py) at the fast_cpc
layer-0 and layer-1 shapes (batch 2), empty columns exactly 0, every output element written, bitwise-repeatable
gradients, graph capture.  Modules: layer 0 (point branch) and layer 1 (voxel branch + sparse U-Net), train and eval,
against the unfused transcription of the reference forward (tests/sa_module_ref.py) with the same weights; the backbone
at the fast_cpc KITTI config, batch 2.

Tolerances (fp32 kernels vs float64 / vs the unfused fp32 composition):
  op forward      max|err| <= 2e-5 * (1 + max|y|)
  op gradients    ||err|| / ||ref|| <= 2e-5 (dF, dWf) and 1e-4 (dWx, a sum over ~0.3 M columns)
  module          features / scores ||err|| / ||ref|| <= 1e-4; parameter gradients <= 2e-3 (BatchNorm in train mode
                  divides by per-batch deviations and max pooling picks one of near-equal maxima)."""
import ctypes

import numpy as np
import pytest
import torch

import group_project_ref as gp
import sa_configs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _pu():
    from pcdet_amd.ops.pointnet2.pointnet2_batch import pointnet2_utils as pu
    return pu


# ------------------------------------------------------------------------------------------------------ the op
SHAPES = {
    # name: (batch, n_src, npoint, nsample, c_in, c_out, form)
    "layer0": (2, 16384, 4096, 32, 1, 16, "both"),
    "layer0_r3": (2, 16384, 4096, 32, 1, 32, "both"),
    "layer1_point_mlp": (2, 3000, 512, 32, 64, 32, "wf_only"),
    "layer1_pos_mlp": (2, 3000, 512, 32, 64, 64, "wx_only"),
    "odd": (3, 101, 7, 5, 3, 5, "both"),
}


def _case(name, seed=0):
    batch, n, npoint, nsample, c_in, c_out, form = SHAPES[name]
    rng = np.random.default_rng(seed)
    c = gp.make_case(rng, batch, n, npoint, nsample, c_in, c_out, empty_frac=0.1)
    Wf = None if form == "wx_only" else c["W"][:, 3:]
    Wx = None if form == "wf_only" else c["W"][:, :3]
    F = None if form == "wx_only" else c["F"]
    dy = rng.standard_normal((batch, c_out, npoint, nsample)).astype(np.float32)
    return c, F, Wf, Wx, dy, batch


def _run_op(c, F, Wf, Wx, dy, batch):
    pu = _pu()
    Ft = None if F is None else _g(F).requires_grad_(True)
    Wft = None if Wf is None else _g(Wf).requires_grad_(True)
    Wxt = None if Wx is None else _g(Wx).requires_grad_(True)
    y = pu.group_project(Ft, Wft, Wxt, _g(c["xyz"]), _g(c["ctr"]), _g(c["idx"]), _g(c["empty"]), batch)
    y.backward(_g(dy))
    return y.detach(), [None if t is None else t.grad.detach().clone() for t in (Ft, Wft, Wxt)]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_op_matches_float64_restatement(name):
    c, F, Wf, Wx, dy, batch = _case(name)
    y, (dF, dWf, dWx) = _run_op(c, F, Wf, Wx, dy, batch)
    y_ref = gp.forward(F, Wf, Wx, c["xyz"], c["ctr"], c["idx"], c["empty"], batch)
    err = float(np.abs(y.cpu().numpy() - y_ref).max())
    assert err <= 2e-5 * (1 + np.abs(y_ref).max()), err
    rF, rWf, rWx = gp.backward(dy, F, Wf, Wx, c["xyz"], c["ctr"], c["idx"], c["empty"])
    if F is not None:
        assert _rel(dF, torch.from_numpy(rF)) <= 2e-5
        assert _rel(dWf, torch.from_numpy(rWf)) <= 2e-5
    if Wx is not None:
        assert _rel(dWx, torch.from_numpy(rWx)) <= 1e-4


def test_empty_columns_are_exactly_zero():
    c, F, Wf, Wx, dy, batch = _case("layer0", seed=1)
    y, _ = _run_op(c, F, Wf, Wx, dy, batch)
    b, co, npoint, s = y.shape
    e = _g(c["empty"]).view(b, npoint)
    assert bool(e.any())
    assert bool((y.permute(0, 2, 1, 3)[e] == 0).all())
    assert bool(torch.isfinite(y).all())


def test_nan_prefilled_output_is_fully_overwritten():
    from spx import _lib
    from spx import ops
    c, F, Wf, Wx, dy, batch = _case("odd", seed=2)
    lib = _lib.load()
    p = _g(F) @ _g(Wf).t()
    y = torch.full(tuple(dy.shape), float("nan"), device=DEV)
    npoint, s = dy.shape[2], dy.shape[3]
    wx, xyz, ctr, idx = _g(Wx).contiguous(), _g(c["xyz"]), _g(c["ctr"]), _g(c["idx"])
    empty = _g(c["empty"].astype(np.uint8))

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    rc = lib.spx_group_project(ptr(p), ptr(wx), ptr(xyz), ptr(ctr), ptr(idx), ptr(empty), p.shape[1], p.shape[0], batch,
                               npoint, s, ptr(y), ops._stream(y))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool(torch.isfinite(y).all())
    want = ops.group_project(p, wx, xyz, ctr, idx, empty, batch)
    assert torch.equal(y, want)


def test_gradients_are_bitwise_repeatable():
    c, F, Wf, Wx, dy, batch = _case("layer0", seed=3)
    _, g1 = _run_op(c, F, Wf, Wx, dy, batch)
    _, g2 = _run_op(c, F, Wf, Wx, dy, batch)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def test_coordinates_requiring_grad_are_refused():
    c, F, Wf, Wx, dy, batch = _case("odd", seed=4)
    with pytest.raises(RuntimeError, match="coordinates"):
        _pu().group_project(_g(F), _g(Wf), _g(Wx), _g(c["xyz"]).requires_grad_(True), _g(c["ctr"]), _g(c["idx"]),
                            _g(c["empty"]), batch)


def test_graph_capture_replay():
    from spx import ops
    c, F, Wf, Wx, dy, batch = _case("layer1_point_mlp", seed=5)
    p = _g(F) @ _g(Wf).t()
    args = [_g(c["xyz"]), _g(c["ctr"]), _g(c["idx"]), _g(c["empty"])]
    g_dy = _g(dy)

    def step():
        y = ops.group_project(p, None, *args, batch)
        dpt, _ = ops.group_project_bwd(g_dy, None, None, args[2], args[3], p.shape[0], need_dwx=False)
        return y, dpt

    eager = step()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                      # warm the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g_dy.mul_(2.0)                                                  # replay sees the new gradient
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static[0], eager[0])
    assert torch.equal(static[1], eager[1] * 2.0)


# ------------------------------------------------------------------------------------------------------ modules
def _frames(batch, n, seed=0):
    """KITTI-shaped synthetic frames (x, y, z, intensity), n points each."""
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    out = []
    for i in range(batch):
        pts = syn.make_frame(1, i + seed)["points"][:, :4]
        out.append(pts[rng.choice(pts.shape[0], n, replace=pts.shape[0] < n)])
    return np.ascontiguousarray(np.stack(out).astype(np.float32))


def _pair(name, seed):
    from pcdet_amd.ops.pointnet2.pointnet2_batch import pointnet2_modules as pm
    torch.manual_seed(seed)
    m = pm.VoxelPointnetSAModuleFSMSGDistillation(**sa_configs.INSTANCES[name]())
    for p in m.parameters():                                        # non-trivial BN affine parameters
        if p.dim() == 1:
            p.data.uniform_(0.5, 1.5)
    r = pm.VoxelPointnetSAModuleFSMSGDistillation(**sa_configs.INSTANCES[name]())
    r.load_state_dict(m.state_dict())
    return m.to(DEV), r.to(DEV)


def _clone_sp(sp):
    import spx
    return spx.SparseConvTensor(sp.features.detach().clone(), sp.indices.clone(), sp.spatial_shape, sp.batch_size)


def _loss(out):
    new_xyz, feats, scores, sp = out[:4]
    w = torch.linspace(-1, 1, feats.numel(), device=DEV).view_as(feats)
    loss = (feats * w).sum() + sp.features.square().mean()
    if scores is not None:
        loss = loss + scores.sum()
    return loss


def _compare(m, r, out, ref):
    assert torch.equal(out[0], ref[0])                              # new_xyz (the sampled points)
    assert torch.equal(out[5], ref[5])                              # centroid voxel indices
    if ref[6] is not None:
        assert torch.equal(out[6], ref[6])                          # unique_idxs
    assert _rel(out[1], ref[1]) <= 1e-4
    assert _rel(out[3].features, ref[3].features) <= 1e-4
    assert torch.equal(out[3].indices, ref[3].indices)
    if ref[2] is not None:
        assert _rel(out[2], ref[2]) <= 1e-4
    if torch.is_grad_enabled() and m.training:
        _loss(out).backward()
        _loss(ref).backward()
        for (n, p), (_, q) in zip(m.named_parameters(), r.named_parameters()):
            if q.grad is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
                continue
            assert _rel(p.grad, q.grad) <= 2e-3, n


@pytest.fixture(scope="module")
def layer0_out():
    """Layer-0 inputs and (teacher, no-grad) outputs: what layer 1 consumes."""
    pts = _g(_frames(2, 16384, seed=11))
    xyz, feats = pts[..., :3].contiguous(), pts[..., 3:].permute(0, 2, 1).contiguous()
    m, _ = _pair("backbone_sa0", 0)
    m.train()
    with torch.no_grad():
        out = m(xyz, feats)
    return xyz, feats, out


@pytest.mark.parametrize("train", [True, False])
def test_layer0_point_branch_matches_unfused_reference(train, layer0_out):
    from sa_module_ref import reference_forward
    xyz, feats, _ = layer0_out
    m, r = _pair("backbone_sa0", 1)
    m.train(train)
    r.train(train)
    out = m(xyz, feats)
    ref = reference_forward(r, xyz, feats)
    _compare(m, r, out, ref)


@pytest.mark.parametrize("train", [True, False])
def test_layer1_voxel_branch_matches_unfused_reference(train, layer0_out):
    from sa_module_ref import reference_forward
    _, _, (l_xyz, l_feat, l_scores, l_sp, l_cent, l_cvi, l_uid, _) = layer0_out
    m, r = _pair("backbone_sa1", 2)
    m.train(train)
    r.train(train)
    out = m(l_xyz, l_feat, scores=l_scores, sp_tensor=_clone_sp(l_sp), centroids=l_cent, centroid_voxel_idxs=l_cvi,
            unique_idxs=l_uid)
    ref = reference_forward(r, l_xyz, l_feat, scores=l_scores, sp_tensor=_clone_sp(l_sp), centroids=l_cent,
                            centroid_voxel_idxs=l_cvi, unique_idxs=l_uid)
    assert out[1].shape == (2, 256, 512) and out[2].shape == (l_sp.features.shape[0], 3)
    _compare(m, r, out, ref)


def test_backbone_fast_cpc_kitti_batch2():
    from pcdet_amd.models import backbones_3d
    from sa_module_ref import reference_forward
    cfg = sa_configs.backbone_cfg()
    torch.manual_seed(7)
    net = backbones_3d.get_backbone_3d(cfg.NAME)(model_cfg=cfg, input_channels=4, grid_size=sa_configs.GRID_SIZE,
                                         voxel_size=sa_configs.VOXEL_SIZE,
                                         point_cloud_range=sa_configs.POINT_CLOUD_RANGE).to(DEV)
    net.train()
    pts = _frames(2, 16384, seed=21)
    bidx = np.repeat(np.arange(2, dtype=np.float32), 16384)[:, None]
    points = _g(np.concatenate([bidx, pts.reshape(-1, 4)], axis=1))
    bd = net({"batch_size": 2, "points": points})
    nvox = bd["last_sp_tensor"].features.shape[0]
    assert bd["last_features"].shape == (2, 256, 512) and bd["s_last_features"].shape == (2, 128, 512)
    # the reference views the teacher's (B, N, C) features as (-1, N), the student's as (-1, C); both are kept
    assert bd["point_features"].shape == (2 * 256, 512) and bd["s_point_features"].shape == (1024, 128)
    assert bd["point_coords"].shape == (1024, 4) and bd["s_point_coords"].shape == (1024, 4)
    assert bd["statistic_feature"].shape == (nvox, 256) and bd["s_statistic_feature"].shape == (nvox, 128)
    assert bd["last_scores"].shape == (nvox, 3) and bd["s_last_scores"].shape == (nvox, 3)
    assert bd["last_centroids"].shape == (nvox, 4) and bd["last_centroid_voxel_idxs"].shape == (nvox, 4)
    assert bd["last_unique_idxs"].shape == (1024,) and bd["s_last_unique_idxs"].shape == (1024,)
    assert len(bd["point_coords_list"]) == 3 and len(bd["point_scores_list"]) == 3
    assert bd["point_scores_list"][0].shape[1] == 3 and bd["point_part_scores_list"] == []
    assert not bd["last_features"].requires_grad and bd["s_last_features"].requires_grad

    # the same chain through the unfused transcription, layer by layer, with the backbone's own weights
    xyz = points[:, 1:4].reshape(2, -1, 3).contiguous()
    feats = points[:, 4:].reshape(2, -1, 1).permute(0, 2, 1).contiguous()
    with torch.no_grad():
        t0 = reference_forward(net.SA_modules[0], xyz, feats)
        t1 = reference_forward(net.SA_modules[1], t0[0], t0[1], scores=t0[2], sp_tensor=_clone_sp(t0[3]),
                               centroids=t0[4], centroid_voxel_idxs=t0[5], unique_idxs=t0[6])
    s1 = reference_forward(net.S_SA_modules[0], t0[0], t0[1], scores=t0[2], sp_tensor=_clone_sp(t0[3]),
                           centroids=t0[4], centroid_voxel_idxs=t0[5], unique_idxs=t0[6])
    assert torch.equal(bd["point_coords_list"][0], t0[4])
    assert torch.equal(bd["last_centroid_voxel_idxs"], t0[5])
    assert torch.equal(bd["last_unique_idxs"], t1[6])
    assert _rel(bd["last_features"], t1[1]) <= 1e-4
    assert _rel(bd["statistic_feature"], t1[3].features) <= 1e-4
    assert _rel(bd["s_last_features"], s1[1]) <= 1e-4
    assert _rel(bd["s_statistic_feature"], s1[3].features) <= 1e-4
    assert _rel(bd["s_last_scores"], s1[2]) <= 1e-4


def test_sparse_conv_wider_than_128_channels_trains():
    """The layer-1 U-Net has 256-channel sparse convs; their weight gradient runs as 128-channel tiles of the kernel."""
    import copy

    import spx
    from oracle.cpu_backend import use_oracle_backend
    g = torch.Generator().manual_seed(6)
    shape, batch = [5, 20, 18], 2
    cells = batch * shape[0] * shape[1] * shape[2]
    lin = torch.randperm(cells, generator=g)[:500]
    vol = shape[0] * shape[1] * shape[2]
    idx = torch.stack([lin // vol, (lin % vol) // (shape[1] * shape[2]), (lin // shape[2]) % shape[1], lin % shape[2]],
                      1).int()
    feat = torch.randn(500, 200, generator=g)
    net = spx.SparseSequential(spx.SubMConv3d(200, 256, 3, bias=False, indice_key="a"),
                               spx.SparseConv3d(256, 144, 3, stride=2, padding=1, bias=False, indice_key="d"))
    ref = copy.deepcopy(net)

    def run(m, f, i):
        f = f.clone().requires_grad_(True)
        out = m(spx.SparseConvTensor(f, i, shape, batch))
        (out.features * torch.linspace(-1, 1, out.features.numel(), device=f.device).view_as(out.features)).sum().backward()
        return out

    with use_oracle_backend():
        run(ref, feat, idx)
    net.to(DEV)
    run(net, feat.to(DEV), idx.to(DEV))
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad, q.grad) < 1e-4, n
