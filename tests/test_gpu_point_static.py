"""The host-sync-free (static-capacity) path of the fast_cpc point detector on the GPU.

Ops (csrc/voxel_rows.hip, include/spx.h §19) against the numpy restatement (tests/voxel_rows_ref.py), exactly, and the
means bit-equal to the eager composition they replace.  The SA layers, chained by hand in static mode, against the eager
modules fed the previous static stage's outputs trimmed to the live rows: sampled points, voxel indices, unique_idxs and
the live count exact, features / sparse features / scores on live rows ||err|| / ||ref|| <= 1e-4 (the tolerance
tests/test_gpu_sa_module.py holds these modules to: the sparse convolutions may pick another kernel for a capacity-sized
launch).  The backbone's wiring, the flags, and the graphed runner, bit-equal to the eager static run."""
import numpy as np
import pytest
import torch

import point_head_configs as phc
import sa_configs
import voxel_rows_ref as vr
from test_point_head_cpu import randomize

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _d_n(n):
    return None if n is None else torch.tensor([n], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------ the ops
def _eager_rows(idx, xyz, feats, n_live):
    """The composition that exists today (_unet_update's chain) on the live rows; points outside the grid are taken out
    first (the eager chain has no range check and would index past the table)."""
    import spx
    from pcdet_amd.utils import voxel_aggregation_utils as va
    n_live = vr.CAP if n_live is None else n_live
    sp = spx.SparseConvTensor(torch.zeros((n_live, vr.C), device=DEV), _g(idx[:n_live]), vr.SHAPE, vr.B)
    _, inside = vr.point_cells(xyz, vr.SHAPE, vr.LO, vr.VS)
    new_xyz = _g(xyz).view(-1, 3)
    keep = _g(inside.reshape(-1))
    vs, lo = torch.tensor(vr.VS, device=DEV).float(), torch.tensor(vr.LO, device=DEV).float()
    pidx = va.get_voxel_indices(new_xyz, voxel_size=vs, point_cloud_range=lo)
    bidx = torch.arange(vr.B, device=DEV).view(-1, 1).expand(vr.B, vr.M).reshape(-1, 1).long()
    vidx = torch.cat((bidx, pidx), dim=-1)[:, [0, 3, 2, 1]]
    pts = torch.cat([bidx.float(), new_xyz, _g(feats).permute(0, 2, 1).reshape(-1, vr.C)], dim=-1)
    cent, cvi, _, _ = va.get_centroid_per_voxel(pts[keep], vidx[keep])
    rows, hit = va.get_nonempty_voxel_feature_indices(cvi, sp)
    src = cent.new_zeros([n_live, vr.C])
    src[rows] = cent[:, 4:][hit]
    return src


@pytest.mark.parametrize("n_live", [0, vr.CAP, 25, 7, None])
def test_ops_match_restatement_and_eager_composition(n_live):
    from spx import ops
    idx, xyz, feats, _ = vr.make_case(n_live, seed=3)
    want_table, status = vr.table_build(idx, n_live, vr.B, vr.SHAPE)
    assert status == 0
    table = ops.voxel_table_build(_g(idx), vr.B, vr.SHAPE, d_n=_d_n(n_live))
    assert table.dtype == torch.int32 and np.array_equal(table.cpu().numpy(), want_table)     # dead rows left no mark
    sentinel = torch.full((vr.CAP, vr.C), 777.0, device=DEV)
    out = ops.voxel_rows_mean(_g(xyz), _g(feats), table, vr.LO, vr.VS, vr.CAP, d_n_rows=_d_n(n_live), out=sentinel.clone())
    want = vr.rows_mean(xyz, feats, want_table, vr.LO, vr.VS, vr.CAP, n_live, out=sentinel.cpu().numpy())
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))        # means, zero rows and untouched rows: bits
    live = vr.CAP if n_live is None else n_live
    assert (got[live:] == 777.0).all()
    again = ops.voxel_rows_mean(_g(xyz), _g(feats), table, vr.LO, vr.VS, vr.CAP, d_n_rows=_d_n(n_live), out=sentinel.clone())
    assert torch.equal(again, out)
    eager = _eager_rows(idx, xyz, feats, n_live)
    assert torch.equal(out[:live], eager)
    ops.check_status(DEV)


def test_live_row_outside_the_grid_sets_the_status_word_and_writes_nothing():
    from spx import _lib, ops
    idx, _, _, _ = vr.make_case(vr.CAP, seed=4)
    ops.check_status(DEV)
    bad = idx.copy()
    bad[3, 2] = vr.SHAPE[1]
    bad[9, 0] = vr.B
    want, status = vr.table_build(bad, 20, vr.B, vr.SHAPE)
    assert status == vr.OUT_OF_GRID
    assert np.array_equal(ops.voxel_table_build(_g(bad), vr.B, vr.SHAPE, d_n=_d_n(20)).cpu().numpy(), want)
    with pytest.raises(_lib.SpxError, match="outside the table"):
        ops.check_status(DEV)
    ops.check_status(DEV)                                                   # reading resets the sticky word
    ops.voxel_table_build(_g(bad), vr.B, vr.SHAPE, d_n=_d_n(3))              # the bad rows are dead: never read
    ops.check_status(DEV)


# ------------------------------------------------------------------------------------------------------ the layers
def _frames(batch, n, seed=0):
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    out = []
    for i in range(batch):
        pts = syn.make_frame(1, i + seed)["points"][:, :4]
        out.append(pts[rng.choice(pts.shape[0], n, replace=pts.shape[0] < n)])
    return np.ascontiguousarray(np.stack(out).astype(np.float32))


def _squeeze(frame, factor=0.04):
    """The frame pulled towards a point inside the range: a few metres across, many samples per voxel."""
    out = frame.copy()
    centre = np.array([20.0, 3.0, -1.0], dtype=np.float32)
    out[:, :3] = centre + (out[:, :3] - centre) * np.float32(factor)
    return out


def _module(cfg, seed):
    from pcdet_amd.ops.pointnet2.pointnet2_batch import pointnet2_modules as pm
    torch.manual_seed(seed)
    m = pm.VoxelPointnetSAModuleFSMSGDistillation(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.weight.uniform_(0.5, 1.5, generator=g)
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    return m.to(DEV).eval()


def _layers(cut):
    c0, c1, ch = sa_configs.layer0(), sa_configs.student_layer1(), sa_configs.head_vsa()
    if cut:                                               # 2 048 -> 256 -> 64 points
        c0.update(npoint_list=[256], sample_range_list=[[0, 2048]])
        c1.update(npoint_list=[64], sample_range_list=[[0, 256]])
    for m in ch["mlps"]:                                  # the head's S_VSA_module reads the student's 128 channels
        m[0] = 128
    return _module(c0, 1), _module(c1, 2), _module(ch, 3)


def _trim(sp, n):
    import spx
    return spx.SparseConvTensor(sp.features[:n].clone(), sp.indices[:n].clone(), sp.spatial_shape, sp.batch_size)


def _votes(new_xyz):
    shift = torch.linspace(-1.0, 1.0, new_xyz.numel(), device=DEV).view_as(new_xyz)
    return (new_xyz + shift).contiguous()


def _static_chain(mods, pts):
    m0, m1, mh = mods
    xyz, feats = pts[..., :3].contiguous(), pts[..., 3:].permute(0, 2, 1).contiguous()
    s0 = m0(xyz, feats, static=True)
    s1 = m1(s0[0], s0[1], scores=s0[2], sp_tensor=s0[3], centroids=s0[4], centroid_voxel_idxs=s0[5], unique_idxs=s0[6])
    s2 = mh(xyz=s1[0], new_xyz=_votes(s1[0][:, :s1[0].shape[1] // 2]), features=s1[1], sp_tensor=s1[3], centroids=s1[4],
            centroid_voxel_idxs=s1[5])
    return (xyz, feats), s0, s1, s2


def _check_stage(static, eager, n, cap):
    assert torch.equal(static[0], eager[0])                                       # sampled points
    assert static[5].shape[0] == cap and eager[5].shape[0] == n                   # capacity vs live count
    assert torch.equal(static[5][:n], eager[5])                                   # voxel indices
    assert torch.equal(static[3].indices[:n], eager[3].indices)
    if eager[6] is not None:
        assert torch.equal(static[6], eager[6])                                   # unique_idxs
    assert _rel(static[1], eager[1]) <= 1e-4
    assert _rel(static[3].features[:n], eager[3].features) <= 1e-4
    if eager[2] is not None:
        assert _rel(static[2][:n], eager[2]) <= 1e-4
    if eager[4] is not None:
        assert torch.equal(static[4][:n], eager[4])                               # centroids


def _check_chain(mods, pts, expect_fewer_than=None):
    m0, m1, mh = mods
    (xyz, feats), s0, s1, s2 = _static_chain(mods, pts)
    cap = s0[5].shape[0]
    n = int(s0[3].n_valid)
    assert cap == xyz.shape[0] * s0[0].shape[1] and 0 < n <= cap
    assert int(s1[3].n_valid) == n and s1[3].n_valid is s0[3].n_valid
    if expect_fewer_than is not None:
        assert n < expect_fewer_than
    _check_stage(s0, m0(xyz, feats), n, cap)
    e1 = m1(s0[0], s0[1], scores=s0[2][:n], sp_tensor=_trim(s0[3], n), centroids=s0[4][:n],
            centroid_voxel_idxs=s0[5][:n], unique_idxs=s0[6])
    _check_stage(s1, e1, n, cap)
    e2 = mh(xyz=s1[0], new_xyz=s2[0], features=s1[1], sp_tensor=_trim(s1[3], n), centroids=s1[4][:n],
            centroid_voxel_idxs=s1[5][:n])
    assert torch.equal(s2[0], e2[0]) and _rel(s2[1], e2[1]) <= 1e-4
    return n


@pytest.mark.parametrize("size", ["cut", "full"])
def test_static_layers_match_eager_on_identical_inputs(size):
    cut = size == "cut"
    n_pts = 2048 if cut else 16384
    mods = _layers(cut)
    a = _frames(2, n_pts, seed=31)
    first = a.copy()
    first[0] = _squeeze(a[0])                              # frame 0 squeezed, frame 1 ordinary
    second = np.stack([_squeeze(a[0], 0.01), _squeeze(a[1], 0.02)])
    with torch.no_grad():
        n_first = _check_chain(mods, _g(first))
        assert n_first < 2 * mods[0].npoint_list[0]        # the squeezed frame shares voxels: live count below capacity
        # again on fewer live voxels: the allocator hands the same blocks back, so the dead rows hold the first
        # run's rows, stale and plausible
        _check_chain(mods, _g(second), expect_fewer_than=n_first)


# ------------------------------------------------------------------------------------------------------ the detector
def _net(seed=0):
    from pcdet_amd.models.detectors import build_detector
    torch.manual_seed(seed)
    cfg = phc.model_cfg()
    cfg.POST_PROCESSING["SCORE_THRESH"] = [0.005, 0.005, 0.005]     # random-init logits sit near -4.6: let boxes through
    net = build_detector(cfg, 3, phc.dataset())
    randomize(net.point_head, seed + 100)
    g = torch.Generator().manual_seed(seed + 200)
    with torch.no_grad():
        for m in net.backbone_3d.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return net.to(DEV).eval()


def _points(batch, n, seed):
    pts = _frames(batch, n, seed)
    bidx = np.repeat(np.arange(batch, dtype=np.float32), n)[:, None]
    return _g(np.concatenate([bidx, pts.reshape(-1, 4)], axis=1))


STATIC_KEYS = ("sel", "count", "pred_boxes", "pred_scores", "pred_labels", "layout_ok")


def _static_run(net, points):
    """backbone -> head -> post_processing_static on a static_caps batch, eagerly."""
    bd = {"batch_size": 2, "points": points, "static_caps": {}}
    with torch.no_grad():
        for m in net.module_list:
            bd = m(bd)
        st = net.post_processing_static(bd)
    return bd, st


@pytest.fixture(scope="module")
def net():
    """The detector after one static pass at the tests' shape: the dense library picks its kernels on the first call at
    a shape (the runners warm up for the same reason), and bit-equality is asserted between later calls."""
    net = _net(seed=5)
    _static_run(net, _points(2, 16384, seed=50))
    return net


def test_backbone_static_wiring_flags_and_out_of_range_point(net):
    points = _points(2, 16384, seed=51)
    bd, st = _static_run(net, points)
    # the same chain by hand: layer 0 in static mode, the student layer on its outputs
    bb = net.backbone_3d
    xyz = points[:, 1:4].reshape(2, -1, 3).contiguous()
    feats = points[:, 4:].reshape(2, -1, 1).permute(0, 2, 1).contiguous()
    with torch.no_grad():
        t0 = bb.SA_modules[0](xyz, feats, static=True)
        s1 = bb.S_SA_modules[0](t0[0], t0[1], scores=t0[2], sp_tensor=t0[3], centroids=t0[4], centroid_voxel_idxs=t0[5],
                                unique_idxs=t0[6])
    n = int(bd["voxel_num_valid"])
    assert 0 < n == int(s1[3].n_valid) < 2 * 4096
    assert torch.equal(bd["s_last_features"], s1[1]) and torch.equal(bd["s_last_unique_idxs"], s1[6])
    assert torch.equal(bd["s_last_centroids"][:n], s1[4][:n])
    assert torch.equal(bd["s_last_centroid_voxel_idxs"][:n], s1[5][:n])
    assert torch.equal(bd["s_statistic_feature"][:n], s1[3].features[:n])
    # s_last_scores (the student's confidence_mlp, a Conv1d over the capacity rows; no later stage reads it in eval):
    # measured on an MI355X, two static runs on the same input agree to ||err|| / ||ref|| <= 1e-4 but NOT bit for bit,
    # although the live rows of its input (s_statistic_feature, above) are bit-equal; the dead rows hold other garbage.
    # The cause was not found, so this one tensor is held to the module tolerance and the finding is recorded here.
    assert _rel(bd["s_last_scores"][:n], s1[2][:n]) <= 1e-4
    # ... and the end of the chain, head and post-processing on the hand-chained backbone outputs, bit for bit
    hand = {"batch_size": 2, "s_point_coords": bd["s_point_coords"], "s_point_features": bd["s_point_features"],
            "s_last_features": s1[1], "s_last_sp_tensor": s1[3], "s_last_centroids": s1[4],
            "s_last_centroid_voxel_idxs": s1[5]}
    with torch.no_grad():
        st_hand = net.post_processing_static(net.point_head(hand))
    for k in STATIC_KEYS:
        assert torch.equal(st[k], st_hand[k]), k
    assert bd["s_statistic_feature"].shape[0] == 2 * 4096                           # capacity rows
    flags = bd["static_flags"]
    assert sorted(flags) == ["in_range", "layout_ok"] and all(bool(v) for v in flags.values())
    assert bool(st["layout_ok"]) and int(st["count"].sum()) > 0
    # one sampled point outside the range (row 0 is FPS's first pick): reported, nothing raised
    moved = points.clone()
    moved[0, 1] = -50.0
    bd2, _ = _static_run(net, moved)
    torch.cuda.synchronize()
    assert not bool(bd2["static_flags"]["in_range"]) and bool(bd2["static_flags"]["layout_ok"])
    swapped = points.clone()
    swapped[5, 0] = 1.0
    bd3, _ = _static_run(net, swapped)
    assert not bool(bd3["static_flags"]["layout_ok"])


def test_graphed_point_detector_replays_bit_equal_to_the_eager_static_run(net):
    from pcdet_amd.models.inference import GraphedPointDetector
    a, b = _points(2, 16384, seed=61), _points(2, 16384, seed=71)
    want = {}
    for name, pts in (("a", a), ("b", b)):
        bd, st = _static_run(net, pts)
        want[name] = ({k: st[k].clone() for k in STATIC_KEYS}, bd["voxel_num_valid"].clone())
    assert not torch.equal(want["a"][0]["pred_boxes"], want["b"][0]["pred_boxes"])
    runner = GraphedPointDetector(net, 2, 16384)          # building it is the proof that no host read is left
    for name, pts in (("a", a), ("b", b), ("a", a)):
        out = runner(pts)
        torch.cuda.synchronize()
        st, n = want[name]
        for k in STATIC_KEYS:
            assert torch.equal(out[k], st[k]), (name, k)
        assert torch.equal(out["voxel_num_valid"], n)
        assert all(bool(v) for v in out["static_flags"].values())
    # pred_dicts against the eager, per-frame post_processing on the same predictions
    preds = runner.pred_dicts()
    assert sum(p["pred_boxes"].shape[0] for p in preds) > 0
    net.model_cfg.POST_PROCESSING["FUSED"] = False
    try:
        with torch.no_grad():
            ref, _ = net.post_processing({k: out[k] for k in ("batch_size", "batch_index", "batch_cls_preds",
                                                              "batch_box_preds", "cls_preds_normalized")})
    finally:
        net.model_cfg.POST_PROCESSING.pop("FUSED")
    for p, r in zip(preds, ref):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(p[k], r[k]), k
    with pytest.raises(ValueError, match="exactly 16384 points"):
        runner(a[:-1])
    moved = a.clone()
    moved[0, 1] = -50.0
    runner(moved)
    with pytest.raises(RuntimeError, match="in_range"):
        runner.pred_dicts()
