"""The fused PillarVFE op on the GPU (csrc/pillar_vfe.hip, include/spx.h §23, spx.ops.pillar_vfe), PointPillarScatter and
the PointPillar detector, against the float64 restatement (tests/pillar_vfe_ref.py, itself pinned to the reference's
recorded values by tests/test_pillar_vfe_ref.py).

Selection: arg and the active mask (out > 0) must equal the float64 ones on every (pillar, channel) pair that is not
ambiguous (pillar_vfe_ref.ambiguous: float64 top-two gap or distance from 0 below 1e-5 max|z|; at most 1 % of the pairs
of a case, asserted on the CPU).  Gradients are compared with the restatement evaluated for the op's OWN selection, and
the eager composition's with the restatement evaluated for the eager selection, so a flipped near-tie does not count as
an arithmetic error of either.

Accuracy rule, per output tensor: e_fused = max |fused - float64| <= point_loss_ref.measured_bound(e_eager, float64),
e_eager being the error of this tree's float32 torch composition on the same device.  Both errors are printed (run with
-s) and appended to profiles/pillar_vfe_accuracy.log."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pillar_vfe_ref as pvr
import point_loss_ref as plr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "pillar_vfe_accuracy.log")
YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/pointpillar.yaml")


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case and its float64 forward in both modes, computed once and shared (never written to)."""
    case = pvr.gpu_case(name)
    return case, pvr.forward(case, training=True), pvr.forward(case, training=False)


def _dev_inputs(case):
    return dict(voxels=_g(case["voxels"]), num=_g(case["num"]), coords=_g(case["coords"]), weight=_g(case["weight"]),
                gamma=_g(case["gamma"]), beta=_g(case["beta"]), d_out=_g(case["d_out"]))


def _fused(case, training, d=None, d_n=None, rows=None):
    """One forward + backward of the raw entry points -> dict of numpy results.  rows: use only the first `rows` pillars."""
    from spx import ops
    d = d or _dev_inputs(case)
    sl = slice(None) if rows is None else slice(0, rows)
    rm, rv = _g(case["running_mean"]), _g(case["running_var"])
    nbt = torch.tensor([int(case["nbt"])], dtype=torch.int64, device=DEV)
    kw = dict(use_absolute_xyz=case["use_abs"], with_distance=case["with_dist"], training=training, d_n=d_n)
    res = ops.pillar_vfe_fwd(d["voxels"][sl], d["num"][sl], d["coords"][sl], d["weight"], d["gamma"], d["beta"], rm, rv, nbt,
                             pvr.MOMENTUM, pvr.EPS, pvr.VOXEL, pvr.offsets(), **kw)
    dw, dg, db = ops.pillar_vfe_bwd(d["d_out"][sl], res["out"], res["arg"], res["stats"], d["voxels"][sl], d["num"][sl],
                                    d["coords"][sl], d["weight"], d["gamma"], rm, rv, pvr.EPS, pvr.VOXEL, pvr.offsets(), **kw)
    torch.cuda.synchronize()
    return dict(out=_n(res["out"]), arg=_n(res["arg"]).astype(np.int64), d_weight=_n(dw), d_gamma=_n(dg), d_beta=_n(db),
                running_mean=_n(rm), running_var=_n(rv), nbt=int(nbt.item()),
                mean=None if res["mean"] is None else _n(res["mean"]),
                invstd=None if res["invstd"] is None else _n(res["invstd"]))


def _vfe(case, fused=None):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.backbones_3d.vfe import PillarVFE
    cfg = AttrDict(NAME="PillarVFE", WITH_DISTANCE=case["with_dist"], USE_ABSLOTE_XYZ=case["use_abs"], USE_NORM=True,
                   NUM_FILTERS=[64])
    if fused is not None:
        cfg["FUSED"] = fused
    lo = [o - v / 2 for o, v in zip(pvr.offsets(), pvr.VOXEL)]
    vfe = PillarVFE(cfg, case["voxels"].shape[2], list(pvr.VOXEL), lo + [lo[0] + 69.12, lo[1] + 79.36, lo[2] + 4.0]).to(DEV)
    pfn = vfe.pfn_layers[0]
    with torch.no_grad():
        pfn.linear.weight.copy_(_g(case["weight"]))
        pfn.norm.weight.copy_(_g(case["gamma"]))
        pfn.norm.bias.copy_(_g(case["beta"]))
        pfn.norm.running_mean.copy_(_g(case["running_mean"]))
        pfn.norm.running_var.copy_(_g(case["running_var"]))
        pfn.norm.num_batches_tracked.fill_(int(case["nbt"]))
    return vfe


def _eager(case, training, d=None):
    """This tree's float32 composition on the device, op by op as PFNLayer.forward runs them, with its own selection."""
    d = d or _dev_inputs(case)
    vfe = _vfe(case, fused=False).train(training)
    pfn = vfe.pfn_layers[0]
    t = case["voxels"].shape[1]
    feats = vfe.point_features(d["voxels"], d["num"], d["coords"])
    x = F.relu(pfn.norm(pfn.linear(feats).permute(0, 2, 1)).permute(0, 2, 1))
    out, idx = torch.max(x, dim=1)
    (out * d["d_out"]).sum().backward()
    torch.cuda.synchronize()
    arg = torch.where(idx >= d["num"].long()[:, None], torch.full_like(idx, t), idx)
    return dict(out=_n(out), arg=_n(arg), active=_n(out > 0), d_weight=_n(pfn.linear.weight.grad),
                d_gamma=_n(pfn.norm.weight.grad), d_beta=_n(pfn.norm.bias.grad), running_mean=_n(pfn.norm.running_mean),
                running_var=_n(pfn.norm.running_var), nbt=int(pfn.norm.num_batches_tracked))


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _report(tag, rows):
    """rows: (tensor name, e_fused, e_eager, float64 values).  Prints, logs, then asserts the rule for every tensor."""
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    lines = []
    for name, e_f, e_e, gold in rows:
        bound = plr.measured_bound(e_e, gold)
        lines.append("%-28s %-14s e_fused %.3e  e_eager %.3e  bound %.3e  max|f64| %.3e" % (tag, name, e_f, e_e, bound,
                                                                                           float(np.abs(gold).max())))
    print("\n" + "\n".join(lines))
    with open(LOG, "a") as f:
        f.write("\n".join(lines) + "\n")
    for name, e_f, e_e, gold in rows:
        assert e_f <= plr.measured_bound(e_e, gold), (tag, name, e_f, e_e)


def _check_selection(case, ref, got):
    t = case["voxels"].shape[1]
    clear = ~pvr.ambiguous(ref)
    assert clear.mean() >= 0.99
    assert np.array_equal(got["arg"][clear], ref["arg"][clear])
    assert np.array_equal((got["out"] > 0)[clear], ref["active"][clear])
    assert got["arg"].max() <= t and (got["arg"][case["num"] >= t] < t).all()
    dup = case["dup"]
    if dup.any():                     # rows 0 and 1 of these pillars are the same point: the lower index wins the tie
        assert not (got["arg"][dup] == 1).any() and (got["arg"][dup] == 0).any()


@pytest.mark.parametrize("name", sorted(pvr.GPU_CASES))
def test_train_forward_and_gradients_against_float64(name):
    case, ref, _ = _case(name)
    d = _dev_inputs(case)
    got, eag = _fused(case, True, d), _eager(case, True, d)
    _check_selection(case, ref, got)
    assert got["nbt"] == ref["nbt"] == eag["nbt"]
    want = dict(zip(("d_weight", "d_gamma", "d_beta"), pvr.backward(case, ref, case["d_out"], got["arg"], got["out"] > 0)))
    want_e = dict(zip(("d_weight", "d_gamma", "d_beta"), pvr.backward(case, ref, case["d_out"], eag["arg"], eag["active"])))
    rows = [(k, _err(got[k], ref[k]), _err(eag[k], ref[k]), ref[k]) for k in ("out", "running_mean", "running_var")]
    rows += [(k, _err(got[k], want[k]), _err(eag[k], want_e[k]), want[k]) for k in ("d_weight", "d_gamma", "d_beta")]
    _report("train/" + name, rows)
    # the saved statistics are float32 roundings (half an ulp, 6e-8 relative) of values taken in double from the features
    # the contract prescribes, whose pillar centre is formed in float32: the restatement with that centre
    ref32 = pvr.forward(case, center_dtype=np.float32)
    assert _err(got["mean"], ref32["mean"]) <= 1e-6 * float(np.abs(ref32["mean"]).max())
    assert _err(got["invstd"], ref32["invstd"]) <= 1e-6 * float(ref32["invstd"].max())


@pytest.mark.parametrize("name", ["m1_t32", "m257_t32", "m1000_t20_dist", "m257_t1_rel", "far"])
def test_eval_forward_and_gradients_against_float64(name):
    case, _, ref = _case(name)
    d = _dev_inputs(case)
    got, eag = _fused(case, False, d), _eager(case, False, d)
    clear = ~pvr.ambiguous(ref)
    assert np.array_equal(got["arg"][clear], ref["arg"][clear]) and np.array_equal((got["out"] > 0)[clear], ref["active"][clear])
    assert got["nbt"] == int(case["nbt"]) and np.array_equal(got["running_mean"], case["running_mean"])
    assert np.array_equal(got["running_var"], case["running_var"]) and got["mean"] is None
    names = ("d_weight", "d_gamma", "d_beta")
    want = dict(zip(names, pvr.backward(case, ref, case["d_out"], got["arg"], got["out"] > 0, training=False)))
    want_e = dict(zip(names, pvr.backward(case, ref, case["d_out"], eag["arg"], eag["active"], training=False)))
    rows = [("out", _err(got["out"], ref["out"]), _err(eag["out"], ref["out"]), ref["out"])]
    rows += [(k, _err(got[k], want[k]), _err(eag[k], want_e[k]), want[k]) for k in names]
    _report("eval/" + name, rows)


def test_two_runs_are_bitwise_equal():
    case, _, _ = _case("m1000_t20_dist")
    d = _dev_inputs(case)
    a, b = _fused(case, True, d), _fused(case, True, d)
    for k in ("out", "arg", "d_weight", "d_gamma", "d_beta", "running_mean", "running_var", "mean", "invstd"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("training", [True, False])
def test_dead_rows_are_never_read_and_come_back_zero(training):
    case, _, _ = _case("m257_t32")
    live = 100
    exact = _fused(case, training, rows=live)
    d = _dev_inputs(case)
    d["voxels"][live:] = float("nan")
    d["num"][live:] = 1 << 30
    d["coords"][live:] = -(1 << 30)
    d["d_out"][live:] = float("nan")
    d_n = torch.tensor([live], dtype=torch.int64, device=DEV)
    got = _fused(case, training, d, d_n=d_n)
    assert np.array_equal(got["out"][:live], exact["out"]) and np.array_equal(got["arg"][:live], exact["arg"])
    assert not got["out"][live:].any() and not got["arg"][live:].any()
    for k in ("d_weight", "d_gamma", "d_beta", "running_mean", "running_var"):
        assert np.array_equal(got[k], exact[k]), k
    assert got["nbt"] == exact["nbt"]
    # the module's d_n may also be an int32 scalar tensor; a live count above the capacity is clamped to it
    d2 = _dev_inputs(case)
    full = _fused(case, training, d2)
    over = _fused(case, training, d2, d_n=torch.tensor([1 << 40], dtype=torch.int64, device=DEV))
    assert np.array_equal(full["out"], over["out"]) and np.array_equal(full["d_weight"], over["d_weight"])


def test_zero_points_row_is_all_padding_and_counts_clamp():
    """The one deliberate deviation: a live row with num_points == 0 is all padding (no NaN); num_points > T is T."""
    from spx import ops
    case, _, _ = _case("m257_t32")
    t = case["voxels"].shape[1]
    d = _dev_inputs(case)
    d["num"][0] = 0
    d["num"][1] = t + 9                    # row 1 is the full pillar of the case
    got = _fused(case, True, d)
    assert np.isfinite(got["out"]).all() and np.isfinite(got["d_weight"]).all()
    assert (got["arg"][0] == t).all()
    twin = dict(case, num=case["num"].copy())
    twin["num"][0] = 0
    ref = pvr.forward(twin)
    assert _err(got["out"], ref["out"]) <= 1e-5 * float(np.abs(ref["out"]).max())
    with pytest.raises(ops._lib.SpxError, match="requires_grad"):
        ops.pillar_vfe(d["voxels"].clone().requires_grad_(True), d["num"], d["coords"], d["weight"], d["gamma"], d["beta"],
                       None, None, None, pvr.MOMENTUM, pvr.EPS, pvr.VOXEL, pvr.offsets(), training=True)
    with pytest.raises(ops._lib.SpxError, match="C_out = 32"):
        ops.pillar_vfe_fwd(d["voxels"], d["num"], d["coords"], d["weight"][:32], d["gamma"][:32], d["beta"][:32], None, None,
                           None, pvr.MOMENTUM, pvr.EPS, pvr.VOXEL, pvr.offsets(), training=True)


def test_forward_and_backward_capture_in_a_graph():
    """Forward + backward under torch.cuda.graph (a host read fails the capture) with the live count on the device: two
    replays with different counts each equal their eager call bit for bit."""
    from spx import ops
    case, _, _ = _case("m257_t32")
    d = _dev_inputs(case)
    d_n = torch.tensor([257], dtype=torch.int64, device=DEV)
    rm0, rv0 = _g(case["running_mean"]), _g(case["running_var"])
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(use_absolute_xyz=case["use_abs"], with_distance=case["with_dist"], training=True, d_n=d_n)

    def step():
        res = ops.pillar_vfe_fwd(d["voxels"], d["num"], d["coords"], d["weight"], d["gamma"], d["beta"], rm, rv, nbt,
                                 pvr.MOMENTUM, pvr.EPS, pvr.VOXEL, pvr.offsets(), **kw)
        grads = ops.pillar_vfe_bwd(d["d_out"], res["out"], res["arg"], res["stats"], d["voxels"], d["num"], d["coords"],
                                   d["weight"], d["gamma"], rm, rv, pvr.EPS, pvr.VOXEL, pvr.offsets(), **kw)
        return (res["out"], res["arg"], res["mean"], res["invstd"]) + tuple(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # warm-up: the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for live in (257, 61):
        d_n.fill_(live)
        rm.copy_(rm0), rv.copy_(rv0)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured] + [rm.clone(), rv.clone()]
        rm.copy_(rm0), rv.copy_(rv0)
        eager = list(step()) + [rm, rv]
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(replayed, eager)):
            assert torch.equal(a, b), (live, i)
        assert not replayed[0][live:].any() and replayed[0][:live].any()


def test_module_fused_path_matches_its_composition_and_the_autograd_wrapper():
    """PillarVFE.forward takes the fused op by default; its outputs and parameter gradients obey the rule as well."""
    case, ref, _ = _case("m257_t32")
    d = _dev_inputs(case)
    batch = dict(voxels=d["voxels"], voxel_num_points=d["num"], voxel_coords=d["coords"], batch_size=2)
    vfe = _vfe(case).train()
    assert vfe.fused_refusal(d["voxels"]) is None
    out = vfe(dict(batch))["pillar_features"]
    assert out.shape == (257, 64) and out.grad_fn is not None and "PillarVFE" in type(out.grad_fn).__name__
    (out * d["d_out"]).sum().backward()
    pfn = vfe.pfn_layers[0]
    raw = _fused(case, True, d)
    assert np.array_equal(_n(out), raw["out"]) and np.array_equal(_n(pfn.linear.weight.grad), raw["d_weight"])
    assert np.array_equal(_n(pfn.norm.weight.grad), raw["d_gamma"]) and np.array_equal(_n(pfn.norm.bias.grad), raw["d_beta"])
    assert np.array_equal(_n(pfn.norm.running_mean), raw["running_mean"]) and int(pfn.norm.num_batches_tracked) == ref["nbt"]
    one = vfe.eval()(dict(voxels=d["voxels"][:1], voxel_num_points=d["num"][:1], voxel_coords=d["coords"][:1], batch_size=1))
    assert one["pillar_features"].shape == (1, 64)


# ------------------------------------------------------------------------------------------------ PointPillarScatter
def _scatter_inputs():
    rng = np.random.default_rng(3)
    nx, ny, b, m = 16, 12, 2, 150
    cells = rng.choice(nx * ny * b, size=m, replace=False)
    coords = np.stack([cells % b, np.zeros(m, np.int64), (cells // b) % ny, (cells // b) // ny], 1).astype(np.int32)
    return nx, ny, b, coords, rng.normal(0, 1, (m, 64)).astype(np.float32)


def test_scatter_equals_the_reference_scatter_and_its_gradient_is_the_gather():
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.backbones_2d.map_to_bev import PointPillarScatter
    nx, ny, b, coords, feats = _scatter_inputs()
    for channels_last in (True, False):
        scat = PointPillarScatter(AttrDict(NUM_BEV_FEATURES=64, CHANNELS_LAST=channels_last), (nx, ny, 1))
        f = _g(feats).requires_grad_(True)
        bev = scat(dict(pillar_features=f, voxel_coords=_g(coords), batch_size=b))["spatial_features"]
        assert bev.shape == (b, 64, ny, nx) and hasattr(bev, "_spx_source")
        assert bev.is_contiguous(memory_format=torch.channels_last) == channels_last
        assert np.array_equal(_n(bev), pvr.scatter(feats, coords, b, nx, ny))
        gy = torch.randn(bev.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
        (bev * gy).sum().backward()
        want = _n(gy)[coords[:, 0], :, coords[:, 2], coords[:, 3]]
        assert np.array_equal(_n(f.grad), want)


def test_bev_backbone_on_the_tagged_map_equals_the_untagged_copy():
    """BaseBEVBackbone runs its first convolution over the live pillars when the map carries the tag: the same values as
    the dense route on a copy, to the 1e-5 relative of test_gpu_model.test_bev_sparse_entry_matches_dense_conv."""
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.backbones_2d import base_bev_backbone as bb
    from pcdet_amd.models.backbones_2d.map_to_bev import PointPillarScatter
    nx, ny, b, coords, feats = _scatter_inputs()
    torch.manual_seed(2)
    net = bb.BaseBEVBackbone(AttrDict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[2, 2], NUM_FILTERS=[64, 128], UPSAMPLE_STRIDES=[1, 2],
                                      NUM_UPSAMPLE_FILTERS=[32, 32]), 64).to(DEV).to(memory_format=torch.channels_last).train()
    scat = PointPillarScatter(AttrDict(NUM_BEV_FEATURES=64), (nx, ny, 1))
    seen = []
    entry = bb._sparse_entry
    bb._sparse_entry = lambda seq, bev: seen.append(entry(seq, bev)) or seen[-1]

    def run(tagged):
        net.zero_grad()
        f = _g(feats).requires_grad_(True)
        bev = scat(dict(pillar_features=f, voxel_coords=_g(coords), batch_size=b))["spatial_features"]
        y = net(dict(spatial_features=bev if tagged else bev.clone()))["spatial_features_2d"]
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).to(DEV)
        (y * gy).sum().backward()
        return y.detach(), f.grad.clone(), net.blocks[0][1].weight.grad.clone()

    try:
        ys, gfs, gws = run(True)
        yd, gfd, gwd = run(False)
    finally:
        bb._sparse_entry = entry
    assert seen[0] is not None and seen[1] is None              # the tagged map took the sparse entry, the copy did not

    def rel(a, c):
        return float((a.double() - c.double()).abs().max() / c.double().abs().max().clamp_min(1e-12))

    assert rel(ys, yd) < 1e-5 and rel(gfs, gfd) < 1e-5 and rel(gws, gwd) < 1e-5


# ----------------------------------------------------------------------------------------------------- the detector
@functools.lru_cache(maxsize=None)
def _pointpillar():
    """PointPillar on a 64 x 64 pillar grid, two synthetic frames voxelised once; the fused and the composition model
    share every parameter value."""
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    from spx import ops
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    cfg.DATA_CONFIG.POINT_CLOUD_RANGE = [0, -5.12, -3, 10.24, 5.12, 1]
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=0)
    assert list(ds.grid_size) == [64, 64, 1]
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, ds).to(DEV)
    cfg.MODEL.VFE.FUSED = False
    plain = build_network(cfg.MODEL, 3, ds).to(DEV)
    plain.load_state_dict(model.state_dict())
    batch = ds.collate_batch([ds[0], ds[1]])
    batch = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    vox = ops.voxelize(batch["points"], ds.point_cloud_range.tolist(), ds.voxel_size, 32, 16000, batch_size=2, batch_col=0,
                       xyz_col=1, feat_col=1, num_features=4, want_mean=False)
    voxels = dict(voxels=vox["voxels"], voxel_num_points=vox["num_points"], voxel_coords=vox["coords"])
    return cfg, ds, model, plain, batch, voxels


def test_pointpillar_train_step():
    _cfg, _ds, model, _plain, batch, _vox = _pointpillar()
    model.train()
    model.zero_grad(set_to_none=True)
    ret, tb_dict, _disp = model(dict(batch))                     # from points: the VFE voxelises
    loss = ret["loss"]
    assert loss.dim() == 0 and torch.isfinite(loss)
    assert "loss_rpn" in tb_dict and all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in tb_dict.values())
    loss.backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert model.vfe.pfn_layers[0].linear.weight.grad.abs().sum() > 0


def test_vfe_static_mode_keeps_capacity_rows_and_passes_the_live_count():
    """`static_caps` in the batch dict: the voxeliser runs without a host read, rows stay at capacity, the live count
    travels as a device tensor to the op and to the scatter; live rows and the BEV map equal the exact-size path."""
    _cfg, _ds, model, _plain, batch, _vox = _pointpillar()
    vfe, scat = model.vfe.eval(), model.map_to_bev_module
    with torch.no_grad():
        exact = scat(vfe(dict(batch)))
        static = scat(vfe(dict(batch, static_caps={})))
    n = exact["pillar_features"].shape[0]
    d_n = static["voxel_num_valid"]
    assert d_n.dtype == torch.int64 and d_n.is_cuda and int(d_n) == n and static["pillar_features"].shape[0] > n
    assert torch.equal(static["pillar_features"][:n], exact["pillar_features"])
    assert not static["pillar_features"][n:].any()
    assert torch.equal(static["spatial_features"], exact["spatial_features"])


def test_pointpillar_fused_loss_matches_the_composition():
    """The accuracy rule on the loss: L(x) is the loss of the rest of the network on pillar features x; the float64
    value is L(float64 restatement of the VFE), e_fused = |L(fused) - it|, e_eager = |L(composition) - it|."""
    _cfg, _ds, model, plain, batch, vox = _pointpillar()
    pfn = plain.vfe.pfn_layers[0]
    case = dict(voxels=_n(vox["voxels"]), num=_n(vox["voxel_num_points"]), coords=_n(vox["voxel_coords"]),
                use_abs=True, with_dist=False, weight=_n(pfn.linear.weight), gamma=_n(pfn.norm.weight),
                beta=_n(pfn.norm.bias), running_mean=_n(pfn.norm.running_mean), running_var=_n(pfn.norm.running_var),
                nbt=0, offs=(plain.vfe.x_offset, plain.vfe.y_offset, plain.vfe.z_offset))
    gold = _g(pvr.forward(case)["out"].astype(np.float32))

    def loss_of(net, features=None):
        net.train()
        first = net.module_list[0]
        if features is not None:
            net.module_list[0] = lambda bd: dict(bd, pillar_features=features)
        try:
            with torch.no_grad():
                return float(net(dict(batch, **vox))[0]["loss"])
        finally:
            net.module_list[0] = first

    l_gold, l_fused, l_eager = loss_of(plain, gold), loss_of(model), loss_of(plain)
    _report("detector", [("loss", abs(l_fused - l_gold), abs(l_eager - l_gold), np.array([l_gold]))])


def test_pointpillar_eval_and_state_dict():
    _cfg, _ds, model, _plain, batch, _vox = _pointpillar()
    model.eval()
    with torch.no_grad():
        model.dense_head.conv_cls.bias.add_(4.0)                 # lift the prior over the 0.1 score threshold
        pred_dicts, recall_dict = model(dict(batch))
        model.dense_head.conv_cls.bias.sub_(4.0)
    assert len(pred_dicts) == 2
    for p in pred_dicts:
        assert set(p) == {"pred_boxes", "pred_scores", "pred_labels"}
        n = p["pred_boxes"].shape[0]
        assert n > 0 and p["pred_boxes"].shape == (n, 7) and p["pred_scores"].shape == p["pred_labels"].shape == (n,)
    assert "gt" in recall_dict
    with open(os.path.join(ROOT, "tests", "golden", "pillar_vfe_state_keys.json")) as f:
        keys = json.load(f)["one_layer"]
    state = {"vfe." + k: torch.full(shape, 0.5) for k, shape in keys}
    twin = copy.deepcopy(model)                                  # the cached model keeps its parameters
    result = twin.load_state_dict(state, strict=False)
    assert not result.unexpected_keys and not [k for k in result.missing_keys if k.startswith("vfe.")]
    assert float(twin.vfe.pfn_layers[0].linear.weight.detach().min()) == 0.5
