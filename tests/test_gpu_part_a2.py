"""The fused sparse RoI-aware pooling (csrc/roiaware_sparse.hip, include/spx.h §30) against its float32 numpy restatement
(tests/roiaware_sparse_ref.py), bit for bit: coords, cnt, arg, row_of_cell, n_rows, faked, the part and rpn rows and both
gradients; integer-valued features; determinism; static capacity (dead rows, overflow -> the status word); graph capture
and replay on a second scene; and the ragged points-in-boxes."""
import numpy as np
import pytest
import torch

import roiaware_sparse_ref as sref
from part_a2_scenes import grid_scene as _grid_scene, scene as _scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = np.float32


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)


def _run(scene, out_size, max_pts, rows=None, frame_cnt=True, grads=None, max_frame_points=None):
    """collect -> (one host read of n_rows unless `rows`) -> pool [-> backward] through spx.ops, as numpy."""
    from spx import ops
    rois, pts, cnt, part, rpn = scene
    tp, tr = _g(part).requires_grad_(grads is not None), _g(rpn).requires_grad_(grads is not None)
    st = ops.roiaware_sparse_collect(_g(rois), _g(pts), tp, tr, out_size, max_pts,
                                     frame_cnt=_g(cnt) if frame_cnt else None, max_frame_points=max_frame_points)
    n_rows = int(st.n_rows.item())
    out = ops.roiaware_sparse_pool(st, n_rows if rows is None else rows)
    res = {k: v.detach().cpu().numpy() for k, v in out.items()}
    res["n_rows"], res["faked"] = n_rows, int(res["faked"][0])
    if grads is not None:
        g_part, g_rpn = grads(n_rows if rows is None else rows)
        (out["part"] * _g(g_part)).sum().add((out["rpn"] * _g(g_rpn)).sum()).backward()
        res["d_part"], res["d_rpn"] = tp.grad.cpu().numpy(), tr.grad.cpu().numpy()
        res["g_part"], res["g_rpn"] = g_part, g_rpn
    return res


def _same(got, want):
    assert got["n_rows"] == want["n_rows"] and got["faked"] == want["faked"]
    for k in ("coords", "cnt", "arg", "row_of_cell"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    for k in ("part", "rpn"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


def _float_scene(seed, cnt, n, c):
    rois, pts, cnt, part, rpn = _scene(seed, cnt, n, c=c)
    rpn = np.random.default_rng(seed + 100).normal(size=rpn.shape).astype(F32)
    return rois, pts, cnt, part, rpn


def _grads(c, seed=0):
    def make(rows):
        rng = np.random.default_rng(seed)
        return rng.normal(size=(rows, 4)).astype(F32), rng.normal(size=(rows, c)).astype(F32)
    return make


# one case per kernel path: frames below / across the 1024-point collection chunk, an empty frame, one and several RoIs
# per frame, cells in LDS (<= 8192) and in the workspace (21 * 20 * 20 = 8400), caps of 1, 3 and 127 kept points, the
# channel counts below, at and across one wave (4 + c lanes: 5, 20, 134 -> three passes)
CASES = [
    ((130, 63), 5, (2, 3, 4), 128, 16),
    ((130, 63), 1, (12, 12, 12), 4, 1),
    ((1025, 2500), 5, (12, 12, 12), 128, 16),
    ((1025, 2500), 1, (2, 3, 4), 2, 130),
    ((0, 77), 5, (2, 3, 4), 4, 16),
    ((0, 77), 1, (12, 12, 12), 2, 130),
    ((130, 63), 5, (21, 20, 20), 4, 1),
    ((1025, 2500), 1, (21, 20, 20), 128, 16),
]


@pytest.mark.parametrize("cnt,n,out_size,max_pts,c", CASES)
def test_op_equals_restatement_bit_for_bit(cnt, n, out_size, max_pts, c):
    scene = _float_scene(21, cnt, n, c)
    got = _run(scene, out_size, max_pts, grads=_grads(c))
    want = sref.pool(*scene, out_size, max_pts)
    _same(got, want)
    assert got["n_rows"] >= 3 and not got["faked"]
    p = scene[1].shape[0]
    assert np.array_equal(_bits(got["d_part"]), _bits(sref.pool_bwd(want, got["g_part"], p, n, 1)))
    assert np.array_equal(_bits(got["d_rpn"]), _bits(sref.pool_bwd(want, got["g_rpn"], p, n, 0)))
    assert np.abs(got["d_part"]).sum() > 0 and np.abs(got["d_rpn"]).sum() > 0
    from spx import ops
    ops.check_status(DEV)


def test_integer_valued_features_are_exact_and_runs_repeat():
    scene = _scene(4, (1025, 2500), 5, c=16)                        # integer rpn; part made integer-valued too
    scene = scene[:3] + (np.round(scene[3] * 8).astype(F32), scene[4])
    g = lambda rows: (np.ones((rows, 4), F32), np.ones((rows, 16), F32))
    a = _run(scene, (12, 12, 12), 128, grads=g)
    b = _run(scene, (12, 12, 12), 128, grads=g, frame_cnt=False)    # the counts from the frame column
    want = sref.pool(*scene, (12, 12, 12), 128)
    _same(a, want)
    for k in ("coords", "cnt", "arg", "row_of_cell", "part", "rpn", "d_part", "d_rpn"):
        assert np.array_equal(_bits(a[k]) if a[k].dtype == F32 else a[k], _bits(b[k]) if b[k].dtype == F32 else b[k]), k
    # exact in float64 too: sums of small integers
    rpn_sum = np.zeros_like(scene[4], dtype=np.float64)
    rows, ch = np.nonzero(want["arg"] >= 0)
    np.add.at(rpn_sum, (want["arg"][rows, ch], ch), 1.0)
    assert np.array_equal(a["d_rpn"].astype(np.float64), rpn_sum)


@pytest.mark.parametrize("cells", [(), (5,), (0, 6)])
def test_fake_branch_on_the_device(cells):
    scene = _grid_scene(cells=cells, zero_cells=(3,), n_rois=3)
    scene = (np.concatenate([scene[0], scene[0]]), np.concatenate([scene[1], scene[1] + [1, 0, 0, 0]]).astype(F32),
             np.asarray([scene[2][0]] * 2, np.int32), np.concatenate([scene[3]] * 2), np.concatenate([scene[4]] * 2))
    if cells:                                                        # frame 1 emits nothing: the batch total decides
        scene[3][scene[2][0]:] = 0
    got = _run(scene, (2, 2, 2), 128, grads=_grads(2))
    want = sref.pool(*scene, (2, 2, 2), 128)
    _same(got, want)
    assert got["faked"] == 1 and got["n_rows"] == 6
    p = scene[1].shape[0]
    assert np.array_equal(_bits(got["d_part"]), _bits(sref.pool_bwd(want, got["g_part"], p, 3, 1)))
    assert np.array_equal(_bits(got["d_rpn"]), _bits(sref.pool_bwd(want, got["g_rpn"], p, 3, 0)))


def test_static_capacity_dead_rows_overflow_and_frame_bound():
    from spx import _lib, ops
    scene = _float_scene(8, (130, 63), 5, 16)
    exact = _run(scene, (2, 3, 4), 4)
    n = exact["n_rows"]
    big = _run(scene, (2, 3, 4), 4, rows=n + 37, grads=_grads(16), max_frame_points=130)
    _same(big, sref.pool(*scene, (2, 3, 4), 4, rows=n + 37))
    for k in ("coords", "part", "rpn", "arg", "cnt"):
        assert np.array_equal(big[k][:n], exact[k]), k
    want = sref.pool(*scene, (2, 3, 4), 4, rows=n + 37)
    assert np.array_equal(_bits(big["d_rpn"]), _bits(sref.pool_bwd(want, big["g_rpn"], 193, 5, 0)))
    ops.check_status(DEV)
    small = _run(scene, (2, 3, 4), 4, rows=n - 5, grads=_grads(16))
    want = sref.pool(*scene, (2, 3, 4), 4, rows=n - 5)
    _same(small, want)
    assert np.array_equal(_bits(small["d_part"]), _bits(sref.pool_bwd(want, small["g_part"], 193, 5, 1)))
    with pytest.raises(_lib.SpxError):
        ops.check_status(DEV)
    ops.check_status(DEV)                                            # read and reset
    _run(scene, (2, 3, 4), 4, max_frame_points=129)                  # a frame longer than the bound: reported, in bounds
    with pytest.raises(_lib.SpxError):
        ops.check_status(DEV)


def test_capture_and_replay_on_a_second_scene():
    from spx import ops
    a = _float_scene(31, (130, 63), 5, 16)
    b = _float_scene(32, (100, 93), 5, 16)
    cap = 400
    ops.status_word(DEV)
    bufs = [_g(x).clone() for x in a]
    def step():
        st = ops.roiaware_sparse_collect(bufs[0], bufs[1], bufs[3], bufs[4], (4, 4, 4), 4, frame_cnt=bufs[2])
        return ops.roiaware_sparse_pool(st, cap)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for scene in (b, a):
        for dst, src in zip(bufs, scene):
            dst.copy_(_g(src))
        graph.replay()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["n_rows"], got["faked"] = int(got["n_rows"][0]), int(got["faked"][0])
        want = sref.pool(*scene, (4, 4, 4), 4, rows=cap)
        assert 3 <= want["n_rows"] < cap
        _same(got, want)
    ops.check_status(DEV)


def test_points_in_boxes_stack_equal_and_ragged_frames():
    from spx import ops
    rois, pts, _, _, _ = _scene(11, (700, 700, 700), 300)             # 300 boxes: two LDS chunks of 256
    rois[1, 1] = rois[1, 0]
    got = ops.points_in_boxes_stack(_g(pts), _g(rois))
    dense = ops.points_in_boxes(_g(pts[:, 1:].reshape(3, 700, 3)), _g(rois))
    assert got.dtype == torch.int32 and torch.equal(got, dense.reshape(-1)) and int((got >= 0).sum()) > 500
    rois, pts, _, _, _ = _scene(12, (130, 63, 0, 600), 7)
    pts = np.concatenate([pts, np.asarray([[-1, 0, 0, 0], [4, 0, 0, 0], [np.nan, 0, 0, 0]], F32)])
    want = sref.points_in_boxes_stack(pts, rois)
    assert np.array_equal(ops.points_in_boxes_stack(_g(pts), _g(rois)).cpu().numpy(), want)
    perm = np.random.default_rng(0).permutation(pts.shape[0])         # frames interleaved inside every workgroup
    assert np.array_equal(ops.points_in_boxes_stack(_g(pts[perm]), _g(rois)).cpu().numpy(), want[perm])
    empty = ops.points_in_boxes_stack(_g(pts), _g(rois[:, :0]))
    assert (empty == -1).all()


# --------------------------------------------------------------------------------------------------------- the heads
import copy      # noqa: E402
import functools  # noqa: E402
import os        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/PartA2.yaml")


def _roi_head(pool_size=4, channels=16, **pool_over):
    import part_a2_ref as A
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads import PartA2FCHead
    torch.manual_seed(3)
    return PartA2FCHead(input_channels=channels, model_cfg=AttrDict(A.roi_head_cfg(pool_size, **pool_over)),
                        num_class=1).to(DEV)


def _head_batch(seed=41, cnt=(130, 63), n=5, channels=16):
    rois, pts, _, part, rpn = _float_scene(seed, cnt, n, channels)
    rng = np.random.default_rng(seed)
    score = np.where(part[:, 3] > 0, rng.uniform(0.0, 1.0, part.shape[0]), 0.0).astype(F32)
    return dict(batch_size=len(cnt), rois=_g(rois), point_coords=_g(pts), point_features=_g(rpn),
                point_part_offset=_g(part[:, :3]), point_cls_scores=_g(score))


def _targets(n_rois, seed=0):
    g = torch.Generator().manual_seed(seed)
    b, n = n_rois
    return dict(rcnn_cls_labels=torch.rand(b, n, generator=g).to(DEV), reg_valid_mask=torch.ones(b, n, dtype=torch.int64, device=DEV))


def _pool_rows(head, batch, training=True):
    head.train(training)
    t = _targets(batch["rois"].shape[:2])
    fn = head.sparse_pool_fused if head.fused else head.sparse_pool_composed
    part, rpn, coords, n_valid = fn(dict(batch), t)
    return part, rpn, coords, n_valid, t


@pytest.mark.parametrize("pool_size", [4, 6])
def test_head_fused_eager_equals_the_composition(pool_size):
    batch = _head_batch()
    batch["point_part_offset"].requires_grad_(True)
    batch["point_features"].requires_grad_(True)
    outs = []
    for fused in (False, True):
        head = _roi_head(pool_size, FUSED=fused)
        part, rpn, coords, n_valid, _ = _pool_rows(head, batch)
        assert n_valid is None and coords.dtype == torch.int32 and part.shape[0] >= 3
        g = torch.Generator().manual_seed(1)
        w1, w2 = torch.randn(part.shape, generator=g).to(DEV), torch.randn(rpn.shape, generator=g).to(DEV)
        grads = torch.autograd.grad((part * w1).sum() + (rpn * w2).sum(), [batch["point_part_offset"], batch["point_features"]])
        outs.append((part, rpn, coords) + grads)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # and through the whole head: the sparse conv branches and the dense tensor the FC layers read are bit-equal, so the
    # two paths hand identical inputs to identical FC layers.  Those layers go through torch's BLAS path, whose float32
    # sums over the 32 * pool^3 inputs are not reproducible from one call to the next (profiles/part_a2_fc_repeat.log,
    # tools/part_a2_bench.py --fc-repeat: the composition alone, the same batch four times, differs from itself after
    # shared_fc_layer while every stage before it is bit-equal).  Past them the outputs are compared to 1e-5, far above
    # what reordering such a sum can move (K eps |terms|, K <= 6912) and far below any real difference between rows.
    head = _roi_head(pool_size, FUSED=False).eval()
    res = []
    for fused in (False, True):
        head.fused = fused
        seen = {}
        hooks = [head.conv_part.register_forward_hook(lambda m, i, o: seen.__setitem__("part", o.features.clone())),
                 head.conv_rpn.register_forward_hook(lambda m, i, o: seen.__setitem__("rpn", o.features.clone())),
                 head.shared_fc_layer.register_forward_pre_hook(lambda m, i: seen.__setitem__("dense", i[0].clone()))]
        with torch.no_grad():
            out = head(dict(batch))
        for h in hooks:
            h.remove()
        res.append((seen["part"], seen["rpn"], seen["dense"], out["batch_cls_preds"].clone(), out["batch_box_preds"].clone()))
    for k in range(3):
        assert torch.equal(res[0][k], res[1][k]), k
    assert res[0][2].abs().sum() > 0 and torch.isfinite(res[0][4]).all()
    assert torch.allclose(res[0][3], res[1][3], rtol=1e-4, atol=1e-5) and torch.allclose(res[0][4], res[1][4], rtol=1e-4, atol=1e-5)


def test_head_static_rows_equal_eager_on_the_live_rows_and_fake_invalidates_labels():
    from spx import ops
    batch = _head_batch()
    eager = _pool_rows(_roi_head(4, FUSED=True), batch)
    n = eager[0].shape[0]
    static = _pool_rows(_roi_head(4, FUSED=True, STATIC_ROWS=n + 50), batch)
    assert static[3] is not None and int(static[3]) == n and static[0].shape[0] == n + 50
    for a, b in zip(eager[:3], static[:3]):
        assert torch.equal(a, b[:n])
    assert not static[0][n:].any() and not static[1][n:].any() and (static[2][n:] == -1).all()
    assert torch.equal(static[4]["rcnn_cls_labels"], eager[4]["rcnn_cls_labels"]) and (static[4]["reg_valid_mask"] == 1).all()
    # whole head, eval: the dense tensor the FC layers read is the same
    res = []
    for over in (dict(FUSED=True), dict(FUSED=True, STATIC_ROWS=n + 50)):
        head = _roi_head(4, **over).eval()
        with torch.no_grad():
            out = head(dict(batch))
        res.append(out["batch_box_preds"])
    assert torch.allclose(res[0], res[1], rtol=1e-5, atol=1e-6)
    ops.check_status(DEV)
    # a batch that emits nothing: faked rows, labels invalidated without a host read
    empty = dict(batch, point_cls_scores=torch.zeros_like(batch["point_cls_scores"]),
                 point_part_offset=torch.zeros_like(batch["point_part_offset"]))
    for over in (dict(FUSED=False), dict(FUSED=True), dict(FUSED=True, STATIC_ROWS=64)):
        part, rpn, coords, n_valid, t = _pool_rows(_roi_head(4, **over), empty)
        live = 10 if n_valid is None else int(n_valid)
        assert live == 10 and (coords[:10, 1:] == 0).all() and torch.equal(coords[:10, 0], torch.arange(10, device=DEV).int())
        assert (t["rcnn_cls_labels"] == -1).all() and (t["reg_valid_mask"] == -1).all()
    ops.check_status(DEV)


def test_eval_second_stage_with_static_rows_captures_and_replays_on_a_second_scene():
    from spx import ops
    a, b = _head_batch(41, (130, 63)), _head_batch(42, (100, 93))
    head = _roi_head(4, FUSED=True, STATIC_ROWS=400).eval()
    eager = _roi_head(4, FUSED=True).eval()
    eager.load_state_dict(head.state_dict())
    bufs = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
    ops.status_word(DEV)

    def run(m, batch):
        with torch.no_grad():
            out = m(dict(batch))
        return out["batch_cls_preds"], out["batch_box_preds"], out["roiaware_layout_ok"]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(2):
            run(head, bufs)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(head, bufs)
    for scene in (b, a):
        for k, v in scene.items():
            if isinstance(v, torch.Tensor):
                bufs[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        want = run(eager, scene)
        assert bool(out[2]) and torch.isfinite(out[1]).all()
        # the linear layers go through the BLAS library, whose kernel choice may differ between a captured and an eager call
        assert torch.allclose(out[0], want[0], rtol=1e-4, atol=1e-5) and torch.allclose(out[1], want[1], rtol=1e-4, atol=1e-5)
    ops.check_status(DEV)


@functools.lru_cache(maxsize=None)
def _detector():
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    roi = cfg.MODEL.ROI_HEAD
    roi.TARGET_CONFIG.ROI_PER_IMAGE = 16
    roi.NMS_CONFIG.TRAIN.NMS_POST_MAXSIZE = 64
    roi.NMS_CONFIG.TEST.NMS_POST_MAXSIZE = 16
    roi.ROI_AWARE_POOL.POOL_SIZE = 6                                   # 128 * 6^3 inputs to the first FC layer
    roi.SHARED_FC, roi.CLS_FC, roi.REG_FC = [64, 64], [64], [64]
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=0)     # the reduced 12.8 m x 16 m geometry
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, ds).to(DEV)
    batch = ds.collate_batch([ds[0], ds[1]])
    batch = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    return model, batch


@pytest.mark.parametrize("path", ["composition", "fused", "static"])
def test_training_step_of_the_small_detector_is_finite(path):
    from spx import ops
    model, batch = _detector()
    state = copy.deepcopy(model.state_dict())
    head = model.roi_head
    head.fused, head.static_rows = path != "composition", (16384 if path == "static" else None)
    try:
        model.train()
        model.zero_grad(set_to_none=True)
        torch.manual_seed(7)
        ret, tb, _ = model(dict(batch))
        loss = ret["loss"]
        assert loss.dim() == 0 and torch.isfinite(loss)
        loss.backward()
        for key in ("rpn_loss", "point_loss_cls", "point_loss_part", "point_pos_num", "rcnn_loss_cls", "rcnn_loss_reg"):
            assert isinstance(tb[key], torch.Tensor) and tb[key].dim() == 0 and torch.isfinite(tb[key]), key
        for name, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert float(tb["point_pos_num"]) > 0
        fwd = head.forward_ret_dict
        assert fwd["rois"].shape == (2, 16, 7) and fwd["rcnn_cls"].shape == (32, 1) and fwd["rcnn_reg"].shape == (32, 7)
        labels = model.point_head.forward_ret_dict["point_part_labels"]
        assert labels.shape[1] == 3 and float(labels.min()) >= 0 and float(labels.max()) <= 1 and float(labels.sum()) > 0
        ops.check_status(DEV)
    finally:
        head.fused, head.static_rows = False, None
        model.load_state_dict(state)


def test_the_float64_stand_in_of_the_recordings_is_spx_submconv3d():
    """tests/golden/part_a2.npz is recorded with SubMConv3d as a dense conv3d read back at the active sites
    (part_a2_ref.SubMConv3d).  The same weight in spx's own SubMConv3d gives the same rows on the device."""
    import part_a2_ref as A
    import spx
    rng = np.random.default_rng(5)
    cells = np.sort(rng.choice(3 * 64, 70, replace=False))
    idx = np.stack([cells // 64, (cells // 16) % 4, (cells // 4) % 4, cells % 4], 1).astype(np.int32)
    feats = rng.normal(size=(70, 4)).astype(F32)
    torch.manual_seed(1)
    real = spx.SubMConv3d(4, 64, 3, bias=False, indice_key="k").to(DEV)
    ref = A.SubMConv3d(4, 64, 3).double()
    with torch.no_grad():
        ref.weight.copy_(real.weight.detach().cpu().double())
        got = real(spx.SparseConvTensor(_g(feats), _g(idx), [4, 4, 4], 3)).features.cpu()
        want = ref(A.SparseConvTensor(torch.from_numpy(feats).double(), torch.from_numpy(idx), [4, 4, 4], 3)).features
    assert got.shape == want.shape == (70, 64)
    # float32 sums of at most 27 * 4 products of O(1) values against float64
    assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
