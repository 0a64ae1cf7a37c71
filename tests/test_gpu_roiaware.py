"""roiaware_pool3d HIP kernels (csrc/roiaware_pool3d.hip) against the float32 numpy restatement (tests/roiaware_ref.py):
box indices bit-exact, pooled features and argmax exact, the backward bit-exact, deterministic and close to float64
torch, autograd and graph capture."""
import numpy as np
import pytest
import torch

import roiaware_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32 = np.float32


def _ru():
    from pcdet_amd.ops.roiaware_pool3d import roiaware_pool3d_utils as ru
    return ru


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.asarray(a, F32).view(np.int32)


def _kitti(batch, m, seed=0):
    """KITTI synthetic frames (m points each, sampled with replacement when short) and their gt boxes, zero-padded to
    the longest frame as the collate does: points (B, m, 3), gt (B, T, 8)."""
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    pts, gts = [], []
    for i in range(batch):
        f = syn.make_frame(1, i)
        p = f["points"][:, :3]
        pts.append(p[rng.choice(p.shape[0], m, replace=p.shape[0] < m)])
        gts.append(f["gt_boxes"])
    t = max(g.shape[0] for g in gts)
    gt = np.zeros((batch, t, 8), F32)
    for i, g in enumerate(gts):
        gt[i, :g.shape[0]] = g
    return np.ascontiguousarray(np.stack(pts).astype(F32)), gt


def _jittered_rois(gt, n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    base = gt[rng.integers(0, gt.shape[0], n), :7].astype(np.float64)
    base[:, 0:3] += rng.normal(scale=0.3 * scale, size=(n, 3))
    base[:, 3:6] *= rng.uniform(0.9, 1.3, size=(n, 3))
    base[:, 6] += rng.normal(scale=0.2, size=n)
    return base.astype(F32)


def _check_pib(pts, boxes):
    got = _ru().points_in_boxes_gpu(_g(pts), _g(boxes))
    assert got.dtype == torch.int32 and tuple(got.shape) == pts.shape[:2]
    want = ref.points_in_boxes(pts, boxes)
    assert np.array_equal(got.cpu().numpy(), want)
    return want


# ------------------------------------------------------------------------------------------------ points in boxes

def test_points_in_boxes_kitti_gt_and_enlarged():
    from pcdet_amd.utils import box_utils
    pts, gt = _kitti(4, 16384)
    want = _check_pib(pts, gt[:, :, :7])
    assert (want >= 0).sum() > 100                                    # the frames have foreground
    big = torch.stack([box_utils.enlarge_box3d(gt[i, :, :7], extra_width=(0.2, 0.2, 0.2)) for i in range(4)]).numpy()
    want_big = _check_pib(pts, big)
    assert (want_big >= 0).sum() > (want >= 0).sum()


def test_points_in_boxes_waymo_size():
    from pcdet_amd.datasets import synthetic as syn
    f = syn.make_frame(3, 0)
    pts = np.stack([f["points"][:163840, :3], f["points"][-163840:, :3]]).astype(F32)
    boxes = np.stack([_jittered_rois(f["gt_boxes"], 200, 5), _jittered_rois(f["gt_boxes"], 200, 6, 3.0)])
    boxes[1, 150:] = 0.0                                               # zero padding at the end of frame 1
    want = _check_pib(pts, boxes)
    assert (want >= 0).sum() > 1000


def _adversarial():
    """Points on and just beside the faces of rotated boxes, the z faces, overlapping boxes and zero-padded boxes."""
    boxes, pts = [], []
    for k, rz in enumerate([0.0, np.pi / 2, -np.pi / 2, np.pi, 0.7]):
        cx, cy, cz, dx, dy, dz = 3.0 * k, -2.0, 0.5, 2.0, 1.0, 1.5
        boxes.append([cx, cy, cz, dx, dy, dz, rz])
        c, s = np.cos(rz), np.sin(rz)
        for off in (0.0, 0.5e-5, 1e-5, 2e-5, -0.5e-5):
            for lx, ly in ((dx / 2 + off, 0.0), (-dx / 2 - off, 0.0), (0.0, dy / 2 + off), (0.0, -dy / 2 - off),
                           (dx / 2 + off, dy / 2 + off)):
                pts.append([cx + c * lx - s * ly, cy + s * lx + c * ly, cz])
        for dzo in (dz / 2, -dz / 2, dz / 2 + 1e-6, -dz / 2 - 1e-6):
            pts.append([cx, cy, cz + dzo])
    boxes.append([0.5, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0])                   # overlaps the next
    boxes.append([0.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0])
    pts += [[-0.9, 0.0, 0.0], [1.3, 0.0, 0.0], [0.0, 0.0, 0.0]]
    boxes += [[0.0] * 7] * 3                                             # padding
    pts += [[0.0, 0.0, 0.0], [5e-6, -5e-6, 0.0], [0.0, 0.0, 1e-7], [2e-5, 0.0, 0.0], [0.0, 9.0, 0.0]]
    return np.array(pts, F32), np.array(boxes, F32)


def test_points_in_boxes_adversarial():
    pts, boxes = _adversarial()
    want = _check_pib(pts[None], boxes[None])
    # a padding box takes an origin point only where no earlier box does: move the two real boxes away
    far = boxes.copy()
    far[-5:-3, 0] += 50.0
    want_far = _check_pib(pts[None], far[None])
    assert want_far[0, -5] == len(boxes) - 3 and want_far[0, -4] == len(boxes) - 3
    assert want_far[0, -3] == -1 and want_far[0, -2] == -1
    assert (want >= 0).sum() > 0


def test_points_in_boxes_no_boxes_and_many_boxes():
    pts, gt = _kitti(2, 4000, seed=1)
    got = _ru().points_in_boxes_gpu(_g(pts), torch.zeros((2, 0, 7), device=DEV))
    assert got.shape == (2, 4000) and bool((got == -1).all())
    many = np.stack([_jittered_rois(np.tile(gt[i], (100, 1)), 1000, 7 + i, 4.0) for i in range(2)])
    want = _check_pib(pts, many)
    assert (want >= 256).any()                                          # hits beyond the first LDS chunk


def test_points_in_boxes_ragged_m():
    pts, gt = _kitti(3, 1001, seed=2)
    _check_pib(pts, gt[:, :, :7])
    _check_pib(pts[:, :37], gt[:, :, :7])


# ------------------------------------------------------------------------------------------------ pooling

def _pool_case(n, npt, c, seed, spread=1.0):
    pts, gt = _kitti(1, npt, seed)
    rois = _jittered_rois(gt[0][gt[0, :, 3] > 0], n, seed + 1, spread)
    feats = np.random.default_rng(seed + 2).normal(size=(npt, c)).astype(F32)
    return rois, pts[0], feats


def _check_pool(rois, pts, feats, out, max_pts, mode):
    from spx import ops
    pooled, argmax, pt_cell, vox_cnt = ops.roiaware_pool3d_fwd(_g(rois), _g(pts), _g(feats), out, max_pts, mode)
    w_pooled, w_argmax, w_cell, w_cnt = ref.pool_fwd(rois, pts, feats, out, max_pts, mode)
    assert np.array_equal(_bits(pooled.cpu().numpy()), _bits(w_pooled))
    if mode == 0:
        assert np.array_equal(argmax.cpu().numpy(), w_argmax)
    assert np.array_equal(pt_cell.cpu().numpy(), w_cell)
    assert np.array_equal(vox_cnt.cpu().numpy(), w_cnt)
    grad = np.random.default_rng(9).normal(size=w_pooled.shape).astype(F32)
    gi = ops.roiaware_pool3d_bwd(_g(grad), argmax, pt_cell, vox_cnt, mode)
    w_gi = ref.pool_bwd(grad, w_argmax, w_cell, w_cnt, mode)
    assert np.array_equal(_bits(gi.cpu().numpy()), _bits(w_gi))
    # the same sum in float64, through torch's index_add_
    g = torch.from_numpy(grad).double().reshape(len(rois), -1, feats.shape[1])
    acc = torch.zeros((len(pts), feats.shape[1]), dtype=torch.float64)
    cell = torch.from_numpy(w_cell).long()
    cnt = torch.from_numpy(w_cnt).reshape(len(rois), -1).double()
    for r in range(len(rois)):
        p = torch.nonzero(cell[r] >= 0)[:, 0]
        v = cell[r, p]
        if mode == 0:
            am = torch.from_numpy(w_argmax).reshape(len(rois), -1, feats.shape[1])[r, v].long()
            contrib = torch.where(am == p[:, None], g[r, v], torch.zeros(()).double())
        else:
            contrib = g[r, v] / cnt[r, v].clamp_min(1)[:, None]
        acc.index_add_(0, p, contrib)
    assert np.allclose(gi.cpu().numpy(), acc.numpy(), rtol=1e-5, atol=1e-5)
    return pooled, argmax, pt_cell, vox_cnt, gi


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c", [128, 4])
def test_pool_parta2_shape(mode, c):
    rois, pts, feats = _pool_case(128, 16384, c, 20)
    _, _, pt_cell, vox_cnt, _ = _check_pool(rois, pts, feats, (14, 14, 14), 128, mode)
    assert int((pt_cell >= 0).sum()) > 1000


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", [((5, 3, 7), 128, 3), ((1, 1, 1), 128, 1), ((4, 4, 4), 2, 130), ((6, 5, 4), 5, 3),
                                  ((32, 16, 20), 4, 3)])
def test_pool_odd_shapes(case, mode):
    out, max_pts, c = case
    rois, pts, feats = _pool_case(24, 5000, c, 30 + c, spread=0.5)
    rois[12:] = rois[:12]                                               # overlapping (identical) RoIs
    rois[12:, 0] += 0.3
    _, _, _, vox_cnt, _ = _check_pool(rois, pts, feats, out, max_pts, mode)
    if max_pts == 2:
        assert int(vox_cnt.max()) == 1


def test_pool_ties_and_nonfinite():
    rois, pts, _ = _pool_case(8, 3000, 3, 40)
    feats = np.random.default_rng(41).integers(-1, 2, size=(3000, 3)).astype(F32)
    feats[::7, 0] = np.nan
    feats[::5, 1] = -np.inf
    for mode in (0, 1):
        _check_pool(rois, pts, feats, (3, 3, 3), 16, mode)


def test_pool_deterministic():
    from spx import ops
    rois, pts, feats = _pool_case(64, 16384, 32, 50)
    outs = []
    for _ in range(2):
        pooled, argmax, pt_cell, vox_cnt = ops.roiaware_pool3d_fwd(_g(rois), _g(pts), _g(feats), (7, 7, 7), 32, 0)
        gi = ops.roiaware_pool3d_bwd(torch.ones_like(pooled), argmax, pt_cell, vox_cnt, 0)
        outs.append([t.cpu().numpy() for t in (pooled, argmax, pt_cell, vox_cnt, gi)])
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.int32) if a.dtype == F32 else a, b.view(np.int32) if b.dtype == F32 else b)


@pytest.mark.parametrize("pool_method", ["max", "avg"])
def test_autograd(pool_method):
    ru = _ru()
    rois, pts, feats = _pool_case(16, 4000, 5, 60)
    f = _g(feats).requires_grad_(True)
    pooled = ru.RoIAwarePool3d(out_size=(4, 5, 6), max_pts_each_voxel=16)(_g(rois), _g(pts), f, pool_method)
    mode = 0 if pool_method == "max" else 1
    w_pooled, w_argmax, w_cell, w_cnt = ref.pool_fwd(rois, pts, feats, (4, 5, 6), 16, mode)
    assert np.array_equal(_bits(pooled.detach().cpu().numpy()), _bits(w_pooled))
    grad = np.random.default_rng(61).normal(size=w_pooled.shape).astype(F32)
    pooled.backward(_g(grad))
    assert np.array_equal(_bits(f.grad.cpu().numpy()), _bits(ref.pool_bwd(grad, w_argmax, w_cell, w_cnt, mode)))
    p2 = ru.RoIAwarePool3dFunction.apply(_g(rois), _g(pts), _g(feats), 3, 16, pool_method)
    assert p2.shape == (16, 3, 3, 3, 5)


def test_graph_capture():
    from spx import ops
    pts, gt = _kitti(2, 16384, seed=3)
    rois, ppts, feats = _pool_case(32, 8192, 16, 70)
    g_pts, g_gt, g_rois, g_ppts, g_feats = _g(pts), _g(gt[:, :, :7]), _g(rois), _g(ppts), _g(feats)
    grad = _g(np.random.default_rng(71).normal(size=(32, 6, 6, 6, 16)).astype(F32))

    def step():
        idx = ops.points_in_boxes(g_pts, g_gt)
        pooled, argmax, pt_cell, vox_cnt = ops.roiaware_pool3d_fwd(g_rois, g_ppts, g_feats, (6, 6, 6), 32, 0)
        gi = ops.roiaware_pool3d_bwd(grad, argmax, pt_cell, vox_cnt, 0)
        return idx, pooled, gi

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]                             # warm the workspace on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t in outs:
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, outs):
        assert torch.equal(a, b)
    assert np.array_equal(eager[0].cpu().numpy(), ref.points_in_boxes(pts, gt[:, :, :7]))


def test_point_head_target_assignment_loop():
    """point_head_template.py:115-127: per frame, gt boxes and enlarged boxes, ignore flags, class labels."""
    from pcdet_amd.utils import box_utils
    pts, gt = _kitti(4, 6000, seed=5)
    g_gt = _g(gt)
    ext = box_utils.enlarge_box3d(g_gt.view(-1, 8), extra_width=(0.2, 0.2, 0.2)).view(4, -1, 8)
    points = torch.cat([torch.cat([torch.full((6000, 1), float(k)), torch.from_numpy(pts[k])], 1)
                        for k in range(4)]).to(DEV)
    ru = _ru()
    labels = points.new_zeros(points.shape[0]).long()
    for k in range(4):
        bs_mask = points[:, 0] == k
        single = points[bs_mask][:, 1:4]
        lab = labels.new_zeros(int(bs_mask.sum()))
        box_idxs = ru.points_in_boxes_gpu(single.unsqueeze(0), g_gt[k:k + 1, :, 0:7].contiguous()).long().squeeze(0)
        fg = box_idxs >= 0
        ext_idxs = ru.points_in_boxes_gpu(single.unsqueeze(0), ext[k:k + 1, :, 0:7].contiguous()).long().squeeze(0)
        ignore = fg ^ (ext_idxs >= 0)
        lab[ignore] = -1
        lab[fg] = g_gt[k][box_idxs[fg]][:, -1].long()
        labels[bs_mask] = lab
    ext_np = ext.cpu().numpy()
    want = []
    for k in range(4):
        bi = ref.points_in_boxes(pts[k:k + 1], gt[k:k + 1, :, :7])[0]
        ei = ref.points_in_boxes(pts[k:k + 1], ext_np[k:k + 1, :, :7])[0]
        lab = np.zeros(6000, np.int64)
        lab[(bi >= 0) ^ (ei >= 0)] = -1
        lab[bi >= 0] = gt[k, bi[bi >= 0], 7].astype(np.int64)
        want.append(lab)
    assert np.array_equal(labels.cpu().numpy(), np.concatenate(want))
    assert (labels > 0).sum() > 0 and (labels < 0).sum() > 0
