"""roiaware_pool3d without a GPU: the numpy restatement (tests/roiaware_ref.py) against plain-Python runs of the
reference's serial loops, closed-form boundary cases, the host op points_in_boxes_cpu, the box_utils helpers, and the
C ABI's argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import roiaware_ref as ref

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ plain-Python simulation of the reference's loops

def _sim_in_box(pt, box, margin):
    x, y, z = (F32(v) for v in pt)
    cx, cy, cz, dx, dy, dz, rz = (F32(v) for v in box)
    if F64(abs(z - cz)) > F64(dz) / 2.0:
        return False, F32(0), F32(0)
    cosa, sina = F32(math.cos(float(-rz))), F32(math.sin(float(-rz)))
    sx, sy = x - cx, y - cy
    lx = sx * cosa + sy * (-sina)
    ly = sx * sina + sy * cosa
    return bool(F64(abs(lx)) < F64(dx) / 2.0 + margin and F64(abs(ly)) < F64(dy) / 2.0 + margin), lx, ly


def _sim_axis(local, d, o):
    with np.errstate(all="ignore"):
        f = (local + d / F32(2)) / (d / F32(o))
    i = 0 if math.isnan(f) else int(max(-2147483648.0, min(2147483647.0, math.trunc(float(f)))))
    return min(i & 0xFFFFFFFF, o - 1)


def _sim_points_in_boxes(pts, boxes):
    out = np.full(pts.shape[:2], -1, np.int32)
    for b in range(pts.shape[0]):
        for i in range(pts.shape[1]):
            for k in range(boxes.shape[1]):
                if _sim_in_box(pts[b, i], boxes[b, k], ref.GPU_MARGIN)[0]:
                    out[b, i] = k
                    break
    return out


def _sim_pool(rois, pts, feats, out_size, max_pts, mode):
    """generate_pts_mask_for_box3d + collect_inside_pts_for_box3d (:78-108) + the per-voxel pools, serially."""
    ox, oy, oz = out_size
    n, npt, c = len(rois), len(pts), feats.shape[1]
    vox = np.zeros((n, ox, oy, oz, max_pts), np.int64)
    for r in range(n):
        for k in range(npt):
            ins, lx, ly = _sim_in_box(pts[k], rois[r], ref.GPU_MARGIN)
            if not ins:
                continue
            lz = F32(pts[k][2]) - F32(rois[r][2])
            xi = _sim_axis(lx, F32(rois[r][3]), ox)
            yi = _sim_axis(ly, F32(rois[r][4]), oy)
            zi = _sim_axis(lz, F32(rois[r][5]), oz)
            cnt = vox[r, xi, yi, zi, 0]
            if cnt < max_pts - 1:
                vox[r, xi, yi, zi, cnt + 1] = k
                vox[r, xi, yi, zi, 0] += 1
    pooled = np.zeros((n, ox, oy, oz, c), F32)
    argmax = np.zeros((n, ox, oy, oz, c), np.int32)
    for idx in np.ndindex(n, ox, oy, oz):
        lst = vox[idx][1:1 + vox[idx][0]]
        for ch in range(c):
            if mode == 0:
                am, mv = -1, F32(-np.inf)
                for k in lst:
                    if feats[k, ch] > mv:
                        mv, am = feats[k, ch], k
                if am != -1:
                    pooled[idx + (ch,)] = mv
                argmax[idx + (ch,)] = am
            else:
                s = F32(0)
                for k in lst:
                    s = s + feats[k, ch]
                if len(lst):
                    pooled[idx + (ch,)] = s / F32(len(lst))
    return pooled, argmax, vox


def _sim_bwd(vox, argmax, grad_out, npt, mode):
    """The reference's two backward kernels, run serially RoI by RoI (the ascending order the restatement pins)."""
    n, ox, oy, oz, c = grad_out.shape
    gi = np.zeros((npt, c), F32)
    for idx in np.ndindex(n, ox, oy, oz):
        lst = vox[idx][1:1 + vox[idx][0]]
        for ch in range(c):
            if mode == 0:
                if argmax[idx + (ch,)] != -1:
                    gi[argmax[idx + (ch,)], ch] += grad_out[idx + (ch,)] * F32(1)
            else:
                cur = F32(1) / max(F32(len(lst)), F32(1))
                for k in lst:
                    gi[k, ch] += grad_out[idx + (ch,)] * cur
    return gi


def _rand_case(seed, n=4, npt=160, c=3, lattice=False):
    rng = np.random.default_rng(seed)
    if lattice:
        pts = (rng.integers(-4, 5, size=(npt, 3)) * 0.5).astype(F32)
    else:
        pts = rng.uniform(-3, 3, size=(npt, 3)).astype(F32)
    rois = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(1.5, 4, (n, 3)),
                           rng.choice([0.0, np.pi / 2, np.pi, 0.3, -1.1], (n, 1))], axis=1).astype(F32)
    feats = rng.normal(size=(npt, c)).astype(F32)
    if lattice:
        feats = rng.integers(-2, 3, size=(npt, c)).astype(F32)      # ties between points
    return rois, pts, feats


# ------------------------------------------------------------------ restatement vs simulation

@pytest.mark.parametrize("lattice", [False, True])
def test_points_in_boxes_matches_serial_scan(lattice):
    rng = np.random.default_rng(3)
    rois, pts, _ = _rand_case(5 if lattice else 6, n=6, npt=150, lattice=lattice)
    pts = np.stack([pts, pts[rng.permutation(len(pts))]])
    boxes = np.stack([rois, rois[::-1].copy()])
    assert np.array_equal(ref.points_in_boxes(pts, boxes), _sim_points_in_boxes(pts, boxes))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", [(0, False, (3, 2, 4), 5), (1, True, (2, 2, 2), 4), (2, True, (1, 1, 1), 2),
                                  (3, False, (5, 3, 7), 128)])
def test_pool_matches_serial_reference(case, mode):
    seed, lattice, out, max_pts = case
    rois, pts, feats = _rand_case(seed, lattice=lattice)
    pooled, argmax, pt_cell, vox_cnt = ref.pool_fwd(rois, pts, feats, out, max_pts, mode)
    s_pooled, s_argmax, vox = _sim_pool(rois, pts, feats, out, max_pts, mode)
    assert np.array_equal(pooled.view(np.int32), s_pooled.view(np.int32))
    if mode == 0:
        assert np.array_equal(argmax, s_argmax)
    assert np.array_equal(vox_cnt, vox[..., 0])
    grad = np.random.default_rng(seed + 10).normal(size=pooled.shape).astype(F32)
    got = ref.pool_bwd(grad, argmax, pt_cell, vox_cnt, mode)
    assert np.array_equal(got.view(np.int32), _sim_bwd(vox, s_argmax, grad, len(pts), mode).view(np.int32))


# ------------------------------------------------------------------ closed-form cases

def _box(cx=0.0, cy=0.0, cz=0.0, dx=2.0, dy=2.0, dz=2.0, rz=0.0):
    return np.array([cx, cy, cz, dx, dy, dz, rz], F32)


def test_xy_margin_boundaries():
    box = _box()[None]
    xs = [1.0, -1.0, 1.0 + 0.5e-5, 1.0 + 2e-5, 1.0 + 0.5e-2, 1.0 + 2e-2]
    pts = np.array([[x, 0, 0] for x in xs] + [[0, y, 0] for y in xs], F32)
    gpu = ref.in_box(pts, box)[0][0]
    cpu = ref.points_in_boxes_cpu(pts, box)[0]
    assert gpu.tolist() == [True, True, True, False, False, False] * 2
    assert cpu.tolist() == [1, 1, 1, 1, 1, 0] * 2


def test_z_face_is_inside():
    pts = np.array([[0, 0, 1.0], [0, 0, -1.0], [0, 0, 1.0 + 1e-6], [0, 0, -1.0 - 1e-6]], F32)
    assert ref.in_box(pts, _box()[None])[0][0].tolist() == [True, True, False, False]


@pytest.mark.parametrize("rz", [0.0, np.pi / 2, -np.pi / 2, np.pi])
def test_rotations(rz):
    box = _box(dx=4.0, dy=1.0, rz=rz)[None]                   # long along its heading
    along = np.array([np.cos(rz), np.sin(rz), 0.0]) * 1.9
    across = np.array([-np.sin(rz), np.cos(rz), 0.0]) * 1.9
    pts = np.array([along, -along, across, -across], F32)
    assert ref.in_box(pts, box)[0][0].tolist() == [True, True, False, False]


def test_overlapping_boxes_first_index_wins():
    boxes = np.stack([_box(cx=5.0), _box(cx=0.5), _box(cx=0.0), _box(cx=0.2)])[None]
    pts = np.array([[[0.0, 0, 0], [1.3, 0, 0], [-0.9, 0, 0], [9, 9, 9]]], F32)
    assert ref.points_in_boxes(pts, boxes).tolist() == [[1, 1, 2, -1]]


def test_zero_padded_box_catches_origin_point():
    boxes = np.stack([_box(cx=10.0), np.zeros(7, F32), np.zeros(7, F32)])[None]
    pts = np.array([[[0, 0, 0], [0, 0, 1e-7], [5e-6, -5e-6, 0], [2e-5, 0, 0], [10, 0, 0]]], F32)
    assert ref.points_in_boxes(pts, boxes).tolist() == [[1, -1, 1, -1, 0]]


def test_full_cell_keeps_lowest_indices():
    rng = np.random.default_rng(0)
    pts = rng.uniform(-0.4, 0.4, size=(40, 3)).astype(F32)   # all in the one cell of a 1x1x1 grid
    pts[::3] = 5.0                                            # outside: every third point
    rois = _box()[None]
    pt_cell, vox_cnt, lists = ref.collect(rois, pts, (1, 1, 1), 8)
    inside = [k for k in range(40) if k % 3]
    assert vox_cnt.tolist() == [[7]]
    assert lists[0][0].tolist() == inside[:7]
    assert np.nonzero(pt_cell[0] >= 0)[0].tolist() == inside[:7]
    s_pooled, _, vox = _sim_pool(rois, pts, np.ones((40, 1), F32), (1, 1, 1), 8, 1)
    assert vox[0, 0, 0, 0, 1:8].tolist() == inside[:7]


def test_negative_cell_index_lands_in_last_cell():
    # the 1e-5 margin lets a point lie up to 1e-5 beyond the face of a 2e-5 wide box: (local_x + dx/2) / x_res is then
    # below -1, its int negative, and the unsigned clamp sends it to the last cell
    box = _box(dx=2e-5, dy=2.0, dz=2.0)[None]                 # x_res = 5e-6 with out_x = 4
    pts = np.array([[-1.9e-5, 0, 0], [1.9e-5, 0, 0], [0, 0, 0]], F32)
    code = ref.cell_codes(box, pts, (4, 1, 1))[0]
    assert code.tolist() == [3, 3, 2]
    assert ref.cell_axis(F32(-3.0), F32(2.0), 4) == 3
    assert ref.cell_axis(F32(np.nan), F32(2.0), 4) == 0
    assert ref.cell_axis(F32(np.inf), F32(0.0), 4) == 3


def test_max_pool_empty_and_nonfinite_voxels():
    rois = _box()[None]
    pts = np.array([[0.1, 0.1, 0.1], [0.2, 0.1, 0.1], [0.3, 0.1, 0.1]], F32)
    feats = np.array([[np.nan, -np.inf, 1.0], [-np.inf, np.nan, 1.0], [np.nan, np.nan, 1.0]], F32)
    pooled, argmax, _, _ = ref.pool_fwd(rois, pts, feats, (1, 1, 1), 128, 0)
    assert argmax.reshape(-1).tolist() == [-1, -1, 0]
    assert pooled.reshape(-1).tolist() == [0.0, 0.0, 1.0]


# ------------------------------------------------------------------ product module (host side)

def _ru():
    from pcdet_amd.ops.roiaware_pool3d import roiaware_pool3d_utils as ru
    return ru


def test_points_in_boxes_cpu_equals_restatement():
    rois, pts, _ = _rand_case(11, n=7, npt=3000)
    got = _ru().points_in_boxes_cpu(pts, rois)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (7, 3000)
    assert np.array_equal(got, ref.points_in_boxes_cpu(pts, rois))
    got_t = _ru().points_in_boxes_cpu(torch.from_numpy(pts), torch.from_numpy(rois))
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == torch.int32
    assert np.array_equal(got_t.numpy(), got)


def test_points_in_boxes_cpu_chunks(monkeypatch):
    ru = _ru()
    rois, pts, _ = _rand_case(12, n=5, npt=1001)
    want = ru.points_in_boxes_cpu(pts, rois)
    monkeypatch.setattr(ru, "_CPU_CHUNK", 37)
    assert np.array_equal(ru.points_in_boxes_cpu(pts, rois), want)


def test_pcdet_alias_resolves():
    import os
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tsm-det-pointcloud-_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as mod
    assert mod is _ru()
    for name in ("points_in_boxes_gpu", "points_in_boxes_cpu", "RoIAwarePool3d", "RoIAwarePool3dFunction"):
        assert hasattr(mod, name)


def test_gpu_entry_points_refuse_cpu_tensors():
    from spx import _lib
    ru = _ru()
    pts = torch.zeros((1, 8, 3))
    with pytest.raises(_lib.SpxError):
        ru.points_in_boxes_gpu(pts, torch.zeros((1, 2, 7)))
    with pytest.raises(_lib.SpxError):
        ru.RoIAwarePool3d(2)(torch.zeros((2, 7)), pts[0], torch.zeros((8, 4)))


def test_box_utils_helpers():
    from pcdet_amd.utils import box_utils, common_utils
    boxes = np.array([[0, 0, 0, 2, 2, 2, 0.3], [5, 5, 0, 1, 1, 1, 0]], F32)
    big = box_utils.enlarge_box3d(boxes, extra_width=(0.2, 0.3, 0.4))
    assert isinstance(big, torch.Tensor)
    assert np.allclose(big.numpy()[:, 3:6], boxes[:, 3:6] + np.array([0.2, 0.3, 0.4], F32))
    assert np.array_equal(big.numpy()[:, [0, 1, 2, 6]], boxes[:, [0, 1, 2, 6]])
    assert np.array_equal(box_utils.enlarge_box3d(torch.from_numpy(boxes)).numpy(), boxes)
    pts = np.array([[0, 0, 0, 7], [1.005, 0, 0, 8], [3, 3, 0, 9], [5.2, 5.2, 0.2, 10], [1.02, 0, 0, 11]], F32)
    left = box_utils.remove_points_in_boxes3d(pts, boxes[:, :7] * np.array([1, 1, 1, 1, 1, 1, 0], F32))
    assert isinstance(left, np.ndarray)
    assert left[:, 3].tolist() == [9.0, 11.0]
    t, is_np = common_utils.check_numpy_to_torch(pts)
    assert is_np and t.dtype == torch.float32
    assert common_utils.check_numpy_to_torch(t) == (t, False)


def test_argument_validation_without_gpu():
    from spx import _lib
    lib = _lib.load()
    assert lib.spx_points_in_boxes(None, None, 1, 10, 2, None, None) == -1
    assert lib.spx_points_in_boxes(None, None, -1, 10, 2, None, None) == -1
    assert lib.spx_points_in_boxes(None, None, 1, 10, -1, None, None) == -1
    assert lib.spx_points_in_boxes(None, None, 1, 0, 2, None, None) == 0
    assert lib.spx_roiaware_pool3d_ws_bytes(128, 16384, 14, 14, 14) >= 2 * 128 * 16384 * 4 + 128 * 14 ** 3 * 4
    assert lib.spx_roiaware_pool3d_ws_bytes(128, 16384, 256, 14, 14) == 0
    fwd = lib.spx_roiaware_pool3d_fwd
    assert fwd(None, None, None, 4, 10, 3, 2, 2, 2, 8, 0, None, None, None, None, None, 0, None) == -1
    assert fwd(None, None, None, -1, 10, 3, 2, 2, 2, 8, 0, None, None, None, None, None, 0, None) == -1
    assert fwd(None, None, None, 4, 10, 3, 0, 2, 2, 8, 0, None, None, None, None, None, 0, None) == -1
    assert fwd(None, None, None, 4, 10, 3, 2, 2, 2, 0, 0, None, None, None, None, None, 0, None) == -1
    assert fwd(None, None, None, 4, 10, 3, 2, 2, 2, 8, 2, None, None, None, None, None, 0, None) == -1
    assert fwd(None, None, None, 0, 10, 3, 2, 2, 2, 8, 0, None, None, None, None, None, 0, None) == 0
    p = ctypes.c_void_p(256)   # never dereferenced: the workspace check comes first
    assert fwd(p, p, p, 4, 10, 3, 2, 2, 2, 8, 0, p, p, p, p, None, 0, None) == -2
    assert fwd(p, p, p, 4, 10, 3, 2, 2, 2, 8, 0, p, None, p, p, p, 1 << 30, None) == -1
    bwd = lib.spx_roiaware_pool3d_bwd
    assert bwd(None, None, None, None, 4, 10, 3, 2, 2, 2, 0, None, None) == -1
    assert bwd(None, None, None, None, 4, -10, 3, 2, 2, 2, 0, None, None) == -1
    assert bwd(None, None, None, None, 4, 10, 3, 2, 2, 2, 1, None, None) == -1
