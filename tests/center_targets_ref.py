"""Numpy restatement of the centre head's target assignment (csrc/center_targets.hip, include/spx.h §20) for a whole
batch and several heads, and the cases the tests run it on.

float32 wherever the reference (CenterHead.assign_target_of_single_head on CPU tensors) computes in float32, in its
operation order; the Gaussian in float64, rounded once, as the reference's numpy code does; log / cos / sin of the
target rows by torch on the CPU, as there.  Per head the semantics are
the INTENDED, non-mutating ones: every head filters the original class column (the reference overwrites it in place
while it filters, which corrupts the labels later heads see)."""
import numpy as np
import torch

F32 = np.float32

# the geometry of every case: W != H so that an x / y swap shows
W, H = 24, 20
STRIDE = 8
VOXEL_SIZE = [0.05, 0.05, 0.1]
RANGE = [0.0, -4.0, -3.0, 9.6, 4.0, 1.0]
OVERLAP = 0.1
MIN_RADIUS = 2
CELL = 0.4                          # metres per heatmap cell

ONE_HEAD = [[1, 2, 3]]              # global class ids (1-based) per head
TWO_HEADS = [[1], [2, 3]]


def gaussian_radius_f32(height, width, min_overlap):
    """gaussian_radius of centernet_utils on float32 arrays: the Python scalars are doubles that are rounded to float32
    where they meet the tensor."""
    height, width = np.asarray(height, F32), np.asarray(width, F32)
    mo = float(min_overlap)
    with np.errstate(invalid="ignore"):
        b1 = height + width
        c1 = width * height * F32(1 - mo) / F32(1 + mo)
        r1 = (b1 + np.sqrt(b1 * b1 - F32(4) * c1)) / F32(2)
        b2 = F32(2) * (height + width)
        c2 = F32(1 - mo) * width * height
        r2 = (b2 + np.sqrt(b2 * b2 - F32(16) * c2)) / F32(2)
        b3 = F32(-2 * mo) * (height + width)
        c3 = F32(mo - 1) * width * height
        r3 = (b3 + np.sqrt(b3 * b3 - F32(4 * (4 * mo)) * c3)) / F32(2)
    out = np.minimum(np.minimum(r1, r2), r3)
    assert out.dtype == F32
    return out


def gaussian_window(r):
    """(2r + 1, 2r + 1) float32: numpy float64 exp, rounded once."""
    sigma = (2 * r + 1) / 6
    y, x = np.ogrid[-r:r + 1, -r:r + 1]
    return np.exp(-(x * x + y * y).astype(np.float64) / (2 * sigma * sigma)).astype(F32)


def table_of(heads, num_class):
    """The op's int32 (num_class + 1, 2) table: (head, 1-based class within the head), -1 where no head owns the class."""
    t = np.full((num_class + 1, 2), -1, np.int32)
    for h, ids in enumerate(heads):
        for s, g in enumerate(ids):
            t[g] = (h, s + 1)
    return t


def assign(gt_boxes, heads, num_max_objs, rng=RANGE, voxel_size=VOXEL_SIZE, stride=STRIDE, size=(W, H),
           overlap=OVERLAP, min_radius=MIN_RADIUS, want_radius=False):
    """gt_boxes (B, M, C) float32, class (1-based, global) in the last column -> list over heads of dicts heatmap
    (B, C_h, H, W) f32, target_boxes (B, K, C) f32, inds, mask (B, K) int64 [, radius: the untruncated radii of the live
    slots]."""
    gt_boxes = np.asarray(gt_boxes, F32)
    b, m, c = gt_boxes.shape
    w, h = size
    k = num_max_objs
    x0, y0, vs0, vs1, st = F32(rng[0]), F32(rng[1]), F32(voxel_size[0]), F32(voxel_size[1]), F32(stride)
    out = []
    for ids in heads:
        o = dict(heatmap=np.zeros((b, len(ids), h, w), F32), target_boxes=np.zeros((b, k, c), F32),
                 inds=np.zeros((b, k), np.int64), mask=np.zeros((b, k), np.int64), radius=[])
        for f in range(b):
            cls = gt_boxes[f, :, -1].astype(np.int64)
            own = [i for i in range(m) if cls[i] in ids]                      # input order; class 0 (padding) owns nothing
            for slot, i in enumerate(own[:k]):
                g = gt_boxes[f, i]
                cx = np.clip((g[0] - x0) / vs0 / st, F32(0), F32(w - 0.5))
                cy = np.clip((g[1] - y0) / vs1 / st, F32(0), F32(h - 0.5))
                sdx, sdy = g[3] / vs0 / st, g[4] / vs1 / st
                if not (sdx > 0 and sdy > 0):
                    continue                                                  # the slot is kept: mask 0, zeros
                rad = gaussian_radius_f32(sdx, sdy, overlap)
                o["radius"].append(float(rad))
                r = max(int(rad), min_radius)
                ix, iy = int(cx), int(cy)
                win = gaussian_window(r)
                left, right = min(ix, r), min(w - ix, r + 1)
                top, bottom = min(iy, r), min(h - iy, r + 1)
                ch = o["heatmap"][f, ids.index(int(cls[i]))]
                np.maximum(ch[iy - top:iy + bottom, ix - left:ix + right],
                           win[r - top:r + bottom, r - left:r + right], out=ch[iy - top:iy + bottom, ix - left:ix + right])
                o["inds"][f, slot] = iy * w + ix
                o["mask"][f, slot] = 1
                row = o["target_boxes"][f, slot]
                row[0], row[1], row[2] = cx - F32(ix), cy - F32(iy), g[2]
                # torch's own CPU log / cos / sin on the shapes the reference calls them with (a 3-slice, a 0-d tensor):
                # numpy's float32 routines are another implementation and may differ in the last bit
                row[3:6] = torch.from_numpy(g[3:6].copy()).log().numpy()
                rz = torch.from_numpy(g[6:7].copy())[0]
                row[6], row[7] = torch.cos(rz).item(), torch.sin(rz).item()
                row[8:] = g[7:-1]
        if not want_radius:
            del o["radius"]
        out.append(o)
    return out


def ulp_distance(a, b):
    """Element-wise distance in float32 units in the last place (both finite, same sign or zero)."""
    a = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 31) - a, a)
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b)
    return np.abs(a - b)


def _box(cell_x, cell_y, dx, dy, cls, dz=1.5, z=-1.0, rz=0.3, extra=()):
    """A box whose centre lies at (cell_x, cell_y) in heatmap cells (fractions allowed, outside the map allowed)."""
    return [RANGE[0] + cell_x * CELL, RANGE[1] + cell_y * CELL, z, dx, dy, dz, rz, *extra, cls]


CAR, PED, CYC = (3.9, 1.6), (0.8, 0.6), (1.76, 0.6)
PAD = [0.0] * 8


def cases():
    """name -> dict(gt (frames, M, C) float32, heads, k = num_max_objs).  The sizes are fixed numbers chosen so that every
    untruncated radius is >= 1e-3 away from an integer (check_radius_margin), so no case hangs on the last bit of it."""
    c = {}
    # 1. two same-class boxes with overlapping windows (max), two boxes of different classes on one cell
    c["overlap"] = dict(heads=ONE_HEAD, k=8, gt=[[
        _box(10.3, 8.6, *CAR, 1), _box(12.7, 9.2, *CAR, 1, rz=-1.1), _box(5.5, 5.5, *PED, 2), _box(5.2, 5.9, *CYC, 3, rz=2.0)]])
    # 2. centres outside the map: low x / high y, and high x / low y (clamp, windows clipped on two sides)
    c["outside"] = dict(heads=ONE_HEAD, k=8, gt=[[_box(-1.75, 22.25, *CAR, 1), _box(27.5, -2.5, *CYC, 3, rz=-0.7)]])
    # 3. a centre in the last cell (W - 1, H - 1)
    c["corner"] = dict(heads=ONE_HEAD, k=8, gt=[[_box(23.4, 19.7, *CAR, 2, rz=1.2)]])
    # 4. dx = 0 between two valid boxes: the slot is kept with mask 0
    c["zero_dx"] = dict(heads=ONE_HEAD, k=8, gt=[[
        _box(4.2, 3.1, *PED, 2), _box(9.0, 9.0, 0.0, 1.6, 1), _box(15.6, 12.8, *CYC, 3, rz=0.9)]])
    # 5. six boxes of one head, four slots
    c["truncate"] = dict(heads=ONE_HEAD, k=4, gt=[[
        _box(2.5 + 3.6 * i, 3.5 + 2.4 * i, *(CAR, PED, CYC)[i % 3], 1 + i % 3, rz=0.4 * i) for i in range(6)]])
    # 6. padding rows in the middle of the list, and a frame with no box at all
    c["padding"] = dict(heads=ONE_HEAD, k=8, gt=[
        [_box(6.1, 4.4, *CAR, 1), PAD, _box(17.3, 14.2, *PED, 2, rz=-2.5), PAD, PAD, _box(11.8, 16.6, *CYC, 3)],
        [PAD] * 6])
    # 7. C = 10: two velocity columns land in target_boxes[:, 8:10]
    c["velocity"] = dict(heads=ONE_HEAD, k=8, gt=[[
        _box(7.7, 6.2, *CAR, 1, extra=(1.25, -0.5)), _box(14.1, 11.9, *PED, 2, extra=(-3.0, 0.75))]])
    # 8. a box small enough for min_radius to decide, one large enough for radius >= 6 (clipped at the low-x border)
    c["radii"] = dict(heads=ONE_HEAD, k=8, gt=[[_box(18.5, 4.5, 0.3, 0.3, 2), _box(4.6, 11.3, 6.4, 6.0, 1, rz=0.1)]])
    # two heads, classes interleaved so that the slots of a head are not the input positions
    c["two_heads"] = dict(heads=TWO_HEADS, k=8, gt=[
        [_box(3.3, 2.2, *PED, 2), _box(8.8, 7.1, *CAR, 1), _box(8.1, 7.9, *CYC, 3, rz=1.0), PAD, _box(16.4, 13.3, *CAR, 1),
         _box(20.6, 17.5, *PED, 2, rz=-0.2)],
        [_box(12.2, 9.9, *CYC, 3), _box(12.9, 9.1, *PED, 2), PAD, PAD, _box(1.4, 18.3, *CAR, 1, rz=2.9), PAD]])
    for v in c.values():
        v["gt"] = np.asarray(v["gt"], F32)
    return c


LOSS_CASES = ("overlap", "padding")      # the frames whose reference targets feed the recorded loss values
BATCH_K = 5     # the cases with 8 columns as one batch: "truncate" loses one box there, two on its own


def batch_of(all_cases, heads):
    """Every 8-column case's frames as one (B, M, 8) batch, zero-padded to the longest list."""
    frames = [f for v in all_cases.values() if v["gt"].shape[2] == 8 for f in v["gt"]]
    m = max(f.shape[0] for f in frames)
    gt = np.zeros((len(frames), m, 8), F32)
    for i, f in enumerate(frames):
        gt[i, :f.shape[0]] = f
    return gt


def check_radius_margin(all_cases):
    """Every untruncated radius of every case is >= 1e-3 away from an integer; returns the radii."""
    radii = []
    for v in all_cases.values():
        for o in assign(v["gt"], v["heads"], v["k"], want_radius=True):
            radii += o["radius"]
    radii = np.asarray(radii)
    assert radii.size and np.abs(radii - np.round(radii)).min() >= 1e-3, radii
    return radii
