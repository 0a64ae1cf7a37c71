"""Configs of the small Part-A2 heads shared by tests/test_part_a2_ref.py and tests/test_gpu_part_a2.py, and the CPU
stand-ins (restatement-backed) of the device ops the two heads call.  Not a test module."""
import contextlib

import numpy as np
import torch

import roiaware_ref
import roiaware_sparse_ref as sref


def point_head_cfg(**over):
    cfg = dict(NAME="PointIntraPartOffsetHead", CLS_FC=[], PART_FC=[], CLASS_AGNOSTIC=True,
               TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2]),
               LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS=dict(point_cls_weight=1.0, point_part_weight=1.0)))
    cfg.update(over)
    return cfg


def roi_head_cfg(pool_size, **pool_over):
    pool = dict(POOL_SIZE=pool_size, NUM_FEATURES=32, MAX_POINTS_PER_VOXEL=8)
    pool.update(pool_over)
    return dict(
        NAME="PartA2FCHead", CLASS_AGNOSTIC=True, SHARED_FC=[16, 16], CLS_FC=[16, 16], REG_FC=[16, 16], DP_RATIO=0.0,
        SEG_MASK_SCORE_THRESH=0.3,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=8,
                                   NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=8,
                                  NMS_THRESH=0.7)),
        ROI_AWARE_POOL=pool,
        TARGET_CONFIG=dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=4, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                           CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                           HARD_BG_RATIO=0.8, REG_FG_THRESH=0.65),
        LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0,
                                           code_weights=[1.0] * 7)))


# ------------------------------------------------------------------------------------------- CPU stand-ins of the ops
def cpu_points_in_boxes_stack(points_bxyz, boxes):
    return torch.from_numpy(sref.points_in_boxes_stack(points_bxyz.detach().numpy(), boxes.detach().numpy()))


def cpu_roiaware_pool3d_fwd(rois, pts, feats, out_size, max_pts, pool_method):
    pooled, argmax, pt_cell, vox_cnt = roiaware_ref.pool_fwd(rois.detach().numpy(), pts.detach().numpy(),
                                                             feats.detach().numpy(), out_size, max_pts, pool_method)
    t = torch.from_numpy
    return t(pooled), (None if argmax is None else t(argmax)), t(pt_cell), t(vox_cnt)


class _State(object):
    pass


def cpu_sparse_collect(rois, points, part, rpn, out_size, max_pts, frame_cnt=None, max_frame_points=None):
    st = _State()
    st.args = (rois.detach().numpy(), points.detach().numpy(), part.detach().numpy(), rpn.detach().numpy(),
               tuple(out_size), int(max_pts))
    b = rois.shape[0]
    frames = points.detach().numpy()[:, 0]
    st.cnt = np.asarray([(frames == f).sum() for f in range(b)], np.int32)
    st.layout_ok = torch.tensor(bool((np.diff(frames) >= 0).all()))
    st.fwd = sref.pool(st.args[0], st.args[1], st.cnt, st.args[2], st.args[3], st.args[4], st.args[5])
    st.n_rows = torch.tensor([st.fwd["n_rows"]], dtype=torch.int64)
    st.faked = torch.tensor([st.fwd["faked"]], dtype=torch.int32)
    return st


def cpu_sparse_pool(st, rows):
    r, p, part, rpn, out_size, max_pts = st.args
    fwd = sref.pool(r, p, st.cnt, part, rpn, out_size, max_pts, rows=rows)
    t = torch.from_numpy
    return {"coords": t(fwd["coords"]), "part": t(fwd["part"]), "rpn": t(fwd["rpn"]), "arg": t(fwd["arg"]),
            "cnt": t(fwd["cnt"]), "row_of_cell": t(fwd["row_of_cell"]), "n_rows": st.n_rows, "faked": st.faked,
            "layout_ok": st.layout_ok}


@contextlib.contextmanager
def cpu_ops():
    """The device ops the Part-A2 heads call, replaced by the restatements for the duration (forward only)."""
    from pcdet_amd.ops.roiaware_pool3d import roiaware_pool3d_utils as rp
    from spx import ops
    real = (rp.points_in_boxes_stack, ops.roiaware_pool3d_fwd, ops.roiaware_sparse_collect, ops.roiaware_sparse_pool)
    rp.points_in_boxes_stack = cpu_points_in_boxes_stack
    ops.roiaware_pool3d_fwd = cpu_roiaware_pool3d_fwd
    ops.roiaware_sparse_collect, ops.roiaware_sparse_pool = cpu_sparse_collect, cpu_sparse_pool
    try:
        yield
    finally:
        rp.points_in_boxes_stack, ops.roiaware_pool3d_fwd, ops.roiaware_sparse_collect, ops.roiaware_sparse_pool = real


def point_scene(seed=17, cnt=(130, 63, 0, 41), n=4, channels=64):
    """numpy inputs of the point head, float64 holding float32 values: points (P, 4) in four ragged frames (one empty),
    gt_boxes (4, n, 8) with a padded row, features (P, channels)."""
    from part_a2_scenes import scene as _scene
    rois, pts, _, _, _ = _scene(seed, cnt, n)
    gt = np.concatenate([rois, np.ones(rois.shape[:2] + (1,), np.float32)], -1).astype(np.float64)
    gt[1, 3] = 0
    feats = np.random.default_rng(seed).normal(size=(pts.shape[0], channels)).astype(np.float32).astype(np.float64)
    return dict(points=pts.astype(np.float64), gt_boxes=gt, features=feats)


# ------------------------------------------------ float64 CPU stand-ins for the recordings of PartA2FCHead
# Used on BOTH sides: tests/golden/make_golden_part_a2.py puts them into the reference's modules while recording, and
# tests/test_part_a2_ref.py puts them into this project's head (cpu_ops64).  What is compared is therefore everything the
# head itself does around them: the part features and the score mask, the per-frame loop, nonzero and the gather, the
# fake branch and its label invalidation, the order of the concatenation, the dense layout, the FC layers, the losses.
import types  # noqa: E402

import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SPARSE_LOG = []          # every stand-in SparseConvTensor, in the order of construction


class SparseConvTensor(object):
    def __init__(self, features, indices, spatial_shape, batch_size, **_unused):
        self.features, self.indices = features, indices
        self.spatial_shape, self.batch_size = [int(s) for s in spatial_shape], int(batch_size)
        SPARSE_LOG.append(self)

    def replace_feature(self, features):
        out = SparseConvTensor.__new__(SparseConvTensor)
        out.features, out.indices, out.spatial_shape, out.batch_size = features, self.indices, self.spatial_shape, self.batch_size
        return out

    def dense(self):
        i = self.indices.long()
        out = self.features.new_zeros([self.batch_size, self.features.shape[1]] + self.spatial_shape)
        out[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]] = self.features
        return out


class SubMConv3d(nn.Module):
    """A 3 x 3 x 3 submanifold convolution as a dense conv3d read back at the active sites; weight
    [C_out, k, k, k, C_in], the layout of spx.modules."""

    def __init__(self, in_channels, out_channels, kernel_size, bias=False, indice_key=None, **_unused):
        super().__init__()
        assert not bias
        k = int(kernel_size)
        self.weight = nn.Parameter(torch.empty(out_channels, k, k, k, in_channels))
        nn.init.kaiming_uniform_(self.weight, a=5 ** 0.5)
        self.pad = k // 2

    def forward(self, x):
        i = x.indices.long()
        y = F.conv3d(x.dense(), self.weight.permute(0, 4, 1, 2, 3), padding=self.pad)
        return x.replace_feature(y[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]])


class SparseSequential(nn.Module):
    def __init__(self, *mods):
        super().__init__()
        for k, m in enumerate(mods):
            self.add_module(str(k), m)

    def __getitem__(self, k):
        return list(self._modules.values())[k]

    def forward(self, x):
        for m in self._modules.values():
            if isinstance(m, (SparseSequential, SubMConv3d)):
                x = m(x)
            elif x.features.shape[0] != 0:
                x = x.replace_feature(m(x.features))
        return x


spconv_standin = types.SimpleNamespace(SparseSequential=SparseSequential, SubMConv3d=SubMConv3d,
                                       SparseConvTensor=SparseConvTensor)


def torch_roiaware_pool(self, rois, pts, pts_feature, pool_method='max'):
    """RoIAwarePool3d.forward: the point lists of roiaware_ref.collect (float32 geometry), the pooling itself in torch at
    the features' precision and differentiable.  Features without ties (strict > = the only maximum)."""
    size = self.out_size
    out_size = (size, size, size) if isinstance(size, int) else tuple(size)
    pt_cell, vox_cnt, _ = roiaware_ref.collect(rois.detach().numpy(), pts.detach().numpy(), out_size,
                                               self.max_pts_each_voxel)
    n, V, c = rois.shape[0], int(np.prod(out_size)), pts_feature.shape[1]
    r, p = np.nonzero(pt_cell >= 0)
    cell = torch.from_numpy(r * V + pt_cell[r, p]).long()
    src = pts_feature[torch.from_numpy(p)]
    out = pts_feature.new_zeros((n * V, c))
    if pool_method == 'avg':
        cnt = torch.from_numpy(vox_cnt.reshape(-1)).to(pts_feature.dtype).clamp(min=1)
        out = out.index_add(0, cell, src) / cnt.unsqueeze(1)
    else:
        out = out.scatter_reduce(0, cell.unsqueeze(1).expand(-1, c), src, 'amax', include_self=False)
    return out.view((n,) + out_size + (c,))


@contextlib.contextmanager
def cpu_ops64():
    """This project's PartA2FCHead on the float64 stand-ins (construct AND run the head inside)."""
    from pcdet_amd.models.roi_heads import partA2_head
    from pcdet_amd.ops.roiaware_pool3d import roiaware_pool3d_utils as rp
    real = (partA2_head.spconv, rp.RoIAwarePool3d.forward)
    partA2_head.spconv, rp.RoIAwarePool3d.forward = spconv_standin, torch_roiaware_pool
    try:
        yield
    finally:
        partA2_head.spconv, rp.RoIAwarePool3d.forward = real


ROI_CASES = {"p4": dict(pool=4, fake=False), "p6": dict(pool=6, fake=False), "fake": dict(pool=4, fake=True)}
ROI_CHANNELS = 6


def roi_scene(fake=False, seed=29, cnt=(130, 63), n=4):
    """numpy inputs of the RoI head (float64 holding float32 values where the geometry reads them): rois (2, n, 7),
    point_coords (P, 4), point_features (P, 6), point_part_offset (P, 3) in [0, 1), point_cls_scores (P), and the
    targets a training forward would have assigned.  fake: no score and no offset anywhere -> the fake branch."""
    from part_a2_scenes import scene
    rois, pts, _, part, _ = scene(seed, cnt, n, c=ROI_CHANNELS)
    rng = np.random.default_rng(seed + 1)
    p = pts.shape[0]
    feats = rng.normal(size=(p, ROI_CHANNELS))
    score = np.where(part[:, 3] > 0, rng.uniform(0, 1, p), 0.0)
    offset = part[:, :3].astype(np.float64)
    if fake:
        score, offset = score * 0, offset * 0
    rois = rois.astype(np.float64)
    b = len(cnt)
    g = np.concatenate([rng.normal(size=(b, n, 3)) * 0.2, rois[..., 3:6] * rng.uniform(0.8, 1.2, (b, n, 3)),
                        rng.uniform(-0.4, 0.4, (b, n, 1)), np.ones((b, n, 1))], -1)      # canonical frame
    src = np.concatenate([rois[..., :3] + g[..., :3], g[..., 3:6], rois[..., 6:7] + g[..., 6:7], g[..., 7:]], -1)
    targets = dict(rois=rois, gt_of_rois=g, gt_of_rois_src=src, reg_valid_mask=(rng.random((b, n)) < 0.6).astype(np.int64),
                   rcnn_cls_labels=rng.random((b, n)), roi_labels=np.ones((b, n), np.int64))
    targets["reg_valid_mask"][0, 0] = 1
    return dict(rois=rois, point_coords=pts.astype(np.float64), point_features=feats, point_part_offset=offset,
                point_cls_scores=score, targets=targets)


def run_roi_head(head, sc, to_tensor, batch_extra=None):
    """One training forward + loss + backward of a PartA2FCHead (either side) on roi_scene's inputs -> dict of numpy
    arrays: coords, part and rpn rows, rcnn_cls, rcnn_reg, the labels after the forward, the gradients."""
    del SPARSE_LOG[:]
    feats = to_tensor(sc["point_features"]).requires_grad_(True)
    offset = to_tensor(sc["point_part_offset"]).requires_grad_(True)
    batch = dict(batch_size=sc["rois"].shape[0], rois=to_tensor(sc["rois"]), point_coords=to_tensor(sc["point_coords"]),
                 point_features=feats, point_part_offset=offset, point_cls_scores=to_tensor(sc["point_cls_scores"]))
    batch.update(batch_extra or {})
    head(batch)
    ret = head.forward_ret_dict
    out = dict(coords=SPARSE_LOG[0].indices.numpy(), part_rows=SPARSE_LOG[0].features.detach().numpy(),
               rpn_rows=SPARSE_LOG[1].features.detach().numpy(), rcnn_cls=ret["rcnn_cls"].detach().numpy(),
               rcnn_reg=ret["rcnn_reg"].detach().numpy(), rcnn_cls_labels=ret["rcnn_cls_labels"].numpy(),
               reg_valid_mask=ret["reg_valid_mask"].numpy())
    return out, ret, feats, offset


def roi_grads(head, feats, offset):
    named = dict(head.named_parameters())
    zero = lambda t, like: (t if t is not None else torch.zeros_like(like)).numpy()      # noqa: E731
    return {"grad/point_features": zero(feats.grad, feats), "grad/point_part_offset": zero(offset.grad, offset),
            "grad/first_weight": zero(named["conv_part.0.0.weight"].grad, named["conv_part.0.0.weight"]).reshape(-1)[::7],
            "grad/last_weight": zero(named["reg_layers.7.weight"].grad, named["reg_layers.7.weight"]),
            "first_weight": named["conv_part.0.0.weight"].detach().numpy().reshape(-1)[::7],
            "last_weight": named["reg_layers.7.weight"].detach().numpy()}


def prepare_roi_head(head, seed):
    """BatchNorm parameters and statistics away from their defaults, the last regression weight away from ~0."""
    from pv_rcnn_ref import randomize_norms
    randomize_norms(head, seed)
    with torch.no_grad():
        head.reg_layers[-1].weight.normal_(0, 0.1, generator=torch.Generator().manual_seed(seed))
    return head
