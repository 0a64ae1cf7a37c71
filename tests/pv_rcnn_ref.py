"""The small PV-RCNN scene shared by tests/golden/make_golden_pv_rcnn.py (which records the reference's own modules on
it), tests/test_pv_rcnn_ref.py and tests/test_gpu_pv_rcnn.py, and the CPU stand-ins of the device ops the modules call.
Not a test module.

Two frames, NUM_KEYPOINTS 32: frame 0 holds 220 points, frame 1 holds 20, fewer than NUM_KEYPOINTS, so its picks repeat
cyclically.  A 24^3 base grid of 0.2 m voxels seen at strides 2 and 4; a 6 x 6 BEV map at stride 4; 3 GT boxes and 4 RoIs
per frame.  Every coordinate is a float32 value, so the float32 ball queries decide alike on every side."""
import contextlib
import types

import numpy as np
import torch

import pointnet2_ref
import pointnet2_stack_ref as psr
import roiaware_ref

RANGE = [0.0, -2.4, -2.4, 4.8, 2.4, 2.4]
VOXEL = [0.2, 0.2, 0.2]
NUM_KEYPOINTS = 32
POINTS_PER_FRAME = (220, 20)
STRIDES = {"x_conv3": 2, "x_conv4": 4}
CHANNELS = {"x_conv3": 4, "x_conv4": 6}
PER_FRAME = {"x_conv3": (300, 257), "x_conv4": (60, 41)}
BEV_CHANNELS, BEV_STRIDE = 5, 4
NUM_RAWPOINT_FEATURES = 4
ROI_GRAD_KEYS = ("roi_grid_pool_layer.mlps.0.0.weight", "roi_grid_pool_layer.mlps.1.3.weight",
                 "roi_grid_pool_layer.mlps.1.4.bias", "shared_fc_layer.0.weight", "cls_layers.4.weight", "reg_layers.7.bias")
YAML_KW = dict(voxel_size=[0.05, 0.05, 0.1], point_cloud_range=[0, -40, -3, 70.4, 40, 1], num_bev_features=256,
               num_rawpoint_features=4)


def pfe_cfg(num_keypoints=NUM_KEYPOINTS, **over):
    """-> a plain dict in the layout of MODEL.PFE (wrap in the config class of the side that reads it)."""
    sa = dict(raw_points=dict(MLPS=[[8, 8], [8, 8]], POOL_RADIUS=[0.5, 1.0], NSAMPLE=[16, 16]),
              x_conv3=dict(DOWNSAMPLE_FACTOR=2, MLPS=[[4, 8], [4, 8]], POOL_RADIUS=[0.6, 1.2], NSAMPLE=[16, 32]),
              x_conv4=dict(DOWNSAMPLE_FACTOR=4, MLPS=[[6, 8], [6, 8]], POOL_RADIUS=[1.2, 2.4], NSAMPLE=[16, 32]))
    cfg = dict(NAME="VoxelSetAbstraction", POINT_SOURCE="raw_points", NUM_KEYPOINTS=num_keypoints, NUM_OUTPUT_FEATURES=16,
               SAMPLE_METHOD="FPS", FEATURES_SOURCE=["bev", "x_conv3", "x_conv4", "raw_points"], SA_LAYER=sa)
    cfg.update(over)
    return cfg


def point_head_cfg():
    return dict(NAME="PointHeadSimple", CLS_FC=[16, 16], CLASS_AGNOSTIC=True, USE_POINT_FEATURES_BEFORE_FUSION=True,
                TARGET_CONFIG=dict(GT_EXTRA_WIDTH=[0.2, 0.2, 0.2]),
                LOSS_CONFIG=dict(LOSS_REG="smooth-l1", LOSS_WEIGHTS=dict(point_cls_weight=1.0)))


def roi_head_cfg(grid_size, **pool_over):
    pool = dict(GRID_SIZE=grid_size, MLPS=[[8, 8], [8, 8]], POOL_RADIUS=[0.8, 1.6], NSAMPLE=[16, 16],
                POOL_METHOD="max_pool")
    pool.update(pool_over)
    return dict(
        NAME="PVRCNNHead", CLASS_AGNOSTIC=True, SHARED_FC=[16, 16], CLS_FC=[16, 16], REG_FC=[16, 16], DP_RATIO=0.0,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=8,
                                   NMS_THRESH=0.8),
                        TEST=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=8,
                                  NMS_THRESH=0.7)),
        ROI_GRID_POOL=pool,
        TARGET_CONFIG=dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=4, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                           CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                           HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
        LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0,
                                           code_weights=[1.0] * 7)))


def scene(seed=33, points_per_frame=POINTS_PER_FRAME):
    """numpy inputs: points (N, 5) [b, x, y, z, intensity] float64 holding float32 values, frame after frame; per level
    indices (N, 4) int32 (b, z, y, x) and features (N, C); spatial_features (2, C, 6, 6); gt_boxes (2, 3, 8); rois
    (2, 4, 7) and the targets a training forward would have assigned."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    rows = []
    for b, n in enumerate(points_per_frame):
        xyz = np.stack([rng.uniform(0.3, 4.5, n), rng.uniform(-2.1, 2.1, n), rng.uniform(-2.1, 2.1, n)], 1)
        rows.append(np.concatenate([np.full((n, 1), float(b)), xyz, rng.random((n, 1))], 1))
    points = f32(np.concatenate(rows))
    levels = {}
    for name, stride in STRIDES.items():
        side = 24 // stride
        lv = []
        for b, n in enumerate(PER_FRAME[name]):
            cells = np.sort(rng.choice(side ** 3, n, replace=False))
            lv.append(np.stack([np.full(n, b), cells // (side * side), (cells // side) % side, cells % side], 1))
        idx = np.concatenate(lv).astype(np.int32)
        levels[name] = dict(indices=idx, features=rng.normal(size=(idx.shape[0], CHANNELS[name])), side=side)
    bev = rng.normal(size=(2, BEV_CHANNELS, 24 // BEV_STRIDE, 24 // BEV_STRIDE))
    gt = np.zeros((2, 3, 8))
    gt[..., 0] = rng.uniform(1.2, 3.6, (2, 3))
    gt[..., 1:3] = rng.uniform(-1.2, 1.2, (2, 3, 2))
    gt[..., 3:6] = rng.uniform(1.0, 2.2, (2, 3, 3))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, (2, 3))
    gt[..., 7] = rng.integers(1, 4, (2, 3))
    gt[1, 2] = 0                                                             # a padded row, as the collate leaves it
    gt = f32(gt)
    rois = np.zeros((2, 4, 7))
    rois[..., 0] = rng.uniform(1.2, 3.6, (2, 4))
    rois[..., 1:3] = rng.uniform(-1.2, 1.2, (2, 4, 2))
    rois[..., 3:6] = rng.uniform(0.8, 2.0, (2, 4, 3))
    rois[..., 6] = rng.uniform(-np.pi, np.pi, (2, 4))
    rois = f32(rois)
    g = np.concatenate([rng.normal(size=(2, 4, 3)) * 0.2, rois[..., 3:6] * rng.uniform(0.8, 1.2, (2, 4, 3)),
                        rng.uniform(-0.4, 0.4, (2, 4, 1)), np.ones((2, 4, 1))], -1)      # canonical frame
    src = np.concatenate([rois[..., :3] + g[..., :3], g[..., 3:6], rois[..., 6:7] + g[..., 6:7], g[..., 7:]], -1)
    targets = dict(rois=rois, gt_of_rois=g, gt_of_rois_src=src, reg_valid_mask=(rng.random((2, 4)) < 0.6).astype(np.int64),
                   rcnn_cls_labels=rng.random((2, 4)), roi_labels=np.ones((2, 4), np.int64))
    targets["reg_valid_mask"][0, 0] = 1
    return dict(points=points, levels=levels, bev=bev, gt_boxes=gt, rois=rois, targets=targets)


def sparse(level, to_tensor):
    """What the modules read of a sparse tensor."""
    return types.SimpleNamespace(indices=to_tensor(level["indices"]), features=to_tensor(level["features"]), n_valid=None,
                                 batch_size=2, spatial_shape=[level["side"]] * 3)


def batch_of(sc, to_tensor):
    return dict(batch_size=2, points=to_tensor(sc["points"]), spatial_features=to_tensor(sc["bev"]),
                spatial_features_stride=BEV_STRIDE, gt_boxes=to_tensor(sc["gt_boxes"]),
                multi_scale_3d_features={k: sparse(v, to_tensor) for k, v in sc["levels"].items()})


# ------------------------------------------------------------------------------------------- CPU stand-ins of the ops
def cpu_ball_query(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    idx, empty = psr.ball_query(xyz.detach().numpy(), xyz_batch_cnt.numpy(), new_xyz.detach().numpy(),
                                new_xyz_batch_cnt.numpy(), radius, nsample)
    return torch.from_numpy(idx), torch.from_numpy(empty)


def cpu_grouping(features, features_batch_cnt, idx, idx_batch_cnt):
    """A differentiable torch gather of the frame-local rows -> (M, C, S)."""
    offsets = torch.cumsum(features_batch_cnt, 0) - features_batch_cnt
    frame = torch.repeat_interleave(torch.arange(idx_batch_cnt.shape[0]), idx_batch_cnt.long())
    return features[idx.long() + offsets.long()[frame][:, None]].permute(0, 2, 1).contiguous()


def cpu_batch_fps(xyz, npoint):
    """(B, N, 3) -> (B, npoint) int32, the batch sampler the reference's VoxelSetAbstraction calls per frame."""
    return torch.from_numpy(pointnet2_ref.furthest_point_sample(int(npoint), xyz=xyz.detach().numpy()).astype(np.int32))


def cpu_stack_fps(xyz, xyz_batch_cnt, npoint, total=None):
    cnt = xyz_batch_cnt.numpy()
    npoint = npoint.tolist() if isinstance(npoint, torch.Tensor) else [int(npoint)] * len(cnt)
    return torch.from_numpy(psr.stack_furthest_point_sample(xyz.detach().numpy(), cnt, npoint))


def cpu_points_in_boxes(points, boxes):
    return torch.from_numpy(roiaware_ref.points_in_boxes(points.detach().numpy(), boxes.detach().numpy()))


@contextlib.contextmanager
def cpu_ops():
    """The device ops the ported modules call, replaced by the restatements for the duration."""
    from pcdet_amd.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    from pcdet_amd.ops.roiaware_pool3d import roiaware_pool3d_utils as rp
    real = (pu.ball_query, pu.grouping_operation, pu.stack_farthest_point_sample, rp.points_in_boxes_gpu)
    pu.ball_query, pu.grouping_operation = cpu_ball_query, cpu_grouping
    pu.stack_farthest_point_sample, rp.points_in_boxes_gpu = cpu_stack_fps, cpu_points_in_boxes
    try:
        yield
    finally:
        pu.ball_query, pu.grouping_operation, pu.stack_farthest_point_sample, rp.points_in_boxes_gpu = real


def randomize_norms(module, gen_seed):
    """BatchNorm weights, biases and running statistics away from their initial values, reproducibly."""
    g = torch.Generator().manual_seed(gen_seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g, dtype=torch.float64) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g, dtype=torch.float64) * 0.6 - 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g, dtype=torch.float64) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g, dtype=torch.float64) + 0.5)
