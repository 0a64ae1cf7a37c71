"""The small Voxel R-CNN head scene shared by tests/golden/make_golden_voxel_rcnn.py (which records the reference's own
head on it) and tests/test_voxel_rcnn_ref.py.  Not a test module.

Two frames; a 24^3 base grid of 0.2 m voxels seen at strides 2 / 3 / 6 (12^3, 8^3 and 4^3 cells, a few hundred voxels per
level); 8 RoIs; radii chosen so that no ball holds more than NSAMPLE voxels: the voxel query's reservoir step never runs
and the brute-force numpy query (voxel_pool_ref.voxel_query_bruteforce) gives the lists."""
import types

import numpy as np

RANGE = [0.0, -2.4, -2.4, 4.8, 2.4, 2.4]
VOXEL = [0.2, 0.2, 0.2]
STRIDES = {"x_conv2": 2, "x_conv3": 3, "x_conv4": 6}
CHANNELS = {"x_conv2": 4, "x_conv3": 6, "x_conv4": 8}
PER_FRAME = {"x_conv2": (300, 257), "x_conv3": (150, 131), "x_conv4": (30, 24)}
RADII = {"x_conv2": 0.5, "x_conv3": 0.8, "x_conv4": 1.5}
NSAMPLE = 16
YAML_CHANNELS = {'x_conv1': 16, 'x_conv2': 32, 'x_conv3': 64, 'x_conv4': 64}      # for the state_dict keys at the yaml
GRAD_KEYS = ("roi_grid_pool_layers.0.mlps_pos.0.0.weight", "roi_grid_pool_layers.1.mlps_in.0.1.weight",
             "roi_grid_pool_layers.2.mlps_pos.0.1.bias", "roi_grid_pool_layers.2.mlps_in.0.0.weight",
             "shared_fc_layer.0.weight", "cls_pred_layer.weight", "reg_pred_layer.bias")


def head_cfg(grid_size):
    """-> a plain dict in the layout of MODEL.ROI_HEAD (wrap in the config class of the side that reads it)."""
    layers = {k: dict(MLPS=[[8]], QUERY_RANGES=[[2, 2, 2]], POOL_RADIUS=[RADII[k]], NSAMPLE=[NSAMPLE],
                      POOL_METHOD="max_pool") for k in STRIDES}
    return dict(
        NAME="VoxelRCNNHead", CLASS_AGNOSTIC=True, SHARED_FC=[32, 32], CLS_FC=[32], REG_FC=[32], DP_RATIO=0.0,
        NMS_CONFIG=dict(TRAIN=dict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=64, NMS_POST_MAXSIZE=8,
                                   NMS_THRESH=0.8)),
        ROI_GRID_POOL=dict(FEATURES_SOURCE=list(STRIDES), GRID_SIZE=grid_size, POOL_LAYERS=layers),
        TARGET_CONFIG=dict(BOX_CODER="ResidualCoder", ROI_PER_IMAGE=4, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True,
                           CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1,
                           HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55),
        LOSS_CONFIG=dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="smooth-l1", CORNER_LOSS_REGULARIZATION=True,
                         LOSS_WEIGHTS=dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.0, rcnn_corner_weight=1.0,
                                           code_weights=[1.0] * 7)))


def scene():
    """numpy inputs: per level indices (N, 4) int32 (b, z, y, x) and features (N, C) float64; rois (2, 4, 7); the targets
    a training forward would have assigned."""
    rng = np.random.default_rng(21)
    levels = {}
    for name, stride in STRIDES.items():
        side = 24 // stride
        rows = []
        for b, n in enumerate(PER_FRAME[name]):
            cells = np.sort(rng.choice(side ** 3, n, replace=False))
            rows.append(np.stack([np.full(n, b), cells // (side * side), (cells // side) % side, cells % side], 1))
        idx = np.concatenate(rows).astype(np.int32)
        levels[name] = dict(indices=idx, features=rng.normal(size=(idx.shape[0], CHANNELS[name])), side=side)
    rois = np.zeros((2, 4, 7))
    rois[..., 0] = rng.uniform(1.2, 3.6, (2, 4))
    rois[..., 1:3] = rng.uniform(-1.2, 1.2, (2, 4, 2))
    rois[..., 3:6] = rng.uniform(0.8, 2.0, (2, 4, 3))
    rois[..., 6] = rng.uniform(-np.pi, np.pi, (2, 4))
    gt = np.concatenate([rng.normal(size=(2, 4, 3)) * 0.2, rois[..., 3:6] * rng.uniform(0.8, 1.2, (2, 4, 3)),
                         rng.uniform(-0.4, 0.4, (2, 4, 1)), np.ones((2, 4, 1))], -1)      # canonical frame
    src = np.concatenate([rois[..., :3] + gt[..., :3], gt[..., 3:6], rois[..., 6:7] + gt[..., 6:7], gt[..., 7:]], -1)
    targets = dict(rois=rois, gt_of_rois=gt, gt_of_rois_src=src, reg_valid_mask=(rng.random((2, 4)) < 0.6).astype(np.int64),
                   rcnn_cls_labels=rng.random((2, 4)), roi_labels=np.ones((2, 4), np.int64))
    targets["reg_valid_mask"][0, 0] = 1
    return levels, rois, targets


def sparse(level, to_tensor):
    """What the head reads of a sparse tensor."""
    return types.SimpleNamespace(indices=to_tensor(level["indices"]), features=to_tensor(level["features"]), n_valid=None,
                                 batch_size=2, spatial_shape=[level["side"]] * 3)
