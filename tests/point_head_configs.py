"""The fast_cpc point-head settings (reference tools/cfgs/kitti_models/fast_cpc.yaml and
waymo_models/waymo_fast_cpc.yaml, MODEL.POINT_HEAD and MODEL.POST_PROCESSING), spelled out for the tests, and a
minimal dataset stand-in so that a Point3DSSD can be built without a data pipeline."""
import types

import numpy as np

import sa_configs

CLASS_NAMES = {"kitti": ["Car", "Pedestrian", "Cyclist"], "waymo": ["Vehicle", "Pedestrian", "Cyclist"]}


def head_dict(dataset="kitti"):
    kitti = dataset == "kitti"
    vote_range = [3.0, 3.0, 2.0] if kitti else [5.0, 5.0, 3.0]
    vsa = {
        "DILATED_RADIUS_GROUP": False,
        "QUERY_RANGE": [[8, 8, 8], [16, 16, 16]],
        "SPARSE_TENSOR_STRIDE": 4,
        "STRIDE": [[1, 1, 1], [1, 1, 1]],
        "RADIUS": [1.6, 3.2],
        "NSAMPLE": [32, 32],
        "MLPS": [[128, 256, 256], [128, 256, 512]],
    }
    s_vsa = dict(vsa, NSAMPLE=[16, 16])
    return {
        "NAME": "PointHeadVoteSASAStatisticDistillation",
        "CLASS_AGNOSTIC": False,
        "USE_BN": True,
        "SAMPLE_RANGE": [0, 512] if kitti else [0, 3072],
        "VOTE_CONFIG": {"VOTE_FC": [128], "MAX_TRANSLATION_RANGE": vote_range},
        "VSA_CONFIG": vsa,
        "S_VOTE_CONFIG": {"VOTE_FC": [128], "MAX_TRANSLATION_RANGE": vote_range},
        "S_VSA_CONFIG": s_vsa,
        "S_FC_CONFIG": {"DP_RATIO": -0.3},
        "SHARED_FC": [256, 256],
        "DP_RATIO": -0.3,
        "CLS_FC": [128],
        "REG_FC": [128],
        "TARGET_CONFIG": {
            "VOTE_EXTRA_WIDTH": [0.1, 0.1, 0.1],
            "ASSIGN_METHOD": "mask",
            "GT_CENTRAL_RADIUS": 10.0,
            "BOX_CODER": "PointBinResidualCoder",
            "BOX_CODER_CONFIG": {"use_mean_size": False, "angle_bin_num": 12},
        },
        "LOSS_CONFIG": {
            "LOSS_CLS": "WeightedBinaryCrossEntropyWithCenterness",
            "LOSS_REG": "WeightedSmoothL1Loss",
            "LOSS_SASA_CONFIG": {"func": "Focal", "set_ignore_flag": True, "extra_width": [1.0, 1.0, 1.0],
                                 "layer_weights": [0.1, 0.1, 0.1], "num_class": 3},
            "AXIS_ALIGNED_IOU_LOSS_REGULARIZATION": False,
            "CORNER_LOSS_REGULARIZATION": True,
            "RDIOU_REGRESS_REGULARIZATION": True,
            "LOSS_WEIGHTS": {"vote_reg_weight": 1.0, "point_cls_weight": 1.0, "point_offset_reg_weight": 0.1,
                             "point_angle_cls_weight": 0.1, "point_angle_reg_weight": 0.1,
                             "point_similarity_weight": 0.1, "point_iou_weight": 1.0, "point_corner_weight": 1.0},
        },
    }


def post_processing_dict(dataset="kitti"):
    kitti = dataset == "kitti"
    return {
        "RECALL_THRESH_LIST": [0.3, 0.5, 0.7],
        "SCORE_THRESH": [0.62, 0.3, 0.3] if kitti else [0.01, 0.01, 0.01],
        "OUTPUT_RAW_SCORE": False,
        "EVAL_METRIC": dataset,
        "NMS_CONFIG": {"MULTI_CLASSES_NMS": False, "NMS_TYPE": "nms_gpu", "NMS_THRESH": 0.1 if kitti else 0.5,
                       "NMS_PRE_MAXSIZE": 4096 if kitti else 3072, "NMS_POST_MAXSIZE": 512 if kitti else 500},
    }


def head_cfg(dataset="kitti"):
    from pcdet_amd.config import AttrDict
    return AttrDict(head_dict(dataset))


def head_kwargs():
    """The detector's keyword arguments to the head at the KITTI voxel setting."""
    return dict(num_class=3, input_channels=256, predict_boxes_when_training=False,
                voxel_size=list(sa_configs.VOXEL_SIZE), point_cloud_range=list(sa_configs.POINT_CLOUD_RANGE))


def model_cfg():
    """MODEL of fast_cpc (KITTI)."""
    from pcdet_amd.config import AttrDict
    return AttrDict({"NAME": "3DSSD", "BACKBONE_3D": dict(sa_configs.backbone_cfg()), "POINT_HEAD": head_dict("kitti"),
                     "POST_PROCESSING": post_processing_dict("kitti")})


def dataset():
    """What Detector3DTemplate.build_networks reads from a dataset, for KITTI points (x, y, z, intensity)."""
    return types.SimpleNamespace(
        class_names=list(CLASS_NAMES["kitti"]), point_feature_encoder=types.SimpleNamespace(num_point_features=4),
        grid_size=sa_configs.GRID_SIZE.copy(), point_cloud_range=np.array(sa_configs.POINT_CLOUD_RANGE, np.float32),
        voxel_size=list(sa_configs.VOXEL_SIZE))
