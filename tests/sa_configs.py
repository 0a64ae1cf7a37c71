"""The fast_cpc KITTI settings of the fork's voxel-point SA layers (reference tools/cfgs/kitti_models/fast_cpc.yaml,
MODEL.BACKBONE_3D and MODEL.POINT_HEAD.VSA_CONFIG), spelled out for the tests.

INSTANCES maps a name to a factory of VoxelPointnetSAModuleFSMSGDistillation keyword arguments (a factory because the
constructor edits its mlps lists in place); the channel counts are the backbone's bookkeeping for 4-channel points."""
import numpy as np

POINT_CLOUD_RANGE = [0, -40, -3, 70.4, 40, 1]
VOXEL_SIZE = [0.2, 0.2, 0.4]                    # VOXEL_SIZE [0.05, 0.05, 0.1] x FACTOR 4 (data processor repository_info)
GRID_SIZE = np.array([352, 400, 10], dtype=np.int64)


def backbone_cfg():
    """MODEL.BACKBONE_3D of fast_cpc (KITTI)."""
    from pcdet_amd.config import AttrDict
    return AttrDict({
        "NAME": "VoxelPointNet2FSMSGDistillation",
        "SA_CONFIG": {
            "NPOINT_LIST": [[4096], [512]],
            "SAMPLE_RANGE_LIST": [[[0, 20000]], [[0, 4096]]],
            "SAMPLE_METHOD_LIST": [["d-fps"], ["s-fps"]],
            "POOL_METHOD": ["max_pool", "max_pool"],
            "SPARSE_TENSOR_STRIDE": [4, 4, 4],
            "QUERY_RANGE": [[[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[2, 2, 2], [4, 4, 4], [8, 8, 8], [16, 16, 16]]],
            "STRIDE": [[[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]],
            "RADIUS": [[0.2, 0.4, 0.8], [0.4, 0.8, 1.6, 3.2]],
            "NSAMPLE": [[32, 32, 32], [32, 32, 32, 32]],
            "MLPS": [[[16, 16, 32], [16, 16, 32], [32, 32, 64]],
                     [[32, 64, 128], [32, 64, 128], [32, 64, 128], [32, 64, 128]]],
            "SPCONV_MLPS_PRE": [[0, 0, 64], [256]],
            "AGGREGATION_MLPS": [[64], [256]],
            "CONFIDENCE_MLPS": [[32], [64]],
            "WEIGHT_GAMMA": 1.0,
            "DILATED_RADIUS_GROUP": True,
        },
        "S_SA_CONFIG": {
            "NPOINT_LIST": [[4096], [512]],
            "SAMPLE_RANGE_LIST": [[[0, 20000]], [[0, 4096]]],
            "SAMPLE_METHOD_LIST": [["d-fps"], ["s-fps"]],
            "POOL_METHOD": ["max_pool", "max_pool"],
            "SPARSE_TENSOR_STRIDE": [4, 4, 4],
            "QUERY_RANGE": [[[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[16, 16, 16]]],
            "STRIDE": [[[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[1, 1, 1]]],
            "RADIUS": [[0.2, 0.4, 0.8], [3.2]],
            "NSAMPLE": [[32, 32, 32], [32]],
            "MLPS": [[[16, 16, 32], [16, 16, 32], [32, 32, 64]], [[128, 256, 512]]],
            "SPCONV_MLPS_PRE": [[0, 0, 64], [128]],
            "AGGREGATION_MLPS": [[64], [128]],
            "CONFIDENCE_MLPS": [[32], [64]],
            "WEIGHT_GAMMA": 1.0,
            "DILATED_RADIUS_GROUP": True,
        },
    })


def _grid():
    return dict(voxel_size=list(VOXEL_SIZE), grid_size=GRID_SIZE.copy(), point_cloud_range=list(POINT_CLOUD_RANGE))


def layer0():
    return dict(npoint_list=[4096], sample_range_list=[[0, 20000]], sample_method_list=["d-fps"], sp_stride=4,
                query_range=[[0, 0, 0], [0, 0, 0], [0, 0, 0]], stride=[[0, 0, 0], [0, 0, 0], [0, 0, 0]],
                radii=[0.2, 0.4, 0.8], nsamples=[32, 32, 32], mlps=[[1, 16, 16, 32], [1, 16, 16, 32], [1, 32, 32, 64]],
                spconv_mlps=[64, 0, 0, 64], pool_method="max_pool", use_xyz=True, dilated_radius_group=True,
                skip_connection=False, weight_gamma=1.0, aggregation_mlp=[64], confidence_mlp=[32], sa_layer_idx=0,
                **_grid())


def layer1():
    return dict(npoint_list=[512], sample_range_list=[[0, 4096]], sample_method_list=["s-fps"], sp_stride=4,
                query_range=[[2, 2, 2], [4, 4, 4], [8, 8, 8], [16, 16, 16]], stride=[[1, 1, 1]] * 4,
                radii=[0.4, 0.8, 1.6, 3.2], nsamples=[32, 32, 32, 32], mlps=[[64, 32, 64, 128] for _ in range(4)],
                spconv_mlps=[64, 256], pool_method="max_pool", use_xyz=True, dilated_radius_group=True,
                skip_connection=False, weight_gamma=1.0, aggregation_mlp=[256], confidence_mlp=[64], sa_layer_idx=1,
                **_grid())


def student_layer1():
    return dict(npoint_list=[512], sample_range_list=[[0, 4096]], sample_method_list=["s-fps"], sp_stride=4,
                query_range=[[16, 16, 16]], stride=[[1, 1, 1]], radii=[3.2], nsamples=[32], mlps=[[64, 128, 256, 512]],
                spconv_mlps=[64, 128], pool_method="max_pool", use_xyz=True, dilated_radius_group=True,
                skip_connection=False, weight_gamma=1.0, aggregation_mlp=[128], confidence_mlp=[64], sa_layer_idx=1,
                **_grid())


def head_vsa():
    return dict(radii=[1.6, 3.2], query_range=[[8, 8, 8], [16, 16, 16]], sp_stride=4, stride=[[1, 1, 1], [1, 1, 1]],
                nsamples=[32, 32], mlps=[[256, 128, 256, 256], [256, 128, 256, 512]], pool_method="max_pool",
                use_xyz=True, bn=True, sa_layer_idx=6, dilated_radius_group=False, voxel_size=list(VOXEL_SIZE),
                point_cloud_range=list(POINT_CLOUD_RANGE))


INSTANCES = {"backbone_sa0": layer0, "backbone_sa1": layer1, "student_sa1": student_layer1, "head_vsa": head_vsa}
