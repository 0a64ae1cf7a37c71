"""Constructor arguments of the stacked set-abstraction modules as the tests build them (a helper, not a test file):
small instances in the shape of the upstream PV-RCNN keypoint layers and of the fork's VoxelPointCross neck.  Every
entry is a function returning fresh keyword arguments, because the constructors edit their `mlps` lists in place."""

INSTANCES = {
    # StackSAModuleMSG over raw points (1 feature channel) and over a voxel level (32 channels)
    "sa_raw": lambda: dict(radii=[0.4, 0.8], nsamples=[16, 16], mlps=[[1, 16, 16], [1, 16, 16]], use_xyz=True,
                           pool_method="max_pool"),
    "sa_conv3": lambda: dict(radii=[1.2, 2.4], nsamples=[16, 32], mlps=[[32, 32, 32], [32, 32, 48]], use_xyz=True,
                             pool_method="avg_pool"),
    # StackPointnetFPModule from keypoints back to raw points
    "fp": lambda: dict(mlp=[32 + 4, 32, 16]),
    # NeighborVoxelSAModuleMSG, the three pool methods
    "neighbor_max": lambda: dict(query_ranges=[[2, 2, 2], [3, 3, 3]], radii=[0.8, 1.6], nsamples=[8, 16],
                                 mlps=[[16, 16], [16, 32]], pool_method="max_pool"),
    "neighbor_avg": lambda: dict(query_ranges=[[2, 2, 2]], radii=[0.8], nsamples=[8], mlps=[[16, 24]],
                                 pool_method="avg_pool"),
    "neighbor_ws": lambda: dict(query_ranges=[[2, 2, 2]], radii=[0.8], nsamples=[8], mlps=[[16, 16]],
                                pool_method="weight_sum"),
}

CLASS_OF = {"sa_raw": "StackSAModuleMSG", "sa_conv3": "StackSAModuleMSG", "fp": "StackPointnetFPModule",
            "neighbor_max": "NeighborVoxelSAModuleMSG", "neighbor_avg": "NeighborVoxelSAModuleMSG",
            "neighbor_ws": "NeighborVoxelSAModuleMSG"}
