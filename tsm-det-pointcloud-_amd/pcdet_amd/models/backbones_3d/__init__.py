from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x
from .pointnet2_backbone import VoxelPointNet2FSMSGDistillation
from .spconv_unet import UNetV2

__all__ = {
    'VoxelBackBone8x': VoxelBackBone8x,
    'VoxelResBackBone8x': VoxelResBackBone8x,
    'UNetV2': UNetV2,
}

# point-based backbones (the fork's fast_cpc); kept apart from the sparse-voxel registry above, whose set is pinned
POINT_BACKBONES = {
    'VoxelPointNet2FSMSGDistillation': VoxelPointNet2FSMSGDistillation,
}


def get_backbone_3d(name):
    """The 3-D backbone class registered under `name` in either registry."""
    return __all__[name] if name in __all__ else POINT_BACKBONES[name]
