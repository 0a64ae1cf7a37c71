from .voxel_set_abstraction import VoxelSetAbstraction

# point-feature encoders: a registry of their own (backbones_3d.__all__ is the sparse-voxel backbones' and is pinned)
__all__ = {
    'VoxelSetAbstraction': VoxelSetAbstraction,
}
