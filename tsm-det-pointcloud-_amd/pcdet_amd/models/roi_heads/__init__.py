from .partA2_head import PartA2FCHead
from .pvrcnn_head import PVRCNNHead
from .roi_head_template import RoIHeadTemplate
from .second_head import SECONDHead
from .voxelrcnn_head import VoxelRCNNHead

__all__ = {
    'RoIHeadTemplate': RoIHeadTemplate,
    'SECONDHead': SECONDHead,
    'VoxelRCNNHead': VoxelRCNNHead,
    'PVRCNNHead': PVRCNNHead,
    'PartA2FCHead': PartA2FCHead,
}

# heads that read the keypoint features a PFE module writes (point_features, point_coords, point_cls_scores)
KEYPOINT_HEADS = {'PVRCNNHead'}
