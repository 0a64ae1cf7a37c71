from .centerpoint import CenterPoint
from .detector3d_template import Detector3DTemplate
from .part_a2_net import PartA2Net
from .point_3dssd import Point3DSSD
from .pointpillar import PointPillar
from .pv_rcnn import PVRCNN
from .second_net import SECONDNet
from .second_net_iou import SECONDNetIoU
from .voxel_rcnn import VoxelRCNN

__all__ = {
    'Detector3DTemplate': Detector3DTemplate,
    'SECONDNet': SECONDNet,
    'SECONDNetIoU': SECONDNetIoU,
    'VoxelRCNN': VoxelRCNN,
    'PVRCNN': PVRCNN,
    'PartA2Net': PartA2Net,
    '3DSSD': Point3DSSD,
    'CenterPoint': CenterPoint,
    'PointPillar': PointPillar,
}


def build_detector(model_cfg, num_class, dataset):
    return __all__[model_cfg.NAME](model_cfg=model_cfg, num_class=num_class, dataset=dataset)
