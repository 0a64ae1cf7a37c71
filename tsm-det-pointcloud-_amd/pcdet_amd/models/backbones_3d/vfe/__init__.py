from .dynamic_mean_vfe import DynamicMeanVFE
from .dynamic_pillar_vfe import DynamicPillarVFE
from .mean_vfe import MeanVFE
from .pillar_vfe import PillarVFE
from .vfe_template import VFETemplate

# DynMeanVFE / DynPillarVFE are the names of the reference's registry (pcdet/models/backbones_3d/vfe/__init__.py)
__all__ = {
    'VFETemplate': VFETemplate,
    'MeanVFE': MeanVFE,
    'DynamicMeanVFE': DynamicMeanVFE,
    'DynMeanVFE': DynamicMeanVFE,
    'PillarVFE': PillarVFE,
    'DynPillarVFE': DynamicPillarVFE,
}
