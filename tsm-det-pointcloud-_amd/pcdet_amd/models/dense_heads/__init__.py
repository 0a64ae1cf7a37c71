from .anchor_head_single import AnchorHeadSingle
from .anchor_head_template import AnchorHeadTemplate
from .center_head import CenterHead
from .point_head_simple import PointHeadSimple
from .point_intra_part_head import PointIntraPartOffsetHead
from .point_head_template import PointHeadTemplate
from .point_head_vote_sasa_statistic_distillation import PointHeadVoteSASAStatisticDistillation

__all__ = {
    'AnchorHeadTemplate': AnchorHeadTemplate,
    'AnchorHeadSingle': AnchorHeadSingle,
    'CenterHead': CenterHead,
    'PointHeadTemplate': PointHeadTemplate,
    'PointHeadSimple': PointHeadSimple,
    'PointIntraPartOffsetHead': PointIntraPartOffsetHead,
    'PointHeadVoteSASAStatisticDistillation': PointHeadVoteSASAStatisticDistillation,
}
