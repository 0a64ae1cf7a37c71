"""The losses of the fast_cpc point head (reference point_head_vote_sasa_statistic_distillation.py:570-1011:
get_vote_layer_loss, get_cls_layer_loss, get_box_layer_loss with generate_centerness_label, get_rdiou and
get_corner_loss_lidar, normalised as get_loss does), twice:

  head_loss_torch   a differentiable torch composition, any dtype and device: the eager baseline and, in float64 on the
                    CPU, what tests/golden/point_head_losses.npz (recorded from the reference) is compared with
  head_loss_fused   one libspx launch group (spx.ops.point_head_loss, csrc/point_loss.hip, include/spx.h §17) that
                    computes the three losses together with d(vote + cls + box)/d(prediction); backward scales the
                    saved gradients.  No host read, so it captures in a graph.  GPU tensors only.

Both take ret_dict with the reference's forward_ret_dict keys (rows = frame * n + point):
  s_point_vote_coords (N, 3), vote_cls_labels (N) long, vote_reg_labels (N, 3),
  s_point_cls_preds (N, C), s_point_reg_preds (N, 6 + 2K), s_point_box_preds (N, 7)           the student, with gradient
  point_cls_preds, point_reg_preds, point_box_preds                                           the teacher, constants
  s_point_cls_labels (N) long (> 0 foreground, 0 background, -1 ignored), s_point_reg_labels (N, 6 + 2K),
  s_point_box_labels (N, 7)
and return (point_loss, components) with point_loss = vote + cls + box (0-d, differentiable) and components (3) =
(vote, cls, box) detached.

Where the gradients come from: vote_coords from the vote loss only (generate_centerness_label is no_grad); cls_preds from
the cls loss; reg_preds from the box loss; box_preds from the RDIoU and corner terms of the box loss AND from the cls
loss, whose soft target (centerness * rdiou + 1e-8) ** 0.25 is built from get_rdiou(box_preds, box_labels) with autograd
on: d BCE / d target = -logit / C on the positive's class column.
"""
import math

import torch
import torch.nn.functional as F

from ...utils import box_coder_utils, loss_utils

# the order of include/spx.h §17; point_similarity_weight belongs to get_similarity_loss, which get_loss does not call
LOSS_WEIGHT_KEYS = ('vote_reg_weight', 'point_cls_weight', 'point_offset_reg_weight', 'point_angle_cls_weight',
                    'point_angle_reg_weight', 'point_similarity_weight', 'point_iou_weight', 'point_corner_weight')
_CORNER_SIGNS = ((1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1))


def centerness_label(point_base, boxes, epsilon=1e-6):
    """generate_centerness_label on rows: point_base (R, 3), boxes (R, 7) -> (R), without gradient."""
    with torch.no_grad():
        c = point_base - boxes[:, 0:3]
        ca, sa = torch.cos(-boxes[:, 6]), torch.sin(-boxes[:, 6])
        local = (c[:, 0] * ca - c[:, 1] * sa, c[:, 0] * sa + c[:, 1] * ca, c[:, 2])
        prod = None
        for k in range(3):
            lo, hi = boxes[:, 3 + k] / 2 - local[k], boxes[:, 3 + k] / 2 + local[k]
            ratio = torch.min(lo, hi) / torch.max(lo, hi)
            prod = ratio if prod is None else prod * ratio
        return torch.clamp(prod, min=epsilon) ** (1 / 3.0)


def rdiou(b1, b2):
    """get_rdiou's second result on rows: b1, b2 (R, 7) -> (R): the 4-D overlap over union of the boxes taken as
    axis-aligned in (x, y, z, t), t1 = sin(r1) cos(r2), t2 = cos(r1) sin(r2) with unit extent, b1's sizes clamped to 10."""
    t1 = torch.sin(b1[:, 6]) * torch.cos(b2[:, 6])
    t2 = torch.cos(b1[:, 6]) * torch.sin(b2[:, 6])
    s1 = torch.clamp(b1[:, 3:6], max=10)
    s2 = b2[:, 3:6]
    one = torch.ones_like(t1)
    dims = [(b1[:, k], s1[:, k], b2[:, k], s2[:, k]) for k in range(3)] + [(t1, one, t2, one)]
    inter = None
    for p1, e1, p2, e2 in dims:
        lo = torch.max(p1 - e1 / 2, p2 - e2 / 2)
        hi = torch.min(p1 + e1 / 2, p2 + e2 / 2)
        edge = torch.clamp(hi - lo, min=0)
        inter = edge if inter is None else inter * edge
    union = s1[:, 0] * s1[:, 1] * s1[:, 2] + s2[:, 0] * s2[:, 1] * s2[:, 2] - inter
    return inter / union


def box_corners(boxes):
    """(R, 7) -> (R, 8, 3), the corner order of box_utils.boxes_to_corners_3d, in the dtype of `boxes` with gradient."""
    signs = boxes.new_tensor(_CORNER_SIGNS) / 2
    local = boxes[:, None, 3:6] * signs[None]
    cos, sin = torch.cos(boxes[:, 6])[:, None], torch.sin(boxes[:, 6])[:, None]
    x = local[..., 0] * cos - local[..., 1] * sin
    y = local[..., 0] * sin + local[..., 1] * cos
    return torch.stack([x, y, local[..., 2]], dim=-1) + boxes[:, None, 0:3]


def corner_loss(pred, gt):
    """get_corner_loss_lidar: pred, gt (R, 7) -> (R): smooth L1 (beta 1) of the corner distances, summed per corner, the
    smaller of gt and gt turned by pi, mean over the corners."""
    flip = torch.cat([gt[:, :6], gt[:, 6:7] + math.pi], dim=1)
    pc = box_corners(pred)
    sl1 = loss_utils.WeightedSmoothL1Loss.smooth_l1_loss
    a = sl1(pc - box_corners(gt), 1.0).sum(dim=2)
    b = sl1(pc - box_corners(flip), 1.0).sum(dim=2)
    return torch.min(a, b).mean(dim=1)


def axis_aligned_iou_loss(pred, gt):
    """get_axis_aligned_iou_loss_lidar: pred, gt (R, 7) -> (R)."""
    len_p, len_g = torch.clamp(pred[:, 3:6], min=1e-5), torch.clamp(gt[:, 3:6], min=1e-5)
    min_p, max_p = pred[:, 0:3] - len_p / 2, pred[:, 0:3] + len_p / 2
    min_g, max_g = gt[:, 0:3] - len_g / 2, gt[:, 0:3] + len_g / 2
    inter = torch.clamp(torch.min(max_p, max_g) - torch.max(min_p, min_g), min=0).prod(dim=-1)
    union = len_p.prod(dim=-1) + len_g.prod(dim=-1) - inter
    return 1 - inter / torch.clamp(union, min=1e-5)


def _centerness_range(loss_cfg):
    cfg = loss_cfg.get('LOSS_CLS_CONFIG', None)
    if cfg is None:
        return 0.0, 1.0
    return float(cfg['centerness_min']), float(cfg['centerness_max'])


def _scatter_rows(mask, values, like):
    """values (R) of the rows where mask holds -> (N), zero elsewhere (the reference's x[mask] = x[mask] + values)."""
    return torch.zeros_like(like).masked_scatter(mask, values)


def head_loss_torch(ret_dict, model_cfg, box_coder, reg_loss_func, cls_loss_func):
    loss_cfg = model_cfg.LOSS_CONFIG
    w = loss_cfg.LOSS_WEIGHTS
    if not isinstance(box_coder, box_coder_utils.PointBinResidualCoder):
        raise NotImplementedError('the point-head losses are ported for PointBinResidualCoder (the fast_cpc setting)')
    bins = box_coder.angle_bin_num

    # ---- vote regression on the vote positives
    vote_pos = ret_dict['vote_cls_labels'] > 0
    vote_w = vote_pos.to(ret_dict['s_point_vote_coords'].dtype)
    vote_w = vote_w / torch.clamp(vote_w.sum(), min=1.0)
    loss_vote = reg_loss_func(ret_dict['s_point_vote_coords'][None], ret_dict['vote_reg_labels'][None],
                              weights=vote_w[None]).sum() * w['vote_reg_weight']

    # ---- classification against the (soft) one-hot target, and against the teacher at temperature 3
    labels = ret_dict['s_point_cls_labels'].view(-1)
    cls_preds = ret_dict['s_point_cls_preds']
    num_class = cls_preds.shape[-1]
    cls_preds = cls_preds.view(-1, num_class)
    t_cls_preds = ret_dict['point_cls_preds'].view(-1, num_class)
    pos = labels > 0
    cls_w = (labels >= 0).to(cls_preds.dtype)
    one_hot = cls_preds.new_zeros(labels.shape[0], num_class + 1)
    one_hot.scatter_(-1, (labels * (labels >= 0).long()).unsqueeze(-1), 1.0)
    vote_coords = ret_dict['s_point_vote_coords']
    box_preds, box_labels = ret_dict['s_point_box_preds'], ret_dict['s_point_box_labels']
    t_box_preds = ret_dict['point_box_preds']
    pos_base, pos_box, pos_lab, pos_tbox = vote_coords[pos], box_preds[pos, :7], box_labels[pos, :7], t_box_preds[pos, :7]
    if 'WithCenterness' in loss_cfg.LOSS_CLS:
        soft = torch.pow(centerness_label(pos_base, pos_lab) * rdiou(pos_box, pos_lab) + 1e-8, 0.25)
        cmin, cmax = _centerness_range(loss_cfg)
        one_hot = one_hot * (cmin + (cmax - cmin) * _scatter_rows(pos, soft, cls_w)).unsqueeze(-1)
    loss_cls = cls_loss_func(cls_preds, one_hot[..., 1:], weights=cls_w)
    t_loss_cls = cls_loss_func(cls_preds / 3, (t_cls_preds / 3).sigmoid(), weights=cls_w)
    loss_cls = (loss_cls * 0.5 + t_loss_cls * 0.5) * w['point_cls_weight']
    loss_cls = loss_cls.sum() / torch.clamp(cls_w.sum(), min=1.0)

    # ---- box: offsets against labels and teacher, angle bin, bin residual, then RDIoU / IoU / corners on the positives
    reg_preds, reg_labels = ret_dict['s_point_reg_preds'], ret_dict['s_point_reg_labels']
    t_reg_preds = ret_dict['point_reg_preds']
    reg_w = pos.to(reg_preds.dtype)
    offset = reg_loss_func(reg_preds[None, :, :6], reg_labels[None, :, :6], weights=reg_w[None]).sum(dim=-1).squeeze(0)
    t_offset = reg_loss_func(reg_preds[None, :, :6], t_reg_preds[None, :, :6], weights=reg_w[None]).sum(dim=-1).squeeze(0)
    offset = 0.5 * offset + 0.5 * t_offset
    if getattr(box_coder, 'pred_velo', False):
        lo = 6 + 2 * bins
        offset = offset + reg_loss_func(reg_preds[None, :, lo:lo + 2], reg_labels[None, :, lo:lo + 2],
                                        weights=reg_w[None]).sum(dim=-1).squeeze(0)
    bin_labels = reg_labels[:, 6:6 + bins]
    angle_cls = F.cross_entropy(reg_preds[:, 6:6 + bins], bin_labels.argmax(dim=-1), reduction='none') * reg_w
    res_pred = (reg_preds[:, 6 + bins:6 + 2 * bins] * bin_labels).sum(dim=-1, keepdim=True)
    res_label = (reg_labels[:, 6 + bins:6 + 2 * bins] * bin_labels).sum(dim=-1, keepdim=True)
    angle_reg = reg_loss_func(res_pred[None], res_label[None], weights=reg_w[None]).view(-1)
    loss_box = offset * w['point_offset_reg_weight'] + angle_cls * w['point_angle_cls_weight'] \
        + angle_reg * w['point_angle_reg_weight']
    aux = pos_box.new_zeros(pos_box.shape[0])
    if loss_cfg.get('RDIOU_REGRESS_REGULARIZATION', False):
        q = torch.pow(rdiou(pos_box, pos_lab) * centerness_label(pos_base, pos_lab) + 1e-8, 0.25)
        t_q = torch.pow(rdiou(pos_box, pos_tbox) * centerness_label(pos_base, pos_tbox) + 1e-8, 0.25)
        aux = aux + (0.5 * (1 - q) + (1 - t_q) * 0.5) * w['point_iou_weight']
    if loss_cfg.get('AXIS_ALIGNED_IOU_LOSS_REGULARIZATION', False):
        aux = aux + axis_aligned_iou_loss(pos_box, pos_lab) * w['point_iou_weight']
    if loss_cfg.get('CORNER_LOSS_REGULARIZATION', False):
        aux = aux + corner_loss(pos_box, pos_lab) * w['point_corner_weight'] * 0.3
        aux = aux + corner_loss(pos_box, pos_tbox) * w['point_corner_weight'] * 0.7
    loss_box = loss_box + _scatter_rows(pos, aux, loss_box)
    loss_box = loss_box.sum() / torch.clamp(reg_w.sum(), min=1.0)

    components = torch.stack([loss_vote, loss_cls, loss_box])
    return loss_vote + loss_cls + loss_box, components.detach()


class _FusedPointHeadLoss(torch.autograd.Function):
    """total = vote + cls + box; the launch group also leaves d(total)/d(vote_coords, cls_preds, reg_preds, box_preds),
    which backward scales by the incoming scalar.  The components go out as a second, non-differentiable output."""

    @staticmethod
    def forward(ctx, vote_coords, cls_preds, reg_preds, box_preds, consts, settings):
        from spx import ops
        losses, d_vote, d_cls, d_reg, d_box = ops.point_head_loss(vote_coords, cls_preds, reg_preds, box_preds,
                                                                  *consts, **settings)
        ctx.save_for_backward(d_vote, d_cls, d_reg, d_box)
        ctx.shapes = (vote_coords.shape, cls_preds.shape, reg_preds.shape, box_preds.shape)
        ctx.mark_non_differentiable(losses)
        return losses.sum(), losses

    @staticmethod
    def backward(ctx, g, _g_components):
        return tuple((d * g).view(s) for d, s in zip(ctx.saved_tensors, ctx.shapes)) + (None, None)


def fused_settings(model_cfg, box_coder, reg_loss_func, cls_loss_func):
    """The keyword arguments of spx.ops.point_head_loss for this head, or NotImplementedError naming the setting the
    kernel does not cover."""
    loss_cfg = model_cfg.LOSS_CONFIG
    if loss_cfg.get('AXIS_ALIGNED_IOU_LOSS_REGULARIZATION', False):
        raise NotImplementedError('fused point-head loss: AXIS_ALIGNED_IOU_LOSS_REGULARIZATION is not covered')
    if not isinstance(box_coder, box_coder_utils.PointBinResidualCoder):
        raise NotImplementedError('fused point-head loss: BOX_CODER must be PointBinResidualCoder')
    if getattr(box_coder, 'pred_velo', False):
        raise NotImplementedError('fused point-head loss: pred_velo is not covered')
    if getattr(box_coder, 'use_mean_size', False):
        raise NotImplementedError('fused point-head loss: use_mean_size is not covered')
    if not isinstance(cls_loss_func, loss_utils.WeightedBinaryCrossEntropyLoss):
        raise NotImplementedError('fused point-head loss: LOSS_CLS %s is not covered (WeightedBinaryCrossEntropy[With'
                                  'Centerness] is)' % loss_cfg.LOSS_CLS)
    if not isinstance(reg_loss_func, loss_utils.WeightedSmoothL1Loss):
        raise NotImplementedError('fused point-head loss: LOSS_REG must be WeightedSmoothL1Loss')
    if reg_loss_func.code_weights is not None:
        raise NotImplementedError('fused point-head loss: code_weights are not covered')
    cmin, cmax = _centerness_range(loss_cfg)
    w = loss_cfg.LOSS_WEIGHTS
    return dict(loss_weights=[float(w.get(k, 0.0)) for k in LOSS_WEIGHT_KEYS], beta=float(reg_loss_func.beta),
                centerness_min=cmin, centerness_max=cmax, with_centerness='WithCenterness' in loss_cfg.LOSS_CLS,
                rdiou=bool(loss_cfg.get('RDIOU_REGRESS_REGULARIZATION', False)),
                corner=bool(loss_cfg.get('CORNER_LOSS_REGULARIZATION', False)))


def head_loss_fused(ret_dict, model_cfg, box_coder, reg_loss_func, cls_loss_func):
    settings = fused_settings(model_cfg, box_coder, reg_loss_func, cls_loss_func)
    num_class = ret_dict['s_point_cls_preds'].shape[-1]
    consts = (ret_dict['point_cls_preds'].view(-1, num_class), ret_dict['point_reg_preds'], ret_dict['point_box_preds'],
              ret_dict['vote_cls_labels'], ret_dict['vote_reg_labels'], ret_dict['s_point_cls_labels'].view(-1),
              ret_dict['s_point_reg_labels'], ret_dict['s_point_box_labels'])
    total, components = _FusedPointHeadLoss.apply(
        ret_dict['s_point_vote_coords'], ret_dict['s_point_cls_preds'].view(-1, num_class),
        ret_dict['s_point_reg_preds'], ret_dict['s_point_box_preds'], consts, settings)
    return total, components
