"""Target assignment of the point heads as one HIP launch per call site (spx.ops.point_assign_targets,
csrc/point_targets.hip, include/spx.h §16), with the argument and return conventions of the reference's methods:

  assign_stack_targets_mask   PointHeadVote*.assign_stack_targets_mask(set_ignore_flag=False, use_ball_constraint=True)
  assign_targets_simple       PointHeadVote*.assign_targets_simple / assign_stack_targets_simple
  sasa_assign_target          loss_utils.PointSASALoss.assign_target
  centerness_label            generate_centerness_label on the points and box labels of assign_stack_targets_mask

The reference loops over the frames and, per frame, calls points_in_boxes_gpu once or twice, indexes with boolean masks
(each reads a count back to the host), encodes the compacted rows and scatters them back.  Here the whole batch is one
launch with outputs of static shape and no host read, so a call can be captured in a graph.

Contract, checked from shapes only: `points` (B * N, 4) [bs_idx, x, y, z] holds the same number of points for every
frame, frame-major, which is what VoxelPointNet2FSMSGDistillation.forward asserts of its outputs; the bs_idx column is
not read.  There is no CPU path: CPU tensors raise spx SpxError.

Differences from the reference, all outside what its losses read (they mask with point_cls_labels > 0):
  - rows are filled for the points whose label is > 0; the reference also fills those of a hit in a box whose class
    column is <= 0 when num_class > 1 (a point at the origin inside a zero-padded gt row);
  - point_box_labels are the first 7 box columns as stored, also for gt_boxes wider than 8 columns; the reference's
    in-place size clamp of encode_torch leaks into its box labels for sizes below 1e-5;
  - the class is column 7 of gt_boxes and the box columns 0..6; the reference takes the class from the LAST column and
    the box from all columns but the last, so the two agree for 8-column gt_boxes and differ for wider
    ones.
"""
from spx import ops as spx_ops


def _frame_points(points, gt_boxes):
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError('points.shape=%s, expected (B * N, 4) [bs_idx, x, y, z]' % str(tuple(points.shape)))
    if gt_boxes.dim() != 3:
        raise ValueError('gt_boxes.shape=%s, expected (B, M, 8)' % str(tuple(gt_boxes.shape)))
    batch_size = gt_boxes.shape[0]
    if batch_size == 0 or points.shape[0] % batch_size != 0:
        raise ValueError('%d points do not make %d frames of equal size' % (points.shape[0], batch_size))
    return points[:, 1:4].reshape(batch_size, -1, 3)


def _check_coder(box_coder):
    if getattr(box_coder, 'use_mean_size', False) or getattr(box_coder, 'pred_velo', False):
        raise NotImplementedError('the fused target assignment supports PointBinResidualCoder with use_mean_size False '
                                  'and pred_velo False (the fast_cpc setting)')


def assign_stack_targets_mask(points, gt_boxes, box_coder, num_class, central_radius=2.0, with_centerness=False):
    """points (B * N, 4), gt_boxes (B, M, 8) -> point_cls_labels (B * N) long (0 background, -1 inside a box but
    outside the ball around its centre), point_reg_labels (B * N, code_size), point_box_labels (B * N, 7); with
    with_centerness also point_centerness_labels (B * N), from the same launch."""
    _check_coder(box_coder)
    xyz = _frame_points(points, gt_boxes)
    want = ('box_labels', 'reg_labels') + (('centerness',) if with_centerness else ())
    out = spx_ops.point_assign_targets(xyz, gt_boxes, spx_ops.TARGET_BALL, central_radius=central_radius,
                                       num_class=num_class, angle_bin_num=box_coder.angle_bin_num, want=want)
    targets_dict = {
        'point_cls_labels': out['cls_labels'],
        'point_reg_labels': out['reg_labels'],
        'point_box_labels': out['box_labels'],
    }
    if with_centerness:
        targets_dict['point_centerness_labels'] = out['centerness']
    return targets_dict


def assign_targets_simple(points, gt_boxes, extra_width=None, set_ignore_flag=True):
    """The vote targets: points (B * N, 4), gt_boxes (B, M, 8) -> point_cls_labels (B * N) long, point_reg_labels
    (B * N, 3) the centre of the point's box.  set_ignore_flag False: foreground (1) is inside the box grown by
    extra_width; True: foreground is inside the gt box and the grown-only ring is -1."""
    xyz = _frame_points(points, gt_boxes)
    mode = spx_ops.TARGET_IGNORE_RING if set_ignore_flag else spx_ops.TARGET_PLAIN
    out = spx_ops.point_assign_targets(xyz, gt_boxes, mode, extra_width=extra_width, num_class=1,
                                       want=('center_labels',))
    return {
        'point_cls_labels': out['cls_labels'],
        'point_reg_labels': out['center_labels'],
    }


def sasa_assign_target(points, gt_boxes, extra_width=None, set_ignore_flag=False, num_class=None):
    """The SASA layer targets: points (B * N, 4), gt_boxes (B, M, 8) -> point_cls_labels (B * N) long (0 background,
    -1 ignored), point_box_labels (B * N, 7), point_part_labels (B * N, 3) (the box centre, as in the reference).
    num_class None (PointSASALoss's default) takes the label from the class column, as any value other than 1 does."""
    xyz = _frame_points(points, gt_boxes)
    mode = spx_ops.TARGET_IGNORE_RING if set_ignore_flag else spx_ops.TARGET_PLAIN
    out = spx_ops.point_assign_targets(xyz, gt_boxes, mode, extra_width=extra_width,
                                       num_class=num_class, want=('box_labels', 'center_labels'))
    return out['cls_labels'], out['box_labels'], out['center_labels']


def centerness_label(points, gt_boxes, num_class, central_radius=2.0):
    """generate_centerness_label(point_base, point_box_labels, point_cls_labels > 0) for the point_box_labels and
    point_cls_labels that assign_stack_targets_mask gives the same points: (B * N), 0 for points that are not
    foreground."""
    xyz = _frame_points(points, gt_boxes)
    out = spx_ops.point_assign_targets(xyz, gt_boxes, spx_ops.TARGET_BALL, central_radius=central_radius,
                                       num_class=num_class, want=('centerness',))
    return out['centerness']
