"""ProposalTargetLayer (reference pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:8-228): per frame,
match every RoI to a ground-truth box by 3-D IoU, sample ROI_PER_IMAGE of them as fg / hard bg / easy bg, and label them.

The reference loops over frames (and classes), reads counts back with nonzero / numel / item and draws from numpy and
CPU torch inside the step.  Here the random numbers are two tensors drawn up front -- fg_keys (B, R), whose argsort is
the reference's np.random.permutation, and slot_u (B, M), the uniforms behind its np.random.rand and torch.randint -- and
the matching and sampling of the whole batch is spx.ops.proposal_sample (csrc/proposal_targets.hip, spx.h §26): two
launches, no host read, capturable.  `_sample_torch` composes the same rules from torch ops; it runs on CPU tensors and
with TARGET_CONFIG.FUSED: False.  The gathers and labels after the sampling are batched torch in both cases."""
import numpy as np
import torch
import torch.nn as nn

from ....ops.iou3d_nms import iou3d_nms_utils


class ProposalTargetLayer(nn.Module):
    def __init__(self, roi_sampler_cfg):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg

    # a float64 IoU for CPU tensors is injected by the tests (there is no CPU kernel); GPU tensors use libspx
    iou3d_fn = staticmethod(iou3d_nms_utils.boxes_iou3d_gpu)

    def forward(self, batch_dict):
        """batch_dict: batch_size, rois (B, R, 7 + C), roi_scores (B, R), roi_labels (B, R), gt_boxes (B, G, 7 + C + 1),
        optionally roi_sampler_rand = (fg_keys (B, R), slot_u (B, M)).  Returns the reference's targets_dict: rois,
        gt_of_rois, gt_iou_of_rois, roi_scores, roi_labels, reg_valid_mask, rcnn_cls_labels."""
        cfg = self.roi_sampler_cfg
        rois, roi_scores, roi_labels = batch_dict['rois'], batch_dict['roi_scores'], batch_dict['roi_labels']
        gt_boxes = batch_dict['gt_boxes']
        b, r = rois.shape[0], rois.shape[1]
        m = int(cfg.ROI_PER_IMAGE)
        rand = batch_dict.get('roi_sampler_rand', None)
        if rand is None:
            fg_keys = torch.rand((b, r), device=rois.device, dtype=torch.float32)
            slot_u = torch.rand((b, m), device=rois.device, dtype=torch.float32)
        else:
            fg_keys, slot_u = rand
        if gt_boxes.shape[1] == 0:                          # the reference samples against one all-zero row
            gt_boxes = gt_boxes.new_zeros((b, 1, gt_boxes.shape[2]))
        sampled, ious, gt_inds = self.sample_rois_for_rcnn(rois, roi_labels, gt_boxes, fg_keys, slot_u)

        def take(t, idx):
            return torch.gather(t, 1, idx.view(b, m, *([1] * (t.dim() - 2))).expand(b, m, *t.shape[2:]))

        batch_rois, batch_gt_of_rois = take(rois, sampled), take(gt_boxes, gt_inds)
        batch_roi_scores, batch_roi_labels = take(roi_scores, sampled), take(roi_labels, sampled)
        batch_roi_ious = ious.to(rois.dtype)

        reg_valid_mask = (batch_roi_ious > cfg.REG_FG_THRESH).long()
        if cfg.CLS_SCORE_TYPE == 'cls':
            batch_cls_labels = (batch_roi_ious > cfg.CLS_FG_THRESH).long()
            ignore_mask = (batch_roi_ious > cfg.CLS_BG_THRESH) & (batch_roi_ious < cfg.CLS_FG_THRESH)
            batch_cls_labels = torch.where(ignore_mask, torch.full_like(batch_cls_labels, -1), batch_cls_labels)
        elif cfg.CLS_SCORE_TYPE == 'roi_iou':
            iou_bg_thresh, iou_fg_thresh = cfg.CLS_BG_THRESH, cfg.CLS_FG_THRESH
            fg_mask = batch_roi_ious > iou_fg_thresh
            bg_mask = batch_roi_ious < iou_bg_thresh
            interval_mask = (fg_mask == 0) & (bg_mask == 0)
            batch_cls_labels = torch.where(interval_mask,
                                           (batch_roi_ious - iou_bg_thresh) / (iou_fg_thresh - iou_bg_thresh),
                                           (fg_mask > 0).to(batch_roi_ious.dtype))
        else:
            raise NotImplementedError('CLS_SCORE_TYPE %s' % cfg.CLS_SCORE_TYPE)
        return {'rois': batch_rois, 'gt_of_rois': batch_gt_of_rois, 'gt_iou_of_rois': batch_roi_ious,
                'roi_scores': batch_roi_scores, 'roi_labels': batch_roi_labels, 'reg_valid_mask': reg_valid_mask,
                'rcnn_cls_labels': batch_cls_labels}

    def sample_rois_for_rcnn(self, rois, roi_labels, gt_boxes, fg_keys, slot_u):
        """-> sampled_inds (B, M) int64, roi_ious (B, M), gt_inds (B, M) int64."""
        cfg = self.roi_sampler_cfg
        m = int(cfg.ROI_PER_IMAGE)
        fg_per_image = int(np.round(cfg.FG_RATIO * m))
        by_class = bool(cfg.get('SAMPLE_ROI_BY_EACH_CLASS', False))
        if rois.is_cuda and cfg.get('FUSED', True):
            from spx import ops
            return ops.proposal_sample(rois, roi_labels, gt_boxes, m, fg_per_image, cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH,
                                       cfg.CLS_BG_THRESH_LO, cfg.HARD_BG_RATIO, by_class, fg_keys, slot_u)
        out = [self._sample_torch(rois[i], roi_labels[i], gt_boxes[i], fg_keys[i], slot_u[i], m, fg_per_image, by_class)
               for i in range(rois.shape[0])]
        return tuple(torch.stack([o[j] for o in out]) for j in range(3))

    def _sample_torch(self, rois, roi_labels, gt, fg_keys, slot_u, m, fg_per_image, by_class):
        """One frame of the rules of include/spx.h §26 from torch ops (host reads included: this is the comparison path)."""
        cfg = self.roi_sampler_cfg
        nz = (gt.sum(dim=1) != 0).nonzero().view(-1)
        k = int(nz.max()) if nz.numel() else 0              # trailing zero rows go, row 0 and interior zero rows stay
        gt = gt[:k + 1]
        iou = self.iou3d_fn(rois[:, 0:7], gt[:, 0:7])        # (R, k + 1)
        if by_class:
            same = roi_labels.view(-1, 1) == gt[:, -1].long().view(1, -1)
            has = same.any(dim=1)
            masked = torch.where(same, iou, torch.full_like(iou, -1.0))
            max_overlaps, gt_assignment = self._first_max(masked)
            max_overlaps = torch.where(has, max_overlaps, torch.zeros_like(max_overlaps))
            gt_assignment = torch.where(has, gt_assignment, torch.zeros_like(gt_assignment))
        else:
            max_overlaps, gt_assignment = self._first_max(iou)
        fg_thresh = min(cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH)
        fg_inds = (max_overlaps >= fg_thresh).nonzero().view(-1)
        easy = (max_overlaps < cfg.CLS_BG_THRESH_LO).nonzero().view(-1)
        hard = ((max_overlaps < cfg.REG_FG_THRESH) & (max_overlaps >= cfg.CLS_BG_THRESH_LO)).nonzero().view(-1)
        n_fg, n_hard, n_easy = fg_inds.numel(), hard.numel(), easy.numel()

        def draw(lst, lo, hi):
            n = lst.numel()
            q = torch.floor(slot_u[lo:hi].double() * n).long().clamp(0, n - 1)
            return lst[q]

        if n_fg > 0 and n_hard + n_easy == 0:
            picked = draw(fg_inds, 0, m)
        else:
            n_take = min(fg_per_image, n_fg)
            if n_take:
                keys = fg_keys[fg_inds]
                order = torch.argsort(keys, stable=True)         # ascending (key, RoI index): fg_inds is ascending
                parts = [fg_inds[order[:n_take]]]
            else:
                parts = []
            bg = m - n_take
            if n_hard > 0 and n_easy > 0:
                n_hs = min(int(bg * cfg.HARD_BG_RATIO), n_hard)
            else:
                n_hs = bg if n_hard > 0 else 0
            if n_hs:
                parts.append(draw(hard, n_take, n_take + n_hs))
            if bg - n_hs:
                parts.append(draw(easy, n_take + n_hs, m))
            picked = torch.cat(parts)
        return picked, max_overlaps[picked], gt_assignment[picked]

    @staticmethod
    def _first_max(x):
        """Row maximum and the LOWEST column that attains it (torch.max leaves the choice among ties open)."""
        best = x.max(dim=1)[0]
        cols = torch.arange(x.shape[1], device=x.device).view(1, -1).expand_as(x)
        arg = torch.where(x == best.view(-1, 1), cols, torch.full_like(cols, x.shape[1])).min(dim=1)[0]
        return best, arg
