"""Generate tests/golden/anchor_head_edges.npz from the REFERENCE's anchor target assigner and anchor-head losses
(build container only; the reference is imported exactly as make_golden_ref.py imports it).

Recorded for the cases that tests/anchor_head_ref.py defines (the inputs are rebuilt from there, only settings and
outputs are stored):
  assignment  AxisAlignedTargetAssigner.assign_targets on the 32 x 40 head for the five-frame edge batch, and on every
              synthetic anchor set: labels and weights as int8, the regression targets of the positive anchors only;
  losses      SigmoidFocalClassificationLoss, WeightedSmoothL1Loss after add_sin_difference, WeightedCrossEntropyLoss
              on get_direction_target, in float64: the three weighted losses of every case and, for the small cases, the
              gradients of their sum.  For the cases on a bin boundary the float32 direction bins (which then also
              select the float64 cross-entropy target).  A NaN heading target makes the reference's own loss NaN
              (recorded as nan_heading_reference_is_nan); the stored values of those cases take the heading target
              from the prediction, the rule its WeightedSmoothL1Loss applies to every other column.
Only DATA is written.  The archive is written with fixed time stamps, so a second run reproduces it bit for bit.

Run:  python tests/golden/make_golden_anchor_head.py
"""
import importlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_ref import import_reference, small_head_cfg  # noqa: E402

import anchor_head_ref as ahr  # noqa: E402


def record_assignment(prefix, out, result):
    labels = result["box_cls_labels"].numpy()
    weights = result["reg_weights"].numpy()
    assert np.abs(labels).max() < 127 and set(np.unique(weights)) <= {0.0, 1.0}
    out[prefix + "_labels"] = labels.astype(np.int8)
    out[prefix + "_weights"] = weights.astype(np.int8)
    out[prefix + "_pos_targets"] = result["box_reg_targets"].numpy()[labels > 0].astype(np.float32)


def reference_losses(ref, c, name):
    """float64 run of the reference's loss modules on a loss case -> dict of arrays to store."""
    loss, template = ref["loss"], ref["head"].AnchorHeadSingle
    t64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    cls, box = t64(c["cls"]).requires_grad_(True), t64(c["box"]).requires_grad_(True)
    dirp = None if c["dir"] is None else t64(c["dir"]).requires_grad_(True)
    labels, targets, anchors = torch.from_numpy(c["labels"]), t64(c["targets"]), t64(c["anchors"])
    B, A, NC = cls.shape
    out = {}
    positives = labels > 0
    pos_norm = torch.clamp(positives.sum(1, keepdim=True).double(), min=1.0)
    cls_weights = (labels >= 0).double() / pos_norm
    one_hot = torch.zeros(B, A, NC + 1, dtype=torch.float64)
    one_hot.scatter_(-1, (labels * (labels >= 0)).long().unsqueeze(-1), 1.0)
    cw, lw, dw = c["weights"]
    l_cls = loss.SigmoidFocalClassificationLoss(alpha=c["alpha"], gamma=2.0)(cls, one_hot[..., 1:],
                                                                             weights=cls_weights).sum() / B * cw
    smooth = loss.WeightedSmoothL1Loss(beta=c["beta"], code_weights=None)
    reg_weights = positives.double() / pos_norm
    nan_heading = torch.isnan(targets[..., 6])
    if bool(nan_heading.any()):
        s, t = template.add_sin_difference(box, targets)
        out["nan_heading_reference_is_nan"] = np.array(bool(torch.isnan(smooth(s, t, weights=reg_weights).sum())))
        targets = targets.clone()
        targets[..., 6] = torch.where(nan_heading, box.detach()[..., 6], targets[..., 6])
    s, t = template.add_sin_difference(box, targets)
    l_loc = smooth(s, t, weights=reg_weights).sum() / B * lw
    total, l_dir = l_cls + l_loc, torch.zeros((), dtype=torch.float64)
    leaves = [cls, box]
    if dirp is not None:
        nb = c["num_dir_bins"]
        kw = dict(dir_offset=c["dir_offset"], num_bins=nb)
        batch_anchors = anchors[None].repeat(B, 1, 1)
        dir_targets = template.get_direction_target(batch_anchors, targets, **kw)
        if name.startswith("boundary"):
            bins32 = template.get_direction_target(batch_anchors.float(), targets.float(), one_hot=False, **kw)
            out["bins32"] = bins32.numpy().astype(np.int8)
            dir_targets = torch.nn.functional.one_hot(bins32, nb).double()
        l_dir = loss.WeightedCrossEntropyLoss()(dirp, dir_targets, weights=reg_weights).sum() / B * dw
        total = total + l_dir
        leaves.append(dirp)
    out["losses"] = np.array([float(v.detach()) for v in (l_cls, l_loc, l_dir)])
    if B * A <= ahr.GOLDEN_GRAD_ROWS:
        for key, g in zip(("dcls", "dbox", "ddir"), torch.autograd.grad(total, leaves)):
            out[key] = g.numpy()
    return out


def save_reproducibly(path, arrays):
    """An .npz (deflated zip of .npy members) with fixed member order and time stamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref = import_reference()
    from pcdet_amd.config import AttrDict
    assigner_mod = importlib.import_module("pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner")
    out = {}

    # ---- assignment on the fixture head
    g = ahr.modules()
    head = ref["head"].AnchorHeadSingle(model_cfg=small_head_cfg().MODEL.DENSE_HEAD, input_channels=16, num_class=3,
                                        class_names=list(ahr.CLASS_NAMES), grid_size=g["head_grid_size"],
                                        point_cloud_range=g["head_pc_range"], predict_boxes_when_training=True)
    for i, a in enumerate(head.anchors):
        assert np.array_equal(a.numpy(), g["anchors_%d" % i])
    record_assignment("fixture", out, head.assign_targets(torch.from_numpy(ahr.fixture_edge_batch())))

    # ---- assignment on the synthetic anchor sets
    coder = ref["box_coder"].ResidualCoder()
    for name in ahr.SYNTH_CASES:
        c = ahr.synth_case(name)
        cfg = AttrDict(ANCHOR_GENERATOR_CONFIG=[{"class_name": n, "matched_threshold": m, "unmatched_threshold": u}
                                                for n, m, u in zip(c["set_names"], c["matched"], c["unmatched"])],
                       TARGET_ASSIGNER_CONFIG=AttrDict(POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False))
        assigner = assigner_mod.AxisAlignedTargetAssigner(cfg, list(c["class_names"]), coder, match_height=False)
        anchors = [torch.from_numpy(a.copy())[None, None, :, None] for a in c["anchor_sets"]]   # [1, 1, L, 1, P, 7]
        record_assignment("synth_" + name, out, assigner.assign_targets(anchors, torch.from_numpy(c["gt"].copy())))

    # ---- losses
    for name in ahr.LOSS_CASES:
        for key, value in reference_losses(ref, ahr.loss_case(name), name).items():
            out[key if key.startswith("nan_heading_reference") else "loss_%s_%s" % (name, key)] = value

    path = os.path.join(HERE, "anchor_head_edges.npz")
    save_reproducibly(path, out)
    print("wrote anchor_head_edges.npz with %d arrays, %.1f KB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
