"""Record the fast_cpc point head's losses and their gradients, as the reference computes them, into
point_head_losses.npz (read by tests/test_point_loss_ref.py and tests/test_gpu_point_loss.py).

Usage: python tests/golden/make_golden_point_head_losses.py /path/to/reference/checkout

The reference's PointHeadVoteSASAStatisticDistillation is built on the CPU with the stubs of
make_golden_point_head_keys.py (KITTI head of tests/point_head_configs.py), its forward_ret_dict is filled with float64
tensors and get_vote_layer_loss / get_cls_layer_loss / get_box_layer_loss run as they are, normalised as get_loss does;
PointSASALoss.loss_forward runs for both loss functions.  Nothing of the project's own loss code is used.  The
reference casts with .float() on the way (the rotation matrix of rotate_points_along_z, the masks' weights), which would
mix float32 into the evaluation and stop its matmul; for the run Tensor.float is pointed at Tensor.double, which changes
no arithmetic, only its precision.

Per case (prefix a_, b_, c_) the file holds the inputs as float32 (vote_coords, cls_preds, reg_preds, box_preds,
t_cls_preds, t_reg_preds, t_box_preds, vote_cls_labels, vote_reg_labels, cls_labels, reg_labels, box_labels; the
reference runs on their float64 images), losses (3) = (vote, cls, box) and, in float64, g<k>_<leaf> the gradient of
component k (0 vote, 1 cls, 2 box) and gsum_<leaf> that of the sum, for the leaves vote, cls, reg, box, of which only
the ones that are not zero by construction are stored (STORED below), and the SASA inputs and results seg_scores1
(N, 1), seg_scores3 (N, 3), seg_labels and
seg_<func>_s<S> (loss), seg_<func>_s<S>_grad for the combinations the reference evaluates (SEG_COMBOS below says
which it does not).

Inputs: points and gt_boxes of tests/point_targets_ref.make_case; labels of point_targets_ref.assign (BALL for the head's
labels, PLAIN for the vote labels, IGNORE_RING for the SASA labels); student reg_preds = labels + N(0, 0.3), box_preds =
the coder's decode of them + N(0, 0.05); the teacher's are an independent draw of the same.  A case is redrawn with the
next seed until every min / max / clamp / smooth-L1 operand pair evaluated on a positive row differs by more than 1e-6,
so that no result depends on how a tie is broken."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tsm-det-pointcloud-_amd"))
import make_golden_point_head_keys as head_keys  # noqa: E402
import point_head_configs  # noqa: E402
import point_targets_ref as ptr  # noqa: E402

BINS = 12
NUM_CLASS = 3
SEG_LAYER_WEIGHT = 0.1
GAP = 1e-6
LEAVES = ("vote", "cls", "reg", "box")
# The gradients that are not identically zero.  The recorder asserts that every other (component, leaf) gradient is all
# zero and that the sum's gradient equals bitwise the one component that reaches the leaf (SUM_IS), so only the box
# predictions, which the cls loss reaches through its soft target and the box loss directly, need a stored sum.
STORED = ((0, "vote"), (1, "cls"), (1, "box"), (2, "reg"), (2, "box"), ("sum", "box"))
SUM_IS = {"vote": 0, "cls": 1, "reg": 2}
# (func, S): the reference's BCE hands a one-column score and a three-column target to
# F.binary_cross_entropy_with_logits, which refuses shapes that differ, so ("BCE", 1) with num_class 3 cannot be recorded
SEG_COMBOS = (("BCE", 3), ("Focal", 1), ("Focal", 3))
#             name  b  n    m  zero_gt
CASES = (("a", 2, 37, 5, False), ("b", 3, 171, 5, False), ("c", 2, 37, 5, True))


def draw(b, n, m, zero_gt, seed, empty_frame):
    pts, gt, _ = ptr.make_case(m, 8, b=b, n=n, seed=seed)
    # make_case puts its points 0..2 on a face and on a box centre, where min and max tie: move them next to others
    pts[:, 0:3] = pts[:, 3:6] + np.random.default_rng(seed).uniform(0.05, 0.3, (b, 3, 3)).astype(np.float32)
    gt[:, 2, 0] += 500.0         # make_case's box 2 is 5e-6 thin, both x faces tie for every point inside: move it away
    if zero_gt:
        gt[:] = 0
    if empty_frame is not None:
        gt[empty_frame] = 0
    head = ptr.assign(pts, gt, ptr.BALL, central_radius=ptr.RADIUS, num_class=NUM_CLASS, bins=BINS)
    vote = ptr.assign(pts, gt, ptr.PLAIN, extra_width=ptr.EXTRA_WIDTH, num_class=1)
    seg = ptr.assign(pts, gt, ptr.IGNORE_RING, extra_width=(1.0, 1.0, 1.0), num_class=NUM_CLASS)
    rng = np.random.default_rng(77 + seed)
    rows = b * n
    t_reg = head["reg_labels"] + rng.normal(0, 0.3, (rows, 6 + 2 * BINS))
    d = {"vote_coords": pts.reshape(-1, 3),
         "vote_cls_labels": vote["cls_labels"], "vote_reg_labels": vote["center_labels"],
         "cls_labels": head["cls_labels"], "reg_labels": head["reg_labels"], "box_labels": head["box_labels"],
         "cls_preds": grid(rng.normal(0, 1.5, (rows, NUM_CLASS))), "t_cls_preds": grid(rng.normal(0, 1.5, (rows, NUM_CLASS))),
         "reg_preds": grid(head["reg_labels"] + rng.normal(0, 0.3, (rows, 6 + 2 * BINS))),
         "t_reg_preds": grid(t_reg),
         "box_noise": rng.normal(0, 0.05, (rows, 7)), "t_box_noise": rng.normal(0, 0.05, (rows, 7)),
         "seg_labels": seg["cls_labels"], "seg_scores1": grid(rng.normal(0, 1.5, (rows, 1))),
         "seg_scores3": grid(rng.normal(0, 1.5, (rows, NUM_CLASS)))}
    return d, gt, t_reg


def grid(x):
    """Round to multiples of 2^-8 and to float32: every input of the fixture is a float32 value, so the float64
    reference and the float32 op start from the same numbers, and the short mantissas keep the file small."""
    return (np.round(np.asarray(x, np.float64) * 256.0) / 256.0).astype(np.float32)


def decode_boxes(coder, d, t_reg):
    """box_preds = the coder's decode of the regression code at the points, perturbed.  The teacher's code is then cut
    to the six offsets the loss reads (the other columns are stored as zeros)."""
    pts = torch.from_numpy(d["vote_coords"].astype(np.float64))
    for pre, reg in (("", d["reg_preds"]), ("t_", t_reg)):
        box = coder.decode_torch(torch.from_numpy(np.asarray(reg, np.float64)), pts).numpy()
        # not on the grid: the student's and the teacher's box faces are compared with each other and would tie on it
        d[pre + "box_preds"] = (box[:, :7] + d.pop(pre + "box_noise")).astype(np.float32)
    d["t_reg_preds"][:, 6:] = 0


# ---------------------------------------------------------------------------------- distance from every breakpoint

def _centerness_pairs(p, box, out):
    c = p - box[:, 0:3]
    ca, sa = np.cos(-box[:, 6]), np.sin(-box[:, 6])
    local = np.stack([c[:, 0] * ca - c[:, 1] * sa, c[:, 0] * sa + c[:, 1] * ca, c[:, 2]], axis=1)
    prod = 1.0
    for k in range(3):
        lo, hi = box[:, 3 + k] / 2 - local[:, k], box[:, 3 + k] / 2 + local[:, k]
        out.append(lo - hi)
        prod = prod * np.minimum(lo, hi) / np.maximum(lo, hi)
    out.append(prod - 1e-6)


def _rdiou_pairs(b1, b2, out):
    t1, t2 = np.sin(b1[:, 6]) * np.cos(b2[:, 6]), np.cos(b1[:, 6]) * np.sin(b2[:, 6])
    size1 = b1[:, 3:6]
    out.append(size1 - 10.0)
    size1 = np.minimum(size1, 10.0)
    dims = [(b1[:, k], size1[:, k], b2[:, k], b2[:, 3 + k]) for k in range(3)] + [(t1, 1.0, t2, 1.0)]
    for p1, s1, p2, s2 in dims:
        out.append((p1 - s1 / 2) - (p2 - s2 / 2))
        out.append((p1 + s1 / 2) - (p2 + s2 / 2))
        out.append(np.minimum(p1 + s1 / 2, p2 + s2 / 2) - np.maximum(p1 - s1 / 2, p2 - s2 / 2))
        out.append(np.maximum(p1 + s1 / 2, p2 + s2 / 2) - np.minimum(p1 - s1 / 2, p2 - s2 / 2))


def _corners(b):
    signs = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]]) / 2
    local = b[:, None, 3:6] * signs[None]
    c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    return np.stack([local[..., 0] * c - local[..., 1] * s, local[..., 0] * s + local[..., 1] * c, local[..., 2]], -1) \
        + b[:, None, 0:3]


def _sl1(x, beta):
    n = np.abs(x)
    return np.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)


def _corner_pairs(b1, b2, out):
    flip = b2.copy()
    flip[:, 6] += np.pi
    d0, d1 = _corners(b1) - _corners(b2), _corners(b1) - _corners(flip)
    out.append(np.abs(d0) - 1.0)
    out.append(np.abs(d1) - 1.0)
    out.append(_sl1(d0, 1.0).sum(-1) - _sl1(d1, 1.0).sum(-1))


def smallest_gap(d, beta):
    """The smallest |a - b| over the operand pairs (a, b) of every min, max, clamp, abs and smooth-L1 branch that a
    positive row (for the SASA scores: a row that is not ignored) evaluates, in float64."""
    d = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in d.items()}
    out = []
    vp = d["vote_cls_labels"] > 0
    out.append(np.abs(d["vote_coords"][vp] - d["vote_reg_labels"][vp]) - beta)
    pos = d["cls_labels"] > 0
    reg, lab, treg = d["reg_preds"][pos], d["reg_labels"][pos], d["t_reg_preds"][pos]
    out.append(np.abs(reg[:, :6] - lab[:, :6]) - beta)
    out.append(np.abs(reg[:, :6] - treg[:, :6]) - beta)
    onehot = lab[:, 6:6 + BINS]
    res = (reg[:, 6 + BINS:] * onehot).sum(-1) - (lab[:, 6 + BINS:] * onehot).sum(-1)
    out.append(np.abs(res) - beta)
    p, box, lbox, tbox = d["vote_coords"][pos], d["box_preds"][pos], d["box_labels"][pos], d["t_box_preds"][pos]
    for other in (lbox, tbox):
        _centerness_pairs(p, other, out)
        _rdiou_pairs(box, other, out)
        _corner_pairs(box, other, out)
    # the focal loss of the SASA layers is written with clamp(x, min=0) and abs(x): a score of exactly 0 is a breakpoint
    counted = d["seg_labels"] >= 0
    out.append(d["seg_scores1"][counted])
    out.append(d["seg_scores3"][counted])
    flat = np.concatenate([np.ravel(o) for o in out]) if out else np.zeros(0)
    return np.abs(flat).min() if flat.size else np.inf


# ---------------------------------------------------------------------------------------------- the reference's run

def run_reference(head, loss_utils, d):
    t = {k: torch.from_numpy(np.ascontiguousarray(v.astype(np.float64) if v.dtype == np.float32 else v))
         for k, v in d.items()}
    leaves = {"vote": t["vote_coords"].clone().requires_grad_(True), "cls": t["cls_preds"].clone().requires_grad_(True),
              "reg": t["reg_preds"].clone().requires_grad_(True), "box": t["box_preds"].clone().requires_grad_(True)}
    head.forward_ret_dict = {
        "s_point_vote_coords": leaves["vote"], "vote_cls_labels": t["vote_cls_labels"],
        "vote_reg_labels": t["vote_reg_labels"],
        "s_point_cls_preds": leaves["cls"], "s_point_reg_preds": leaves["reg"], "s_point_box_preds": leaves["box"],
        "point_cls_preds": t["t_cls_preds"], "point_reg_preds": t["t_reg_preds"], "point_box_preds": t["t_box_preds"],
        "s_point_cls_labels": t["cls_labels"], "s_point_reg_labels": t["reg_labels"],
        "s_point_box_labels": t["box_labels"],
    }
    vote, _ = head.get_vote_layer_loss()
    cls, cls_w, _ = head.get_cls_layer_loss()
    box, box_w, _ = head.get_box_layer_loss()
    cls = cls.sum() / torch.clamp(cls_w.sum(), min=1.0)
    box = box.sum() / torch.clamp(box_w.sum(), min=1.0)
    comps = [vote, cls, box]
    out = {"losses": np.array([c.item() for c in comps])}
    order = [leaves[k] for k in LEAVES]
    for k, comp in list(enumerate(comps)) + [("sum", vote + cls + box)]:
        grads = torch.autograd.grad(comp, order, retain_graph=True, allow_unused=True)
        for name, leaf, g in zip(LEAVES, order, grads):
            g = (torch.zeros_like(leaf) if g is None else g).numpy()
            if (k, name) in STORED:
                out["g%s_%s" % (k, name)] = g
            elif k == "sum":
                assert np.array_equal(g, out["g%d_%s" % (SUM_IS[name], name)]), name
            else:
                assert not g.any(), (k, name)
    for func, s in SEG_COMBOS:
        sasa = loss_utils.PointSASALoss(func=func, layer_weights=[SEG_LAYER_WEIGHT], extra_width=[1.0, 1.0, 1.0],
                                        set_ignore_flag=True, num_class=NUM_CLASS)
        scores = t["seg_scores%d" % s].clone().requires_grad_(True)
        loss, = sasa.loss_forward([scores], [t["seg_labels"]], [None], [None], [None])
        out["seg_%s_s%d" % (func, s)] = np.array(loss.item())
        out["seg_%s_s%d_grad" % (func, s)] = torch.autograd.grad(loss.sum(), scores)[0].numpy()
    return out


def main(ref_root):
    head_keys.install_stubs(ref_root)
    from pcdet_amd.config import AttrDict
    real_tensor = torch.tensor

    def cpu_tensor(*a, **kw):
        if str(kw.get("device", "")).startswith("cuda"):
            kw["device"] = "cpu"
        return real_tensor(*a, **kw)

    torch.tensor = cpu_tensor
    real_float = torch.Tensor.float
    try:
        from pcdet.models.dense_heads import point_head_vote_sasa_statistic_distillation as ref
        from pcdet.utils import loss_utils
        head = ref.PointHeadVoteSASAStatisticDistillation(model_cfg=AttrDict(point_head_configs.head_dict("kitti")),
                                                          **point_head_configs.head_kwargs())
        beta = head.reg_loss_func.beta
        torch.Tensor.float = torch.Tensor.double      # see the module docstring
        record = {}
        for name, b, n, m, zero_gt in CASES:
            empty_frame = 1 if name == "b" else None
            for seed in range(100):
                d, gt, t_reg = draw(b, n, m, zero_gt, seed, empty_frame)
                decode_boxes(head.box_coder, d, t_reg)
                lab, per_frame = d["cls_labels"], (d["cls_labels"].reshape(b, n) > 0).sum(axis=1)
                if name == "a" and not ((lab > 0).sum() >= 12 and (lab == -1).sum() >= 4 and (lab == 0).sum() >= 20):
                    continue
                if name == "b" and not (per_frame[1] == 0 and per_frame[0] > 0 and per_frame[2] > 0):
                    continue
                if smallest_gap(d, beta) > GAP:
                    break
            else:
                raise RuntimeError("case %s: no seed meets the conditions" % name)
            if name == "a":
                assert b * n == 74 and (lab > 0).sum() >= 12 and (lab == -1).sum() >= 4 and (lab == 0).sum() >= 20
            elif name == "b":
                assert b * n == 513 and per_frame[1] == 0 and per_frame.sum() > 0
            else:
                assert b * n == 74 and not gt.any() and (lab > 0).sum() == 0 and (d["vote_cls_labels"] > 0).sum() == 0
            assert smallest_gap(d, beta) > GAP
            res = run_reference(head, loss_utils, d)
            print("case %s seed %d: rows %d, positives %d, ignored %d, vote positives %d, smallest gap %.3g, losses %s"
                  % (name, seed, b * n, (lab > 0).sum(), (lab == -1).sum(), (d["vote_cls_labels"] > 0).sum(),
                     smallest_gap(d, beta), res["losses"]))
            for k, v in list(d.items()) + list(res.items()):
                v = np.asarray(v)
                assert np.isfinite(v).all(), (name, k)
                record["%s_%s" % (name, k)] = v
            record["%s_shape" % name] = np.array([b, n])
    finally:
        torch.tensor = real_tensor
        torch.Tensor.float = real_float
    path = os.path.join(HERE, "point_head_losses.npz")
    np.savez_compressed(path, **record)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print("wrote %s: %d arrays, %d bytes" % (path, len(record), size))


if __name__ == "__main__":
    main(sys.argv[1])
