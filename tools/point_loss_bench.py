"""Times the point head's get_loss_fused (csrc/point_loss.hip, include/spx.h §17) against get_loss_torch, the eager
torch composition of the same losses, forward + backward onto the four prediction tensors; prints one table.

  python tools/point_loss_bench.py [--iters N]

Shapes: KITTI 4 x 512 and 16 x 512, Waymo 4 x 3072 rows, with the SASA layers of the fast_cpc config (4096, 512, 512 /
16384, 3072, 3072 points per frame, one score column, three classes).  The targets are assigned once, before timing, by
the head's own assignment ops on the frames of tools/point_targets_bench.py; predictions are the labels plus noise.  Both
paths are compared on the timed inputs before timing.  Times are HIP-event times around windows of back-to-back calls
(`iters` eager, 10 x `iters` fused), the median of five alternating windows, host work and the eager path's host reads
(its boolean-mask indexing) included."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tsm-det-pointcloud-_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import point_targets_bench as ptb  # noqa: E402  (same directory)

LEAVES = ("s_point_vote_coords", "s_point_cls_preds", "s_point_reg_preds", "s_point_box_preds")


def make_ret_dict(head, kind, batch, n, m, layer_points, dev):
    points, gt = ptb.make_batch(kind, batch, n, m, 1, dev)
    stu = head.assign_stu_targets({"s_point_vote_coords": points, "gt_boxes": gt})
    vote = head.assign_targets_simple(points, gt, extra_width=head.model_cfg.TARGET_CONFIG.VOTE_EXTRA_WIDTH,
                                      set_ignore_flag=False)
    gen = torch.Generator().manual_seed(0)

    def noisy(t, sigma):
        return (t.cpu() + torch.randn(t.shape, generator=gen) * sigma).to(dev)

    rows = points.shape[0]
    xyz = points[:, 1:4].contiguous()
    reg, t_reg = noisy(stu["point_reg_labels"], 0.3), noisy(stu["point_reg_labels"], 0.3)
    layers = [ptb.make_batch(kind, batch, k, m, 2 + i, dev)[0] for i, k in enumerate(layer_points)]
    scores = [noisy(torch.zeros(p.shape[0], 1), 1.5) for p in layers]
    l_labels, l_boxes, l_parts = head.loss_point_sasa(layers, scores, gt)
    rd = {"s_point_vote_coords": xyz, "vote_cls_labels": vote["point_cls_labels"],
          "vote_reg_labels": vote["point_reg_labels"],
          "s_point_cls_preds": noisy(torch.zeros(rows, head.num_class), 1.5), "s_point_reg_preds": reg,
          "s_point_box_preds": noisy(head.box_coder.decode_torch(reg, xyz)[:, :7], 0.05),
          "point_cls_preds": noisy(torch.zeros(rows, head.num_class), 1.5), "point_reg_preds": t_reg,
          "point_box_preds": noisy(head.box_coder.decode_torch(t_reg, xyz)[:, :7], 0.05),
          "s_point_cls_labels": stu["point_cls_labels"], "s_point_reg_labels": stu["point_reg_labels"],
          "s_point_box_labels": stu["point_box_labels"],
          "point_sasa_preds": scores, "point_sasa_labels": l_labels, "point_sasa": layers,
          "point_sasa_boxes": l_boxes, "point_sasa_parts": l_parts}
    for k in LEAVES:
        rd[k].requires_grad_(True)
    for s in scores:
        s.requires_grad_(True)
    return rd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    import point_head_configs as phc
    from pcdet_amd.models import dense_heads
    from spx import _lib
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    head = dense_heads.__all__["PointHeadVoteSASAStatisticDistillation"](model_cfg=phc.head_cfg(), **phc.head_kwargs())
    head = head.to(dev)
    rows = []
    for name, kind, batch, n, m, layer_points in (("KITTI  4 x  512", 1, 4, 512, 40, (4096, 512, 512)),
                                                  ("KITTI 16 x  512", 1, 16, 512, 40, (4096, 512, 512)),
                                                  ("Waymo  4 x 3072", 3, 4, 3072, 160, (16384, 3072, 3072))):
        rd = make_ret_dict(head, kind, batch, n, m, layer_points, dev)
        wrt = [rd[k] for k in LEAVES] + list(rd["point_sasa_preds"])

        def step(method):
            loss, _ = method(rd)
            return loss, torch.autograd.grad(loss, wrt)

        (le, ge), (lf, gf) = step(head.get_loss_torch), step(head.get_loss_fused)
        le, lf = le.detach(), lf.detach()
        worst = max(float((a - b).abs().max() / a.abs().max().clamp(min=1e-12)) for a, b in zip(ge, gf))
        if abs(float(le) - float(lf)) > 1e-4 * abs(float(le)) or worst > 1e-3:
            raise SystemExit("%s: fused and eager differ: loss %r vs %r, gradients by %.3g of their largest entry"
                             % (name, float(le), float(lf), worst))
        te, tf, sp = ptb.timed_pair(lambda: step(head.get_loss_torch), lambda: step(head.get_loss_fused), args.iters)
        rows.append((name, te, tf, sp, int((rd["s_point_cls_labels"] > 0).sum()) / batch))

    print("device: %s" % torch.cuda.get_device_name(0))
    print("library: %s" % os.path.relpath(_lib.LIB_PATH, ROOT))
    print()
    print("%-18s %10s %10s %9s %8s %10s" % ("get_loss + backward", "eager us", "fused us", "eager/f", "spread", "pos/frame"))
    for name, te, tf, sp, fg in rows:
        print("%-18s %10.1f %10.1f %8.1fx %7.1f%% %10.1f" % (name, te, tf, te / tf, 100 * sp, fg))
    print()
    print("eager = get_loss_torch (torch composition of the reference's three loss methods and three SASA layers, with its")
    print("boolean-mask host reads) + autograd; fused = get_loss_fused: 3 launches for the head's losses and 3 per SASA")
    print("layer, gradients saved by the forward, backward scales them.  Losses equal to 1e-4 relative and gradients to")
    print("1e-3 of their largest entry on these inputs before timing.")
    print("Per call, median of 5 alternating windows of %d eager / %d fused calls; spread = largest deviation of a window"
          % (args.iters, 10 * args.iters))
    print("from its median.")
    slower = [name for name, te, tf, _, _ in rows if tf >= te]
    print("fused NOT faster than eager at: %s" % (", ".join(slower) if slower else "none"))


if __name__ == "__main__":
    main()
