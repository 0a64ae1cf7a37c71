"""Record what the reference's PointIntraPartOffsetHead (the fork's version) computes on a small ragged scene into
part_a2.npz and part_a2_state_keys.json (read by tests/test_part_a2_ref.py).

Usage: python tests/golden/make_golden_part_a2.py /path/to/reference/checkout

The reference is only imported, with the stubs of make_golden_roi_head.py (its compiled extensions are empty modules).
Everything runs in float64 on the CPU, in training mode.  Patched in the reference while recording:
  roiaware_pool3d_utils.points_in_boxes_gpu -> tests/roiaware_ref.points_in_boxes;
  Tensor.cuda                               -> a no-op;
  torch.matmul                              -> the second operand converted to the first's dtype AFTER the reference's
                                               own `.float()` rounded the rotation matrix (make_golden_pv_rcnn.py);
  partA2_head.spconv                        -> tests/part_a2_ref.spconv_standin: SparseConvTensor, SparseSequential and
                                               SubMConv3d as a dense float64 conv3d read back at the active sites;
  RoIAwarePool3d.forward                    -> tests/part_a2_ref.torch_roiaware_pool: the point lists of
                                               tests/roiaware_ref.collect, the pooling in differentiable float64 torch;
  PartA2FCHead.assign_targets (instance)    -> the scene's fixed targets (the sampler draws random numbers);
  Tensor.float inside the forward and the losses -> double (float32 weights and labels would meet float64 scores), as
                                                 make_golden_roi_head.py does.
Recorded: the state_dict keys and shapes of the head with FEATURES_FC [32] on 64 input channels; its weights (w/point/);
the scene (four ragged frames, one empty, a padded box row); the class labels, the part labels, point_cls_scores,
point_part_offset, every 16th column of the rewritten x_points_mean features and the loss.
For the reference's PartA2FCHead, DP_RATIO 0, on part_a2_ref.roi_scene (two frames of 130 and 63 points, 4 RoIs each) at
POOL_SIZE 4 and 6 and on the scene without scores that takes the fake branch: the state_dict keys, coords, the pooled part
and rpn rows, rcnn_cls, rcnn_reg, the labels after the forward (the fake branch invalidates them), the loss (for the fake scene the sum of rcnn_cls
and rcnn_reg instead: binary_cross_entropy refuses its -1 labels on the CPU), and the
gradients w.r.t. point_features, point_part_offset and the head's first (every 7th element) and last weights."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tsm-det-pointcloud-_amd"))
import make_golden_roi_head as roi_golden  # noqa: E402
import part_a2_ref as A  # noqa: E402
import pv_rcnn_ref as V  # noqa: E402


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main(ref_root):
    roi_golden.install_stubs(ref_root)
    from pcdet_amd.config import AttrDict
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as ref_rp
    from pcdet.models.dense_heads import point_intra_part_head as ref_point
    ref_rp.points_in_boxes_gpu = V.cpu_points_in_boxes
    real_cuda, real_matmul = torch.Tensor.cuda, torch.matmul
    torch.Tensor.cuda = lambda self, *a, **kw: self
    torch.matmul = lambda a, b: real_matmul(a, b.to(a.dtype))
    try:
        data = record(ref_point, AttrDict)
        from pcdet.models.roi_heads import partA2_head as ref_head_mod
        ref_head_mod.spconv = A.spconv_standin
        ref_rp.RoIAwarePool3d.forward = A.torch_roiaware_pool
        keys = None
        for name, case in A.ROI_CASES.items():
            keys = record_roi(ref_head_mod, AttrDict, name, case, data)
        write(data, keys)
    finally:
        torch.Tensor.cuda, torch.matmul = real_cuda, real_matmul


def record(ref_point, AttrDict):
    sc = A.point_scene()
    torch.manual_seed(2)
    head = ref_point.PointIntraPartOffsetHead(num_class=1, input_channels=64,
                                              model_cfg=AttrDict(A.point_head_cfg(FEATURES_FC=[32], CLS_FC=[8]))).double().train()
    V.randomize_norms(head, 13)
    data = {"w/point/" + k: v.numpy().copy() for k, v in head.state_dict().items()}
    keys = [[k, list(v.shape)] for k, v in head.state_dict().items()]
    sp = types.SimpleNamespace(features=None)
    sp.replace_feature = lambda f: types.SimpleNamespace(features=f)
    batch = dict(batch_size=4, point_features=t(sc["features"]), point_coords=t(sc["points"]), gt_boxes=t(sc["gt_boxes"]),
                 multi_scale_3d_features={"x_points_mean": sp, "x_points_max": sp})
    with roi_golden._float_is_double():
        batch = head(batch)
        loss, tb = head.get_loss()
    ret = head.forward_ret_dict
    data.update(points=sc["points"], gt_boxes=sc["gt_boxes"],
                point_cls_labels=ret["point_cls_labels"].numpy(), point_part_labels=ret["point_part_labels"].numpy(),
                point_cls_scores=batch["point_cls_scores"].detach().numpy(),
                point_part_offset=batch["point_part_offset"].detach().numpy(), point_loss=loss.detach().numpy(),
                x_points_mean=batch["multi_scale_3d_features"]["x_points_mean"].features.detach().numpy()[:, ::16])
    print("loss", float(loss), "labels", np.unique(data["point_cls_labels"], return_counts=True))
    data["_point_keys"] = keys
    return data


def record_roi(ref_head_mod, AttrDict, name, case, data):
    """One training forward, loss and backward of the reference's PartA2FCHead on A.roi_scene; the weights are not stored:
    both sides build the head after torch.manual_seed(5) and prepare it with A.prepare_roi_head (checked through the
    recorded first and last weights)."""
    sc = A.roi_scene(fake=case["fake"])
    torch.manual_seed(5)
    head = ref_head_mod.PartA2FCHead(input_channels=A.ROI_CHANNELS, model_cfg=AttrDict(A.roi_head_cfg(case["pool"])),
                                     num_class=1).double().train()
    A.prepare_roi_head(head, 31)
    targets = {k: t(v.copy()) for k, v in sc["targets"].items()}
    head.assign_targets = lambda batch_dict: targets
    out, ret, feats, offset = A.run_roi_head(head, sc, t)
    if case["fake"]:
        # every label is -1 now, which binary_cross_entropy refuses on the CPU: the gradients are those of a plain sum
        loss = ret["rcnn_cls"].sum() + ret["rcnn_reg"].sum()
    else:
        with roi_golden._float_is_double():
            loss_cls, _ = head.get_box_cls_layer_loss(ret)
        loss_reg, _ = head.get_box_reg_layer_loss(ret)
        loss = loss_cls + loss_reg
    loss.backward()
    out["loss"] = loss.detach().numpy()
    out.update(A.roi_grads(head, feats, offset))
    for k, v in out.items():
        data["%s/%s" % (name, k)] = v
    print(name, "rows", out["coords"].shape[0], "loss", float(loss), "labels", out["rcnn_cls_labels"].reshape(-1)[:3])
    return [[k, list(v.shape)] for k, v in head.state_dict().items()]


def write(data, roi_keys):
    keys = data.pop("_point_keys")
    with open(os.path.join(HERE, "part_a2_state_keys.json"), "w") as f:
        f.write("{\n\"point_head\": [\n%s\n],\n\"roi_head\": [\n%s\n]\n}\n"
                % (",\n".join(json.dumps(e) for e in keys), ",\n".join(json.dumps(e) for e in roi_keys)))
    path = os.path.join(HERE, "part_a2.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
