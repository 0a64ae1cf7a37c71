"""Record what the reference's centre head computes into center_head_state_keys.json and center_head.npz (read by
tests/test_center_head_ref.py and tests/test_gpu_center_head.py).

Usage: python tests/golden/make_golden_center_head.py /path/to/reference/checkout

The reference is only imported, with the stubs of make_golden_point_head_keys.py, a `numba` stub whose jit returns the
function unchanged and Tensor.cuda() as a no-op.  Recorded:
  keys   state_dict keys and shapes of CenterHead at the one-head KITTI configuration of
         tools/cfgs/kitti_models/centerpoint.yaml and at the two-head one [['Car'], ['Pedestrian', 'Cyclist']];
  (a)    CenterHead.assign_target_of_single_head, called unbound on CPU tensors with a stub `self`, on the cases of
         tests/center_targets_ref.py: per case, head and frame the boxes of the head (filtered WITHOUT writing the
         input, class rewritten to the id within the head on a copy) and the four outputs;
  (b)    decode_bbox_from_heatmap on a random (2, 3, 20, 24) head output, K = 16, a score threshold that keeps about half;
  (c)    FocalLossCenterNet and RegLossCenterNet in float64 on targets of (a): values and gradients."""
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
import make_golden_point_head_keys as head_keys  # noqa: E402
import center_targets_ref as ctr  # noqa: E402


def install_stubs(ref_root):
    head_keys.install_stubs(ref_root)
    head_keys.sa_keys._pkg("pcdet.models.model_utils", os.path.join(ref_root, "pcdet", "models", "model_utils"))
    numba = types.ModuleType("numba")

    def jit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda fn: fn

    numba.jit = jit
    sys.modules["numba"] = numba


def head_cfg(names_each_head):
    """The DENSE_HEAD block of tools/cfgs/kitti_models/centerpoint.yaml with the given CLASS_NAMES_EACH_HEAD."""
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    cfg = cfg_from_yaml_file(os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/centerpoint.yaml"),
                             AttrDict())
    head = cfg.MODEL.DENSE_HEAD
    head.CLASS_NAMES_EACH_HEAD = names_each_head
    return cfg, head


KEY_CONFIGS = {"one_head": [["Car", "Pedestrian", "Cyclist"]], "two_heads": [["Car"], ["Pedestrian", "Cyclist"]]}


def record_keys(ref_head):
    out = {}
    for name, each in KEY_CONFIGS.items():
        cfg, head = head_cfg(each)
        m = ref_head.CenterHead(model_cfg=head, input_channels=512, num_class=3, class_names=list(cfg.CLASS_NAMES),
                                grid_size=np.array([1408, 1600, 40]), point_cloud_range=np.array(ctr.RANGE, np.float32),
                                voxel_size=[0.05, 0.05, 0.1], predict_boxes_when_training=False)
        out[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "center_head_state_keys.json"), "w") as f:   # one key per line
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(json.dumps(e) for e in entries))
                                   for name, entries in out.items()) + "\n}\n")
    return {k: len(v) for k, v in out.items()}


def record_targets(ref_head, data):
    stub = types.SimpleNamespace(point_cloud_range=np.array(ctr.RANGE, np.float32), voxel_size=list(ctr.VOXEL_SIZE))
    cases = ctr.cases()
    data["a/names"] = np.array(sorted(cases))
    for name, case in cases.items():
        data["a/%s/gt" % name] = case["gt"]
        data["a/%s/k" % name] = np.int64(case["k"])
        data["a/%s/heads" % name] = np.array([",".join(str(i) for i in ids) for ids in case["heads"]])
        for h, ids in enumerate(case["heads"]):
            for f, frame in enumerate(case["gt"]):
                rows = [r.copy() for r in frame if int(r[-1]) in ids]
                for r in rows:
                    r[-1] = ids.index(int(r[-1])) + 1
                own = torch.from_numpy(np.stack(rows)) if rows else torch.zeros((0, frame.shape[1]))
                heatmap, boxes, inds, mask = ref_head.CenterHead.assign_target_of_single_head(
                    stub, num_classes=len(ids), gt_boxes=own, feature_map_size=[ctr.W, ctr.H],
                    feature_map_stride=ctr.STRIDE, num_max_objs=case["k"], gaussian_overlap=ctr.OVERLAP,
                    min_radius=ctr.MIN_RADIUS)
                assert inds.dtype == mask.dtype == torch.int64 and heatmap.dtype == boxes.dtype == torch.float32
                key = "a/%s/h%d/f%d/" % (name, h, f)
                data[key + "heatmap"], data[key + "target_boxes"] = heatmap.numpy(), boxes.numpy()
                data[key + "inds"], data[key + "mask"] = inds.numpy(), mask.numpy()
    radii = ctr.check_radius_margin(cases)       # asserts the 1e-3 margin to the next integer
    return radii


def record_decode(ref_utils, data):
    g = torch.Generator().manual_seed(20)
    hm = torch.randn(2, 3, 20, 24, generator=g).sigmoid()
    parts = dict(heatmap=hm, rot_cos=torch.randn(2, 1, 20, 24, generator=g), rot_sin=torch.randn(2, 1, 20, 24, generator=g),
                 center=torch.rand(2, 2, 20, 24, generator=g), center_z=torch.randn(2, 1, 20, 24, generator=g),
                 dim=torch.randn(2, 3, 20, 24, generator=g).mul(0.3).exp())
    k = 16
    top = torch.topk(hm.flatten(1), k)[0]
    thresh = float(top[:, k // 2 - 1:k // 2 + 1].mean())     # between the 8th and 9th best: keeps about half
    limit = torch.tensor([-5.0, -9.0, -3.0, 14.6, 9.0, 3.0])
    out = ref_utils.decode_bbox_from_heatmap(point_cloud_range=np.array(ctr.RANGE, np.float32),
                                             voxel_size=list(ctr.VOXEL_SIZE), feature_map_stride=ctr.STRIDE, K=k,
                                             circle_nms=False, score_thresh=thresh, post_center_limit_range=limit, **parts)
    for name, t in parts.items():
        data["b/in/" + name] = t.numpy()
    data["b/k"], data["b/score_thresh"], data["b/limit"] = np.int64(k), np.float64(thresh), limit.numpy()
    kept = []
    for f, d in enumerate(out):
        kept.append(len(d["pred_scores"]))
        for key, t in d.items():
            data["b/out/f%d/%s" % (f, key)] = t.numpy()
    return kept


def record_losses(ref_loss, data):
    heat, boxes, inds, mask = [], [], [], []
    for name in ctr.LOSS_CASES:      # three frames as one batch
        f = 0
        while "a/%s/h0/f%d/heatmap" % (name, f) in data:
            key = "a/%s/h0/f%d/" % (name, f)
            heat.append(data[key + "heatmap"]), boxes.append(data[key + "target_boxes"])
            inds.append(data[key + "inds"]), mask.append(data[key + "mask"])
            f += 1
    heat, boxes = torch.from_numpy(np.stack(heat)).double(), torch.from_numpy(np.stack(boxes)).double()
    inds, mask = torch.from_numpy(np.stack(inds)), torch.from_numpy(np.stack(mask))
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(heat.shape, generator=g)                       # float32 values, evaluated in float64
    regs = torch.randn(heat.shape[0], 8, ctr.H, ctr.W, generator=g)
    weights = torch.rand(8, generator=g).double() + 0.5                 # tells the columns apart in the gradient
    data["c/logits"], data["c/regs"], data["c/weights"] = logits.numpy(), regs.numpy(), weights.numpy()
    for tag, target in (("hm", heat), ("hm_empty", torch.zeros_like(heat))):
        pred = torch.clamp(logits.double().sigmoid(), min=1e-4, max=1 - 1e-4).requires_grad_(True)
        loss = ref_loss.FocalLossCenterNet()(pred, target)
        loss.backward()
        data["c/%s/loss" % tag], data["c/%s/grad" % tag] = loss.detach().numpy(), pred.grad.numpy()
    out = regs.double().requires_grad_(True)
    loss = ref_loss.RegLossCenterNet()(out, mask, inds, boxes)
    (loss * weights).sum().backward()
    data["c/reg/loss"], data["c/reg/grad"] = loss.detach().numpy(), out.grad.numpy()
    return float(data["c/hm/loss"]), loss.detach().numpy().round(3).tolist()


def main(ref_root):
    install_stubs(ref_root)
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **kw: self
    try:
        from pcdet.models.dense_heads import center_head as ref_head
        from pcdet.models.model_utils import centernet_utils as ref_utils
        from pcdet.utils import loss_utils as ref_loss
        print("keys", record_keys(ref_head))
        data = {}
        print("radii", np.round(np.unique(record_targets(ref_head, data)), 4))
        print("decode kept", record_decode(ref_utils, data))
        print("losses", record_losses(ref_loss, data))
    finally:
        torch.Tensor.cuda = real_cuda
    path = os.path.join(HERE, "center_head.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
