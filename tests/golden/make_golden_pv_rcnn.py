"""Record what the reference's VoxelSetAbstraction, PointHeadSimple and PVRCNNHead compute on the scene of
tests/pv_rcnn_ref.py into pv_rcnn.npz and pv_rcnn_state_keys.json (read by tests/test_pv_rcnn_ref.py).

Usage: python tests/golden/make_golden_pv_rcnn.py /path/to/reference/checkout

The reference is only imported, with the stubs of make_golden_roi_head.py (its compiled extensions are empty modules).
Everything runs in float64 on the CPU, in training mode, DP_RATIO 0.  Patched in the reference while recording:
  pointnet2_stack_utils.ball_query            -> tests/pointnet2_stack_ref.ball_query (a CUDA extension in the reference);
  pointnet2_stack_utils.farthest_point_sample -> tests/pointnet2_ref.furthest_point_sample, the batch sampler the
                                                 reference calls frame by frame;
  pointnet2_stack_utils.grouping_operation    -> a torch gather of the frame-local rows;
  roiaware_pool3d_utils.points_in_boxes_gpu   -> tests/roiaware_ref.points_in_boxes;
  common_utils.get_voxel_centers (in the PFE) -> its own float32 result converted to double: QueryAndGroup subtracts the
                                                 float64 keypoints from the grouped centres IN PLACE, which would round
                                                 the offsets to float32 in a float64 run;
  torch.matmul                                -> the second operand converted to the first's dtype AFTER the reference's
                                                 own `.float()` rounded the rotation matrix;
  Tensor.cuda                                 -> a no-op;
  Tensor.float inside the point head's class loss and the RoI head's class loss -> double (float32 weights and labels
                                                 would meet float64 scores), as make_golden_roi_head.py does.
Recorded: the state_dict keys and shapes of the three modules at tools/cfgs/kitti_models/pv_rcnn.yaml; the modules'
weights (w/); keypoints, point_features_before_fusion, point_features; the point head's labels and loss; for GRID_SIZE 2
and 3 the RoI head's pooled features, rcnn_cls, rcnn_reg, the loss on the scene's targets and the gradients of
pv_rcnn_ref.ROI_GRAD_KEYS."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tsm-det-pointcloud-_amd"))
import make_golden_roi_head as roi_golden  # noqa: E402
import pv_rcnn_ref as V  # noqa: E402

YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/pv_rcnn.yaml")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def randomize(module, seed):
    V.randomize_norms(module, seed)
    return module


def record_front(ref_vsa, ref_point, data):
    from pcdet_amd.config import AttrDict
    sc = V.scene()
    torch.manual_seed(1)
    vsa = randomize(ref_vsa.VoxelSetAbstraction(
        model_cfg=AttrDict(V.pfe_cfg()), voxel_size=V.VOXEL, point_cloud_range=V.RANGE, num_bev_features=V.BEV_CHANNELS,
        num_rawpoint_features=V.NUM_RAWPOINT_FEATURES).double().train(), 11)
    head = randomize(ref_point.PointHeadSimple(num_class=1, input_channels=vsa.num_point_features_before_fusion,
                                               model_cfg=AttrDict(V.point_head_cfg())).double().train(), 12)
    for name, m in (("vsa", vsa), ("point", head)):
        for k, v in m.state_dict().items():
            data["w/%s/%s" % (name, k)] = v.numpy().copy()
    batch = vsa(V.batch_of(sc, t))
    batch = head(batch)
    with roi_golden._float_is_double():
        loss, tb = head.get_loss()
    data["keypoints"] = batch["point_coords"].detach().numpy()
    data["point_features_before_fusion"] = batch["point_features_before_fusion"].detach().numpy()
    data["point_features"] = batch["point_features"].detach().numpy()
    data["point_cls_scores"] = batch["point_cls_scores"].detach().numpy()
    data["point_cls_labels"] = head.forward_ret_dict["point_cls_labels"].numpy()
    data["point_loss"] = loss.detach().numpy()
    return batch, float(loss)


def record_roi(ref_head_mod, grid, front, data):
    from pcdet_amd.config import AttrDict
    sc = V.scene()
    torch.manual_seed(grid)
    head = randomize(ref_head_mod.PVRCNNHead(input_channels=16, model_cfg=AttrDict(V.roi_head_cfg(grid)),
                                             num_class=1).double().train(), 20 + grid)
    with torch.no_grad():
        head.reg_layers[-1].weight.normal_(0, 0.1)
    for k, v in head.state_dict().items():
        data["g%d/w/%s" % (grid, k)] = v.numpy().copy()
    batch = dict(batch_size=2, rois=t(sc["rois"]), point_coords=front["point_coords"].detach(),
                 point_features=front["point_features"].detach(), point_cls_scores=front["point_cls_scores"].detach())
    pooled = head.roi_grid_pool(batch)
    n = pooled.shape[0]
    flat = pooled.permute(0, 2, 1).contiguous().view(n, -1, 1)
    shared = head.shared_fc_layer(flat)
    rcnn_cls = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
    rcnn_reg = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
    ret = dict({k: t(v.copy()) for k, v in sc["targets"].items()}, rcnn_cls=rcnn_cls, rcnn_reg=rcnn_reg)
    with roi_golden._float_is_double():
        loss_cls, _ = head.get_box_cls_layer_loss(ret)
    loss_reg, _ = head.get_box_reg_layer_loss(ret)
    loss = loss_cls + loss_reg
    loss.backward()
    named = dict(head.named_parameters())
    data["g%d/pooled" % grid], data["g%d/rcnn_cls" % grid] = pooled.detach().numpy(), rcnn_cls.detach().numpy()
    data["g%d/rcnn_reg" % grid], data["g%d/loss" % grid] = rcnn_reg.detach().numpy(), loss.detach().numpy()
    for k in V.ROI_GRAD_KEYS:
        data["g%d/grad/%s" % (grid, k)] = named[k].grad.numpy()
    return float(loss)


def record_keys(ref_vsa, ref_point, ref_head_mod):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    vsa = ref_vsa.VoxelSetAbstraction(model_cfg=cfg.MODEL.PFE, **V.YAML_KW)
    point = ref_point.PointHeadSimple(num_class=1, input_channels=vsa.num_point_features_before_fusion,
                                      model_cfg=cfg.MODEL.POINT_HEAD)
    roi = ref_head_mod.PVRCNNHead(input_channels=vsa.num_point_features, model_cfg=cfg.MODEL.ROI_HEAD, num_class=1)
    out = {name: [[k, list(v.shape)] for k, v in m.state_dict().items()]
           for name, m in (("pfe", vsa), ("point_head", point), ("roi_head", roi))}
    out["num_point_features_before_fusion"] = vsa.num_point_features_before_fusion
    with open(os.path.join(HERE, "pv_rcnn_state_keys.json"), "w") as f:      # one key per line
        f.write("{\n" + ",\n".join(
            "%s: %s" % (json.dumps(name), json.dumps(v) if not isinstance(v, list) else
                        "[\n%s\n]" % ",\n".join(json.dumps(e) for e in v)) for name, v in out.items()) + "\n}\n")
    return {k: len(v) for k, v in out.items() if isinstance(v, list)}


def main(ref_root):
    roi_golden.install_stubs(ref_root)
    roi_golden.head_keys.sa_keys._pkg("pcdet.models.backbones_3d", os.path.join(ref_root, "pcdet/models/backbones_3d"))
    roi_golden.head_keys.sa_keys._pkg("pcdet.models.backbones_3d.pfe",
                                      os.path.join(ref_root, "pcdet/models/backbones_3d/pfe"))
    real_matmul, real_cuda = torch.matmul, torch.Tensor.cuda
    torch.matmul = lambda a, b: real_matmul(a, b.to(a.dtype))
    torch.Tensor.cuda = lambda self, *a, **kw: self
    try:
        from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as ref_pu
        from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils as ref_rp
        from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as ref_vsa
        from pcdet.models.dense_heads import point_head_simple as ref_point
        from pcdet.models.roi_heads import pvrcnn_head as ref_head_mod
        ref_pu.ball_query = V.cpu_ball_query
        ref_pu.grouping_operation = V.cpu_grouping
        ref_pu.farthest_point_sample = ref_pu.furthest_point_sample = V.cpu_batch_fps
        ref_rp.points_in_boxes_gpu = V.cpu_points_in_boxes
        real_centers = ref_vsa.common_utils.get_voxel_centers
        ref_vsa.common_utils.get_voxel_centers = lambda *a, **kw: real_centers(*a, **kw).double()
        print("keys", record_keys(ref_vsa, ref_point, ref_head_mod))
        data = {}
        front, loss = record_front(ref_vsa, ref_point, data)
        print("point loss", loss, "labels", np.unique(data["point_cls_labels"], return_counts=True))
        for grid in (2, 3):
            print("grid", grid, "loss", record_roi(ref_head_mod, grid, front, data))
    finally:
        torch.matmul, torch.Tensor.cuda = real_matmul, real_cuda
    path = os.path.join(HERE, "pv_rcnn.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
