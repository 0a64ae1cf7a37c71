"""Record the state_dict keys and shapes of the reference's PointHeadVoteSASAStatisticDistillation at the fast_cpc
KITTI and Waymo configs into point_head_state_keys.json (read by tests/test_point_head_cpu.py).

Usage: python tests/golden/make_golden_point_head_keys.py /path/to/reference/checkout

Only the constructor runs, with the stubs of make_golden_sa_keys.py plus stubs for the compiled iou3d_nms and
roiaware_pool3d extensions.  The head configuration is tests/point_head_configs.py."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tsm-det-pointcloud-_amd"))
import make_golden_sa_keys as sa_keys  # noqa: E402
import point_head_configs  # noqa: E402


def install_stubs(ref_root):
    sa_keys.install_stubs(ref_root)
    pc = os.path.join(ref_root, "pcdet")
    sa_keys._pkg("pcdet.models", os.path.join(pc, "models"))
    sa_keys._pkg("pcdet.models.dense_heads", os.path.join(pc, "models", "dense_heads"))
    sa_keys._pkg("pcdet.ops.iou3d_nms", os.path.join(pc, "ops", "iou3d_nms"))
    sa_keys._pkg("pcdet.ops.roiaware_pool3d", os.path.join(pc, "ops", "roiaware_pool3d"))
    sa_keys._pkg("pcdet.ops.iou3d_nms.iou3d_nms_cuda")
    sa_keys._pkg("pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda")


def main(ref_root):
    install_stubs(ref_root)
    from pcdet_amd.config import AttrDict
    real_tensor = torch.tensor

    def cpu_tensor(*a, **kw):
        if str(kw.get("device", "")).startswith("cuda"):
            kw["device"] = "cpu"
        return real_tensor(*a, **kw)

    torch.tensor = cpu_tensor
    try:
        from pcdet.models.dense_heads import point_head_vote_sasa_statistic_distillation as ref
        out = {}
        for name in ("kitti", "waymo"):
            m = ref.PointHeadVoteSASAStatisticDistillation(model_cfg=AttrDict(point_head_configs.head_dict(name)),
                                                           **point_head_configs.head_kwargs())
            out[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    finally:
        torch.tensor = real_tensor
    with open(os.path.join(HERE, "point_head_state_keys.json"), "w") as f:   # one key per line
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(json.dumps(e) for e in entries))
                                   for name, entries in out.items()) + "\n}\n")
    print("wrote", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
