"""Record the state_dict keys and shapes of the reference's VoxelPointnetSAModuleFSMSGDistillation at the four fast_cpc
instances into sa_module_state_keys.json (read by tests/test_sa_module_keys.py).

Usage: python tests/golden/make_golden_sa_keys.py /path/to/reference/checkout

Only the module constructors run.  The compiled CUDA extensions the reference modules import, SharedArray and spconv
are replaced by stubs; the spconv stub builds parameters in the spconv 2.x layout (weight (out, kz, ky, kx, in), bias
(out,)).  The constructors' torch.tensor(..., device='cuda:0') calls are redirected to the CPU.
"""
import json
import os
import sys
import types

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from sa_configs import INSTANCES  # noqa: E402  (tests/sa_configs.py: the fast_cpc SA settings)


def _pkg(name, path=None):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    sys.modules[name] = m
    return m


class _SparseModule(nn.Module):
    pass


class _SparseConv(_SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, **kw):
        super().__init__()
        k = (kernel_size,) * 3 if isinstance(kernel_size, int) else tuple(kernel_size)
        self.weight = nn.Parameter(torch.empty(out_channels, *k, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None


class _SparseInverseConv(_SparseConv):
    def __init__(self, in_channels, out_channels, kernel_size, indice_key=None, bias=True, **kw):
        super().__init__(in_channels, out_channels, kernel_size, bias=bias)


class _SparseSequential(_SparseModule):
    def __init__(self, *mods):
        super().__init__()
        for i, m in enumerate(mods):
            self.add_module(str(i), m)


def install_stubs(ref_root):
    pc = os.path.join(ref_root, "pcdet")
    _pkg("pcdet", pc)
    _pkg("pcdet.ops", os.path.join(pc, "ops"))
    _pkg("pcdet.ops.pointnet2", os.path.join(pc, "ops", "pointnet2"))
    _pkg("pcdet.ops.pointnet2.pointnet2_batch", os.path.join(pc, "ops", "pointnet2", "pointnet2_batch"))
    _pkg("pcdet.ops.pointnet2.pointnet2_stack", os.path.join(pc, "ops", "pointnet2", "pointnet2_stack"))
    _pkg("pcdet.utils", os.path.join(pc, "utils"))
    _pkg("pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda")
    _pkg("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda")
    _pkg("SharedArray")
    sp = _pkg("spconv", "")
    spp = _pkg("spconv.pytorch", "")
    for m in (sp, spp):
        m.SparseModule = _SparseModule
        m.SubMConv3d = _SparseConv
        m.SparseConv3d = _SparseConv
        m.SparseInverseConv3d = _SparseInverseConv
        m.SparseSequential = _SparseSequential
        m.SparseConvTensor = object
    sp.pytorch = spp
    for name in ("spconv.core_cc", "spconv.core_cc.csrc", "spconv.core_cc.csrc.sparse", "spconv.core_cc.csrc.sparse.all"):
        _pkg(name, "")
    _pkg("spconv.core_cc.csrc.sparse.all.ops3d").Point2Voxel = object
    _pkg("spconv.core_cc.csrc.sparse.all.ops_cpu3d").Point2VoxelCPU = object


def main(ref_root):
    install_stubs(ref_root)
    real_tensor = torch.tensor

    def cpu_tensor(*a, **kw):
        if str(kw.get("device", "")).startswith("cuda"):
            kw["device"] = "cpu"
        return real_tensor(*a, **kw)

    torch.tensor = cpu_tensor
    try:
        from pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as ref
        out = {}
        for name, kw in INSTANCES.items():
            m = ref.VoxelPointnetSAModuleFSMSGDistillation(**kw())
            out[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    finally:
        torch.tensor = real_tensor
    with open(os.path.join(HERE, "sa_module_state_keys.json"), "w") as f:   # one key per line
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(json.dumps(e) for e in entries))
                                   for name, entries in out.items()) + "\n}\n")
    print("wrote", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
