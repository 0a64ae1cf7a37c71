"""Record the state_dict keys and shapes of the reference's StackSAModuleMSG, StackPointnetFPModule and
NeighborVoxelSAModuleMSG at the instances of tests/stack_configs.py into stack_module_state_keys.json (read by
tests/test_pointnet2_stack_ref.py).

Usage: python tests/golden/make_golden_stack_keys.py /path/to/reference/checkout

Only the module constructors run; the compiled CUDA extensions the reference modules import are replaced by the stubs
of make_golden_sa_keys.py.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden_sa_keys import install_stubs  # noqa: E402
from stack_configs import CLASS_OF, INSTANCES  # noqa: E402  (tests/stack_configs.py)


def main(ref_root):
    install_stubs(ref_root)
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules, voxel_pool_modules
    out = {}
    for name, kw in INSTANCES.items():
        cls = getattr(pointnet2_modules, CLASS_OF[name], None) or getattr(voxel_pool_modules, CLASS_OF[name])
        m = cls(**kw())
        out[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "stack_module_state_keys.json"), "w") as f:   # one key per line
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(name), ",\n".join(json.dumps(e) for e in entries))
                                   for name, entries in out.items()) + "\n}\n")
    print("wrote", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1])
