"""The two-layer SA-MLP pooling entry point (include/spx.h §28) is exported with the documented signature and checks its
arguments on the host, before any launch; the tensor-level op refuses CPU tensors.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spx_sa_mlp2_max",)
BAD, UNSUPPORTED, TOO_LARGE = -1, -3, -5
PTRS = ("p", "xyz", "new_xyz", "idx", "empty", "wx", "a1", "b1", "w2", "a2", "b2", "out")


def _call(lib, null=(), c1=16, c2=16, n_src=10, m=6, s=16, misalign_p=False):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    p = {k: ctypes.c_void_p(4096 + 256 * i) for i, k in enumerate(PTRS)}
    if misalign_p:
        p["p"] = ctypes.c_void_p(4096 + 4)
    for k in null:
        p[k] = None
    return lib.spx_sa_mlp2_max(p["p"], p["xyz"], p["new_xyz"], p["idx"], p["empty"], p["wx"], p["a1"], p["b1"], p["w2"],
                               p["a2"], p["b2"], c1, c2, n_src, m, s, p["out"], None)


def test_symbols_exported_and_declared():
    from spx import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spx.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(params.split(",")), name
    res, args = _lib.SIGNATURES["spx_sa_mlp2_max"]
    assert res is ctypes.c_int and args[:11] == [ctypes.c_void_p] * 11
    assert args[11:16] == [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]


def test_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for null in ("xyz", "new_xyz", "idx", "wx", "a1", "b1", "w2", "a2", "b2", "out"):
        assert _call(lib, null=(null,)) == BAD, null
    for kw in (dict(c1=0), dict(c2=-16), dict(s=0), dict(m=-1), dict(n_src=-1), dict(misalign_p=True)):
        assert _call(lib, **kw) == BAD, kw
    for kw in (dict(c1=24), dict(c2=48), dict(c1=128), dict(s=8), dict(s=17), dict(s=64)):
        assert _call(lib, **kw) == UNSUPPORTED, kw
    assert _call(lib, m=1 << 28, s=16) == TOO_LARGE and _call(lib, m=1 << 26, c2=64) == TOO_LARGE
    assert _call(lib, n_src=1 << 31) == TOO_LARGE
    assert _call(lib, m=0) == 0 and _call(lib, m=0, null=PTRS) == 0
    assert b"" != lib.spx_strerror(UNSUPPORTED)


def test_op_refuses_cpu_tensors_and_is_listed():
    from spx import _lib, ops
    xyz, new_xyz = torch.zeros(5, 3), torch.zeros(3, 3)
    idx, empty = torch.zeros(3, 16, dtype=torch.int32), torch.zeros(3, dtype=torch.bool)
    with pytest.raises(_lib.SpxError):
        ops.sa_mlp2_max(torch.zeros(5, 16), xyz, new_xyz, idx, empty, torch.zeros(16, 3), torch.zeros(16), torch.zeros(16),
                        torch.zeros(16, 16), torch.zeros(16), torch.zeros(16))
    assert ops.sa_mlp2_supported(64, 16, 32) and ops.sa_mlp2_supported(16, 64, 16)
    assert not ops.sa_mlp2_supported(24, 16, 16) and not ops.sa_mlp2_supported(16, 16, 8)
    assert not ops.sa_mlp2_supported(16, 128, 16)
