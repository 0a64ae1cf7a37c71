"""The voxel-grid pooling entry points (include/spx.h §27) are exported with the documented signatures and check their
arguments on the host, before any launch; the tensor-level ops refuse CPU tensors.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spx_voxel_pool_moments_ws_bytes", "spx_voxel_pool_moments", "spx_voxel_pool_max_fwd",
         "spx_voxel_pool_max_bwd_ws_bytes", "spx_voxel_pool_max_bwd")
BAD, WORKSPACE, TOO_LARGE = -1, -2, -5


def _fake(names):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return {k: ctypes.c_void_p(4096 + 256 * i) for i, k in enumerate(names)}


def _moments(lib, null=(), n_src=10, m=6, s=4, ws_bytes=1 << 20):
    p = _fake(("xyz", "new_xyz", "idx", "empty", "out", "ws"))
    for k in null:
        p[k] = None
    return lib.spx_voxel_pool_moments(p["xyz"], p["new_xyz"], p["idx"], p["empty"], n_src, m, s, p["out"], p["ws"],
                                      ws_bytes, None)


def _fwd(lib, null=(), c=8, n_src=10, m=6, s=4):
    p = _fake(("f", "xyz", "new_xyz", "idx", "empty", "a", "b", "out", "arg"))
    for k in null:
        p[k] = None
    return lib.spx_voxel_pool_max_fwd(p["f"], p["xyz"], p["new_xyz"], p["idx"], p["empty"], p["a"], p["b"], c, n_src, m, s,
                                      p["out"], p["arg"], None)


def _bwd(lib, null=(), c=8, n_src=10, m=6, s=4, ws_bytes=1 << 24):
    p = _fake(("dout", "arg", "idx", "empty", "xyz", "new_xyz", "df", "da", "db", "ws"))
    for k in null:
        p[k] = None
    return lib.spx_voxel_pool_max_bwd(p["dout"], p["arg"], p["idx"], p["empty"], p["xyz"], p["new_xyz"], c, n_src, m, s,
                                      p["df"], p["da"], p["db"], p["ws"], ws_bytes, None)


def test_symbols_exported_and_declared():
    from spx import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spx.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(params.split(",")), name
    assert lib.spx_voxel_pool_moments_ws_bytes(110592, 16) >= (110592 * 16 // 2048) * 9 * 8
    assert lib.spx_voxel_pool_moments_ws_bytes(-1, 16) == 0
    assert lib.spx_voxel_pool_max_bwd_ws_bytes(32, 80000, 110592, 16) >= 4 * 110592 * 16 * 4 + 2 * 80000 * 4
    assert lib.spx_voxel_pool_max_bwd_ws_bytes(0, 80000, 110592, 16) == 0


def test_moments_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for kw in (dict(null=("new_xyz",)), dict(null=("idx",)), dict(null=("xyz",)), dict(null=("out",)), dict(s=0), dict(m=-1),
               dict(n_src=-1)):
        assert _moments(lib, **kw) == BAD, kw
    assert _moments(lib, null=("ws",)) == WORKSPACE and _moments(lib, ws_bytes=8) == WORKSPACE
    assert _moments(lib, m=1 << 28, s=16) == TOO_LARGE
    assert _moments(lib, null=("empty",), ws_bytes=0) == WORKSPACE          # empty may be NULL; the workspace may not


def test_max_fwd_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for null in ("f", "xyz", "new_xyz", "idx", "a", "b", "out", "arg"):
        assert _fwd(lib, null=(null,)) == BAD, null
    for kw in (dict(c=0), dict(s=0), dict(m=-1), dict(n_src=-1), dict(c=-3)):
        assert _fwd(lib, **kw) == BAD, kw
    assert _fwd(lib, m=1 << 28, s=16) == TOO_LARGE and _fwd(lib, m=1 << 26, c=64) == TOO_LARGE
    assert _fwd(lib, c=1 << 16) == TOO_LARGE
    assert _fwd(lib, m=0) == 0 and _fwd(lib, m=0, null=("out", "arg", "f")) == 0


def test_max_bwd_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for null in ("dout", "arg", "idx", "xyz", "new_xyz"):
        assert _bwd(lib, null=(null,)) == BAD, null
    assert _bwd(lib, null=("df", "da", "db")) == BAD
    for kw in (dict(c=0), dict(s=0), dict(m=-1), dict(n_src=-1)):
        assert _bwd(lib, **kw) == BAD, kw
    assert _bwd(lib, null=("ws",)) == WORKSPACE and _bwd(lib, ws_bytes=64) == WORKSPACE
    assert _bwd(lib, m=1 << 28, s=16) == TOO_LARGE


def test_ops_refuse_cpu_tensors():
    from spx import _lib, ops
    f, xyz, new_xyz = torch.zeros(5, 4), torch.zeros(5, 3), torch.zeros(3, 3)
    idx, empty = torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, dtype=torch.bool)
    a, b = torch.zeros(4, 3), torch.zeros(4)
    with pytest.raises(_lib.SpxError):
        ops.voxel_pool_moments(xyz, new_xyz, idx, empty)
    with pytest.raises(_lib.SpxError):
        ops.voxel_pool_max(f, xyz, new_xyz, idx, empty, a, b)
    with pytest.raises(_lib.SpxError):
        ops.voxel_pool_max_bwd(torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.int32), xyz, new_xyz, idx, empty, 5)
