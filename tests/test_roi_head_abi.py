"""The second-stage entry points (include/spx.h §25, §26) are exported with the documented signatures and check their
arguments on the host, before any launch.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake(n):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def _pool(lib, null=(), batch=2, n=5, stride=7, c=8, h=5, w=7, strides=(280, 35, 7, 1), g=7, step=(0.4, 0.4)):
    p = dict(zip(("rois", "d_n", "features", "out"), _fake(4)))
    for k in null:
        p[k] = None
    return lib.spx_roi_grid_pool_bev(p["rois"], batch, n, stride, p["d_n"], p["features"], c, h, w, *strides, g, 0.0, -1.0,
                                     step[0], step[1], p["out"], None)


def _sample(lib, null=(), batch=2, r=16, rs=7, gmax=4, gs=8, m=8, fg=4, ratio=0.8, ws_bytes=1 << 20):
    names = ("rois", "labels", "gt", "keys", "u", "sampled", "ious", "gt_inds", "ws")
    p = dict(zip(names, _fake(len(names))))
    for k in null:
        p[k] = None
    return lib.spx_proposal_sample(p["rois"], p["labels"], p["gt"], batch, r, rs, gmax, gs, m, fg, 0.55, 0.75, 0.1, ratio, 1,
                                   p["keys"], p["u"], p["sampled"], p["ious"], p["gt_inds"], p["ws"], ws_bytes, None)


def test_symbols_exported_and_declared():
    from spx import _lib
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spx.h")).read(), flags=re.S)
    for name in ("spx_roi_grid_pool_bev", "spx_proposal_sample", "spx_proposal_sample_ws_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    # the binding's argument count equals the header's parameter count
    for name in ("spx_roi_grid_pool_bev", "spx_proposal_sample", "spx_proposal_sample_ws_bytes"):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(params.split(",")), name
    pool = _lib.SIGNATURES["spx_roi_grid_pool_bev"][1]
    assert pool[14:18] == [ctypes.c_double] * 4 and pool[9:13] == [ctypes.c_int64] * 4      # range / step, the strides
    assert _lib.SIGNATURES["spx_proposal_sample"][1][13] is ctypes.c_double                   # HARD_BG_RATIO
    assert lib.spx_proposal_sample_ws_bytes(4, 512, 50) >= 4 * 512 * 50 * 4
    assert lib.spx_proposal_sample_ws_bytes(0, 512, 50) == 0


def test_roi_grid_pool_argument_validation():
    from spx import _lib
    lib = _lib.load()
    bad, unsupported = -1, -3
    for kw in (dict(null=("rois",)), dict(null=("features",)), dict(null=("out",)), dict(stride=6), dict(c=0), dict(h=1),
               dict(w=1), dict(g=0), dict(step=(0.0, 0.4)), dict(step=(0.4, -1.0)), dict(step=(float("nan"), 0.4)),
               dict(strides=(280, 0, 7, 1)), dict(strides=(280, 35, 0, 1)), dict(strides=(280, 35, 7, 0)), dict(batch=-1),
               dict(n=-1)):
        assert _pool(lib, **kw) == bad, kw
    assert _pool(lib, g=13) == unsupported
    assert _pool(lib, batch=0) == 0 and _pool(lib, n=0) == 0 and _pool(lib, n=0, null=("rois", "out")) == 0
    assert _pool(lib, n=1 << 31) == -5


def test_proposal_sample_argument_validation():
    from spx import _lib
    lib = _lib.load()
    bad, workspace, too_large = -1, -2, -5
    for null in ("rois", "labels", "gt", "keys", "u", "sampled", "ious", "gt_inds"):
        assert _sample(lib, null=(null,)) == bad, null
    for kw in (dict(r=0), dict(rs=6), dict(gmax=0), dict(gs=7), dict(m=0), dict(fg=-1), dict(fg=9), dict(ratio=-0.1),
               dict(ratio=1.5), dict(ratio=float("nan")), dict(batch=-1)):
        assert _sample(lib, **kw) == bad, kw
    assert _sample(lib, r=2049) == too_large and _sample(lib, batch=1 << 20, r=2048, gmax=1 << 10) == too_large
    assert _sample(lib, null=("ws",)) == workspace and _sample(lib, ws_bytes=16) == workspace
    assert _sample(lib, batch=0) == 0
