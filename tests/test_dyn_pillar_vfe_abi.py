"""The DynamicPillarVFE entry points (include/spx.h §24) are exported and check their arguments on the host, before any
launch.  No GPU."""
import ctypes


def _fake(n):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def _f(*v):
    return (ctypes.c_float * len(v))(*v)


def _i2(*v):
    return (ctypes.c_int32 * 2)(*v)


def _pillarize(lib, null=None, n=100, stride=5, batch_col=0, xyz_col=1, lo=(0.0, 0.0), vs=(0.16, 0.16), grid=(16, 12),
               batch=2, cap=100, ws_bytes=1 << 24):
    ptrs = _fake(9)                   # points, coords, inverse, count, offset, order, d_num_pillars, d_num_points, ws
    if null is not None:
        ptrs[null] = None
    pts, coords, inv, count, offset, order, d_np, d_npts, ws = ptrs
    return lib.spx_dynamic_pillarize(pts, n, stride, batch_col, xyz_col, None if lo is None else _f(*lo),
                                     None if vs is None else _f(*vs), None if grid is None else _i2(*grid), batch, coords,
                                     inv, count, offset, order, d_np, d_npts, cap, None, ws, ws_bytes, None)


def _geom():
    return _f(0.16, 0.16, 0.08, 0.08, -1.0)


def _fwd(lib, n=100, stride=5, xyz_col=1, c=4, cap=50, c_in=10, c_out=64, use_abs=1, dist=0, training=1, geom=True,
         null=(), ws_bytes=1 << 26):
    names = ("points", "coords", "inverse", "offset", "order", "d_np", "d_npts", "weight", "gamma", "beta", "rm", "rv", "nbt",
             "out", "arg", "pmean", "save_mean", "save_invstd", "stats", "ws")
    p = dict(zip(names, _fake(len(names))))
    for k in null:
        p[k] = None
    return lib.spx_dynamic_pillar_vfe_fwd(p["points"], n, stride, xyz_col, c, p["coords"], p["inverse"], p["offset"],
                                          p["order"], cap, p["d_np"], p["d_npts"], p["weight"], c_in, c_out, p["gamma"],
                                          p["beta"], p["rm"], p["rv"], p["nbt"], 0.01, 1e-3, _geom() if geom else None,
                                          use_abs, dist, training, p["out"], p["arg"], p["pmean"], p["save_mean"],
                                          p["save_invstd"], p["stats"], None, p["ws"], ws_bytes, None)


def _bwd(lib, n=100, stride=5, xyz_col=1, c=4, cap=50, c_in=10, c_out=64, training=1, null=(), ws_bytes=1 << 26):
    names = ("points", "coords", "d_np", "weight", "gamma", "rm", "rv", "out", "arg", "d_out", "pmean", "stats", "d_weight",
             "d_gamma", "d_beta", "ws")
    p = dict(zip(names, _fake(len(names))))
    for k in null:
        p[k] = None
    return lib.spx_dynamic_pillar_vfe_bwd(p["points"], n, stride, xyz_col, c, p["coords"], cap, p["d_np"], p["weight"], c_in,
                                          c_out, p["gamma"], p["rm"], p["rv"], 1e-3, _geom(), 1, 0, training, p["out"],
                                          p["arg"], p["d_out"], p["pmean"], p["stats"], p["d_weight"], p["d_gamma"],
                                          p["d_beta"], p["ws"], ws_bytes, None)


def test_symbols_exported():
    from spx import _lib
    lib = _lib.load()
    for name in ("spx_dynamic_pillarize", "spx_dynamic_pillarize_ws_bytes", "spx_dynamic_pillar_vfe_fwd",
                 "spx_dynamic_pillar_vfe_bwd", "spx_dynamic_pillar_vfe_ws_bytes", "spx_dynamic_pillar_vfe_stats_len"):
        assert hasattr(lib, name), name
    assert lib.spx_dynamic_pillar_vfe_stats_len() >= 13 * 13 + 13 + 2 * 64 + 1
    assert lib.spx_dynamic_pillar_vfe_ws_bytes(720000) >= 256 * 15 * 64 * 8 + (720000 // 64) * 2 * 64 * 12
    # bitmap + ranks over the cells, keys over the points
    assert lib.spx_dynamic_pillarize_ws_bytes(80000, 4, _i2(432, 496), 80000) >= 4 * 432 * 496 * 3 // 16 + 80000 * 4
    assert lib.spx_dynamic_pillarize_ws_bytes(100, 0, _i2(16, 12), 100) == 0
    assert lib.spx_dynamic_pillarize_ws_bytes(100, 2, None, 100) == 0
    assert len(lib.spx_strerror(-10)) > 4 and b"unknown" not in lib.spx_strerror(-10)


def test_pillarize_argument_validation():
    from spx import _lib
    lib = _lib.load()
    bad, too_large, workspace = -1, -5, -2
    for null in range(8):             # every pointer but the workspace
        assert _pillarize(lib, null=null) == bad, null
    assert _pillarize(lib, lo=None) == bad and _pillarize(lib, vs=None) == bad and _pillarize(lib, grid=None) == bad
    for kw in (dict(n=-1), dict(stride=0), dict(xyz_col=-1), dict(xyz_col=4), dict(batch_col=5), dict(batch=0), dict(cap=0),
               dict(cap=-3), dict(grid=(0, 12)), dict(grid=(16, -1)), dict(vs=(0.0, 0.16)), dict(vs=(0.16, -1.0))):
        assert _pillarize(lib, **kw) == bad, kw
    assert _pillarize(lib, n=1 << 31) == too_large and _pillarize(lib, cap=1 << 31) == too_large
    assert _pillarize(lib, batch=8, grid=(1 << 14, 1 << 14)) == too_large        # the cell key is an int32
    assert _pillarize(lib, null=8) == workspace and _pillarize(lib, ws_bytes=64) == workspace


def test_pfn_argument_validation():
    from spx import _lib
    lib = _lib.load()
    bad, unsupported, workspace = -1, -3, -2
    assert b"unsupported" in lib.spx_strerror(unsupported).lower()
    for kw in (dict(c=2), dict(c=7), dict(c_in=11), dict(c_in=7, use_abs=0, dist=1), dict(n=-1), dict(cap=0), dict(stride=4),
               dict(xyz_col=-1), dict(geom=False), dict(null=("weight",)), dict(null=("gamma",)), dict(null=("beta",)),
               dict(null=("coords",)), dict(null=("offset",)), dict(null=("d_np",)), dict(null=("d_npts",)),
               dict(null=("out",)), dict(null=("arg",)), dict(null=("pmean",)), dict(null=("points",)),
               dict(null=("inverse",)), dict(null=("order",)), dict(null=("stats",)), dict(null=("save_mean",)),
               dict(training=0, null=("rm", "rv")), dict(null=("rm",))):
        assert _fwd(lib, **kw) == bad, kw
    for kw in (dict(c=7), dict(c_in=9), dict(cap=0), dict(null=("stats",)), dict(training=0, null=("rm",)),
               dict(null=("d_weight",)), dict(null=("d_gamma",)), dict(null=("d_beta",)), dict(null=("arg",)),
               dict(null=("pmean",)), dict(null=("d_out",)), dict(null=("d_np",)), dict(null=("points",))):
        assert _bwd(lib, **kw) == bad, kw
    assert _fwd(lib, c_out=128) == unsupported and _bwd(lib, c_out=16) == unsupported
    assert _fwd(lib, null=("ws",)) == workspace and _fwd(lib, ws_bytes=16) == workspace
    assert _bwd(lib, null=("ws",)) == workspace and _bwd(lib, ws_bytes=8) == workspace
    assert _fwd(lib, stride=6, c=5, c_in=9, use_abs=0, dist=1, null=("ws",)) == workspace    # a valid layout gets past the checks
