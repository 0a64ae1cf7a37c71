"""The post-processing entry points (include/spx.h §15) are exported and check their arguments on the host, before any
launch, so this runs without a GPU."""
import ctypes

import pytest
import torch


def _fake(n=1):
    """Non-null device-pointer stand-ins: the argument checks return before anything is dereferenced."""
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def _post(lib, _lib, b=2, n=64, thresholds=(0.3, 0.3, 0.3), pre_max=16, post_max=8, per_class=1, null=None):
    ptrs = _fake(9)
    if null is not None:
        ptrs[null] = None
    scores, labels, boxes, sel, count, ob, osc, ol, ws = ptrs
    th = _lib.f_arr(thresholds) if thresholds is not None else None
    return lib.spx_point_post_process(scores, labels, boxes, b, n, th, len(thresholds or ()), 0.1, pre_max, post_max, 0,
                                      per_class, sel, count, ob, osc, ol, ws, 1 << 20, None)


def test_symbols_exported_and_capacity():
    from spx import _lib
    lib = _lib.load()
    for name in ("spx_point_post_process", "spx_point_post_process_ws_bytes", "spx_point_post_process_capacity",
                 "spx_recall_count"):
        assert hasattr(lib, name), name
    assert lib.spx_point_post_process_capacity(512, 3, 512, 1) == 512
    assert lib.spx_point_post_process_capacity(3072, 3, 500, 1) == 1500
    assert lib.spx_point_post_process_capacity(3072, 1, 500, 0) == 500
    assert lib.spx_point_post_process_capacity(7, 3, 4, 1) == 7
    assert lib.spx_point_post_process_ws_bytes(4, 3072, 3, 500) >= 4 * 3 * 500 * 8 + 4 * 3 * 4


def test_post_process_argument_validation():
    from spx import _lib
    lib = _lib.load()
    for null in range(8):                       # every input and output pointer
        assert _post(lib, _lib, null=null) == -1, null
    assert _post(lib, _lib, thresholds=None) == -1
    assert _post(lib, _lib, b=-1) == -1
    assert _post(lib, _lib, n=-1) == -1
    assert _post(lib, _lib, pre_max=0) == -1
    assert _post(lib, _lib, pre_max=-3) == -1
    assert _post(lib, _lib, post_max=0) == -1
    assert _post(lib, _lib, post_max=-1) == -1
    assert _post(lib, _lib, thresholds=(0.3, 0.3), per_class=0) == -1       # agnostic mode takes one threshold
    assert _post(lib, _lib, thresholds=(0.3,) * 9) == -3                    # more than 8 thresholds
    assert _post(lib, _lib, n=4097) == -5                                   # SPX_ERR_TOO_LARGE
    assert _post(lib, _lib, n=1 << 20) == -5
    assert _post(lib, _lib, b=0) == 0                                       # nothing to do, nothing launched
    assert _post(lib, _lib, null=8) == -2                                   # no workspace


def test_recall_count_argument_validation():
    from spx import _lib
    lib = _lib.load()
    ob, cnt, gt, rec, ng = _fake(5)
    th = _lib.f_arr([0.3, 0.5, 0.7])

    def call(ob=ob, cnt=cnt, b=2, cap=8, gt=gt, g=4, ld=8, th=th, nt=3, rec=rec, ng=ng):
        return lib.spx_recall_count(ob, cnt, b, cap, gt, g, ld, th, nt, rec, ng, None)

    assert call(ob=None) == -1 and call(cnt=None) == -1 and call(gt=None) == -1 and call(th=None) == -1
    assert call(rec=None) == -1 and call(ng=None) == -1
    assert call(b=-1) == -1 and call(cap=-1) == -1 and call(g=-1) == -1 and call(ld=6) == -1 and call(nt=0) == -1
    assert call(nt=9, th=_lib.f_arr([0.5] * 9)) == -3
    assert call(b=0) == 0


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from spx import _lib, ops
    scores, labels, boxes = torch.rand(8), torch.ones(8, dtype=torch.int64), torch.rand(8, 7)
    with pytest.raises(_lib.SpxError):
        ops.point_post_process(scores, labels, boxes, 2, [0.3, 0.3, 0.3], 0.1, 16, 8)
    with pytest.raises(_lib.SpxError):
        ops.recall_count(torch.zeros(2, 4, 7), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3, 8), [0.3, 0.5, 0.7])
    assert ops.POST_PROCESS_MAX_N == 4096
