"""Dense post-processing (include/spx.h §29) without a GPU: the restatement's selection against the one of
tests/post_process_ref.py, the exported symbols and their host-side argument checks, the operator layer's checks, and
the opt-in logic of the detector layer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dense_post_process_ref as dref
import post_process_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(6))
def test_selection_equals_the_point_restatement(seed):
    g = torch.Generator().manual_seed(seed)
    b, n = 1 + seed % 3, (1, 70, 513, 4096, 1000, 64)[seed]
    scores = torch.randint(0, 33, (b * n,), generator=g).float() / 32          # ties
    labels = torch.randint(1, 5, (b * n,), generator=g)
    for thresholds, per_class, pre_max in (([0.5, 0.25, 0.25], True, 16), ([0.25], False, 100), ([0.0] * 4, True, 5000)):
        cand, count = dref.select(scores, labels, b, thresholds, pre_max, per_class=per_class)
        s, lab = scores.numpy(), labels.numpy()
        for f in range(b):
            fs, fl = s[f * n:(f + 1) * n], lab[f * n:(f + 1) * n]
            for c, t in enumerate(thresholds):
                member = fs >= np.float32(t)
                if per_class:
                    member &= fl == c + 1
                want = ref._ordered(np.nonzero(member)[0], fs)[:pre_max] + f * n
                assert count[f, c] == len(want)
                assert np.array_equal(cand[f, c, :len(want)], want) and (cand[f, c, len(want):] == -1).all()


def test_restatement_nan_and_signed_zero():
    scores = torch.tensor([0.0, float("nan"), -0.0, -1.0, 0.0, 2.0])
    cand, count = dref.select(scores, torch.ones(6, dtype=torch.int64), 1, None, 8, per_class=False)
    assert count.tolist() == [[5]] and cand[0, 0].tolist() == [5, 0, 2, 4, 3, -1, -1, -1]
    cand, count = dref.select(scores, torch.ones(6, dtype=torch.int64), 1, [0.0], 2, per_class=False)
    assert count.tolist() == [[2]] and cand[0, 0].tolist() == [5, 0]


def _fake(n=1):
    return [ctypes.c_void_p(4096 + 256 * i) for i in range(n)]


def test_symbols_exported_with_the_declared_signatures():
    from spx import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "spx.h")).read()
    want = {"spx_dense_select_ws_bytes": 4, "spx_dense_select": 13, "spx_dense_post_process_ws_bytes": 5,
            "spx_dense_post_process": 21}
    for name, nargs in want.items():
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert lib.spx_abi_version() == 3
    small = lib.spx_dense_post_process_ws_bytes(4, 211200, 3, 4096, 500)
    assert small >= 4 * 3 * 4096 * 64 * 8                       # the bit matrices
    assert lib.spx_dense_select_ws_bytes(4, 211200, 3, 4096) < small


def test_c_argument_validation():
    from spx import _lib
    lib = _lib.load()

    def select(b=2, n=1000, th=(0.3, 0.3, 0.3), pre_max=16, per_class=1, null=None, ws_bytes=1 << 30):
        ptrs = _fake(5)
        if null is not None:
            ptrs[null] = None
        scores, labels, cand, cnt, ws = ptrs
        return lib.spx_dense_select(scores, labels, b, n, _lib.f_arr(th), len(th), pre_max, per_class, cand, cnt, ws,
                                    ws_bytes, None)

    def post(b=2, n=1000, th=(0.3, 0.3, 0.3), pre_max=16, post_max=8, per_class=1, ld=7, null=None, ws_bytes=1 << 30):
        ptrs = _fake(9)
        if null is not None:
            ptrs[null] = None
        scores, labels, boxes, sel, count, ob, osc, ol, ws = ptrs
        return lib.spx_dense_post_process(scores, labels, boxes, ld, b, n, _lib.f_arr(th), len(th), 0.1, pre_max, post_max,
                                          0, per_class, sel, count, ob, osc, ol, ws, ws_bytes, None)

    for null in range(4):
        assert select(null=null) == -1, null
    for null in range(8):
        assert post(null=null) == -1, null
    assert select(null=4) == -2 and post(null=8) == -2 and select(ws_bytes=16) == -2 and post(ws_bytes=16) == -2
    for f in (select, post):
        assert f(b=-1) == -1 and f(n=-1) == -1 and f(pre_max=0) == -1
        assert f(th=(0.3, 0.3), per_class=0) == -1
        assert f(th=(0.3,) * 9) == -3
        assert f(pre_max=16385) == -5                               # SPX_ERR_TOO_LARGE
        assert f(b=2, n=1 << 30) == -5                              # b * n >= 2^31
        assert f(b=0) == 0
    assert select(n=0) == 0                                         # nothing to do, nothing launched
    assert post(post_max=0) == -1 and post(ld=6) == -1
    assert post(th=(0.3,) * 8, pre_max=4096, post_max=513, n=100000) == -5      # 8 x 513 survivors > 4096
    assert post(th=(0.3,), per_class=0, pre_max=9000, post_max=4097, n=100000) == -5


def test_ops_check_arguments_before_touching_the_device():
    from spx import _lib, ops
    assert ops.DENSE_POST_PROCESS_MAX_PRE == 16384 and ops.POST_PROCESS_MAX_N == 4096
    s, lab, bx = torch.rand(8), torch.ones(8, dtype=torch.int64), torch.rand(8, 7)
    with pytest.raises(_lib.SpxError, match="GPU"):
        ops.dense_select(s, lab, 2, [0.3], 4, per_class=False)
    with pytest.raises(_lib.SpxError, match="GPU"):
        ops.dense_post_process(s, lab, bx, 2, [0.3, 0.3, 0.3], 0.1, 16, 8)
    for bad in (lambda: ops.dense_select(s, lab[:-1], 2, [0.3], 4, per_class=False),
                lambda: ops.dense_select(s, lab, 3, [0.3], 4, per_class=False),               # 8 rows, 3 frames
                lambda: ops.dense_select(s, lab, 2, [0.3, 0.3], 4, per_class=False),
                lambda: ops.dense_select(s, lab, 2, [0.3] * 9, 4),
                lambda: ops.dense_select(s, lab, 2, [0.3], 0, per_class=False),
                lambda: ops.dense_select(s, lab, 2, [0.3], 16385, per_class=False),
                lambda: ops.dense_select(s, lab, 2, None, 4, per_class=True),
                lambda: ops.dense_post_process(s, lab, bx[:, :6], 2, [0.3], 0.1, 16, 8, per_class=False),
                lambda: ops.dense_post_process(s, lab, bx[:-1], 2, [0.3], 0.1, 16, 8, per_class=False),
                lambda: ops.dense_post_process(s, lab, bx, 2, [0.3], 0.1, 16, 0, per_class=False),
                lambda: ops.dense_post_process(s, lab, bx, 2, [0.3], 0.1, 16385, 8, per_class=False),
                lambda: ops.dense_post_process(torch.rand(20000), torch.ones(20000, dtype=torch.int64),
                                               torch.rand(20000, 7), 1, [0.3] * 8, 0.1, 4096, 513)):
        with pytest.raises(_lib.SpxError) as e:
            bad()
        assert "GPU" not in str(e.value)


class _Template(object):
    """Just enough of a detector for Detector3DTemplate's plan logic."""
    num_class = 3

    def __init__(self, **post):
        from pcdet_amd.config import AttrDict
        cfg = dict(SCORE_THRESH=[0.1, 0.1, 0.1], NMS_CONFIG=dict(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu",
                                                                 NMS_THRESH=0.01, NMS_PRE_MAXSIZE=4096,
                                                                 NMS_POST_MAXSIZE=500))
        cfg.update(post)
        self.model_cfg = AttrDict(POST_PROCESSING=cfg)


def _plan(batch, dense=None, **post):
    from pcdet_amd.models.detectors.detector3d_template import Detector3DTemplate
    t = _Template(**post)
    t._FUSED_NMS_TYPES = Detector3DTemplate._FUSED_NMS_TYPES
    t._dense_post_plan = lambda bd: Detector3DTemplate._dense_post_plan(t, bd)
    return Detector3DTemplate._fused_post_plan(t, batch, **({} if dense is None else {"dense": dense}))


def test_dense_predictions_give_a_plan_only_when_asked():
    meta = torch.device("meta")

    class Fake(torch.Tensor):
        """A meta tensor that says it lives on the GPU: the plan reads shapes and flags only."""
        is_cuda = True

    def fake(*shape):
        return torch.empty(shape, device=meta).as_subclass(Fake)

    batch = dict(batch_size=2, batch_box_preds=fake(2, 7680, 7), batch_cls_preds=fake(2, 7680, 3))
    assert _plan(batch) is None                                     # FUSED absent
    assert _plan(batch, FUSED=False) is None
    plan = _plan(batch, FUSED=True)
    assert plan is not None and plan["dense"] and plan["n"] == 7680 and plan["per_class"] and plan["pre_max"] == 4096
    assert _plan(batch, dense=True)["thresholds"] == [0.1, 0.1, 0.1]
    assert _plan(batch, FUSED=True, SCORE_THRESH=0.1)["per_class"] is False
    assert _plan(dict(batch, batch_cls_preds=fake(2, 7680, 2)), FUSED=True) is None       # neither 1 nor num_class columns
    assert _plan(dict(batch, batch_cls_preds=fake(2, 7000, 3)), FUSED=True) is None
    nms = dict(MULTI_CLASSES_NMS=False, NMS_TYPE="nms_gpu", NMS_THRESH=0.01, NMS_PRE_MAXSIZE=20000, NMS_POST_MAXSIZE=500)
    assert _plan(batch, FUSED=True, NMS_CONFIG=nms) is None         # beyond DENSE_POST_PROCESS_MAX_PRE
    assert _plan(batch, FUSED=True, NMS_CONFIG=dict(nms, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=2000)) is None
    assert _plan(batch, FUSED=True, NMS_CONFIG=dict(nms, NMS_PRE_MAXSIZE=4096, NMS_TYPE="circle_nms")) is None
    assert _plan(batch, FUSED=True, NMS_CONFIG=dict(nms, NMS_PRE_MAXSIZE=4096, MULTI_CLASSES_NMS=True)) is None
    # flat point-head predictions keep their own rules: FUSED is not needed, n is limited
    flat = dict(batch_size=2, batch_index=fake(1024), batch_box_preds=fake(1024, 7), batch_cls_preds=fake(1024, 3))
    assert _plan(flat) is not None and "dense" not in _plan(flat)
    assert _plan(dict(flat, batch_index=fake(10000), batch_box_preds=fake(10000, 7), batch_cls_preds=fake(10000, 3)),
                 FUSED=True) is None


def test_proposal_layer_without_fused_calls_topk(monkeypatch):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads.roi_head_template import RoIHeadTemplate
    from spx import ops
    head = RoIHeadTemplate.__new__(RoIHeadTemplate)
    calls = []

    class Stop(Exception):
        pass

    def topk(*a, **k):
        calls.append("topk")
        raise Stop()

    def dense(*a, **k):
        calls.append("dense")
        raise Stop()

    monkeypatch.setattr(torch, "topk", topk)
    monkeypatch.setattr(ops, "dense_post_process", dense)
    batch = dict(batch_size=1, batch_box_preds=torch.zeros(1, 4, 7), batch_cls_preds=torch.zeros(1, 4, 3))
    nms = AttrDict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=4, NMS_POST_MAXSIZE=2, NMS_THRESH=0.5)
    with pytest.raises(Stop):
        head.proposal_layer(dict(batch), nms)
    assert calls == ["topk"]
    with pytest.raises(Stop):
        head.proposal_layer(dict(batch), AttrDict(dict(nms, FUSED=False)))
    assert calls == ["topk", "topk"]
    with pytest.raises(Stop):
        head.proposal_layer(dict(batch), AttrDict(dict(nms, FUSED=True)))
    assert calls == ["topk", "topk", "dense"]
