"""Post-processing of dense predictions without a host read (csrc/dense_post_process.hip, include/spx.h §29) on the GPU.

spx_dense_select and spx_dense_post_process against the plain restatement (tests/dense_post_process_ref.py), exactly:
every comparison is an integer decision or a copied value, so there is no tolerance anywhere.  The selection cases aim
at what a radix select can get wrong: ties that straddle the cut, scores that share their leading bits, all scores
equal, negative scores and -0.0, NaN, members fewer than / equal to / more than pre_max, a class without a member, and
sizes on both sides of a workgroup's row range, of the 64-box word and of the LDS sort's power of two.  The NMS cases
aim at the bit matrix and its greedy walk: chains across the 64-box word boundary, identical boxes, disjoint boxes with
the early stop at post_max, survivors that cross classes.  At n <= 4096 the op must equal §15's in every output."""
import ctypes

import numpy as np
import pytest
import torch

import dense_post_process_ref as dref
import post_process_ref as ref
from test_gpu_post_process import NMS_THRESH, THRESH, check_against, make_inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PRE_MAX = (1, 64, 65, 4096, 4097, 9000, 16384)


def _scores(kind, rows, gen):
    if kind == "ties":            # 65 distinct values: every cut falls inside a run of equal scores
        return torch.randint(0, 65, (rows,), generator=gen).float() / 64
    if kind == "equal":
        return torch.full((rows,), 0.625)
    if kind == "top_bits":        # 0.5 + k 2^-24: the leading 20 bits are shared, and values repeat
        return 0.5 + torch.randint(0, 4096, (rows,), generator=gen).float() * 2.0 ** -24
    if kind == "top_bits24":      # 0.5 + k 2^-24, k < 256: the leading 24 bits are shared, 256 distinct values
        return 0.5 + torch.randint(0, 256, (rows,), generator=gen).float() * 2.0 ** -24
    if kind == "signed":          # logits: negative values, +0.0 and -0.0
        s = torch.randn(rows, generator=gen)
        s[torch.rand(rows, generator=gen) < 0.1] = 0.0
        s[torch.rand(rows, generator=gen) < 0.1] = -0.0
        return s
    if kind == "nan":
        s = torch.rand(rows, generator=gen)
        s[torch.rand(rows, generator=gen) < 0.2] = float("nan")
        return s
    raise KeyError(kind)


def _check_select(scores, labels, b, thresholds, pre_max, per_class, full=None):
    """full: the restatement's answer for a larger pre_max (its first pre_max columns are the answer for this one)."""
    from spx import ops
    cand, count = ops.dense_select(scores, labels, b, thresholds, pre_max, per_class=per_class)
    if full is None:
        want_cand, want_count = dref.select(scores, labels, b, thresholds, pre_max, per_class=per_class)
    else:
        want_cand, want_count = full[0][:, :, :pre_max], np.minimum(full[1], pre_max)
    assert cand.dtype == torch.int64 and count.dtype == torch.int32
    assert tuple(cand.shape) == want_cand.shape and tuple(count.shape) == want_count.shape
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(cand.cpu().numpy(), want_cand)
    return want_count


SELECT_CASES = (("ties", [0.5], False), ("ties", [0.5, 0.25, 0.25], True), ("ties", [0.5] + [0.25] * 7, True),
                ("top_bits", [0.5], False), ("top_bits24", [0.5], False), ("top_bits24", [0.5, 0.5, 0.5], True),
                ("equal", [0.5, 0.25, 0.25], True), ("nan", [0.5, 0.25, 0.25], True),
                ("nan", None, False), ("signed", None, False))


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 4097, 70001])
def test_select_matches_restatement(n, b):
    gen = torch.Generator().manual_seed(1000 * b + n)
    rows = b * n
    labels = torch.tensor([1, 3, 4])[torch.randint(0, 3, (rows,), generator=gen)].to(DEV)      # class 2 has no member
    seen = set()
    for kind, thresholds, per_class in SELECT_CASES:
        scores = _scores(kind, rows, gen).to(DEV)
        full = dref.select(scores, labels, b, thresholds, max(PRE_MAX), per_class=per_class)
        for pre_max in PRE_MAX:
            cnt = _check_select(scores, labels, b, thresholds, pre_max, per_class, full=full)
            if per_class:
                assert not cnt[:, 1].any() and not cnt[:, 4:].any()
            if kind == "signed":
                assert (cnt == min(pre_max, n)).all()        # no threshold: every row is a member
            seen.update(np.sign(cnt.astype(np.int64) - pre_max).ravel().tolist())
    assert seen <= {-1, 0} and (n == 1 or seen == {-1, 0})         # fewer members than pre_max, and the cut reached


def test_select_edges():
    from spx import ops
    # all scores equal: the lowest rows, per frame
    scores = torch.full((2 * 5000,), 0.75, device=DEV)
    labels = torch.ones(2 * 5000, dtype=torch.int64, device=DEV)
    cand, count = ops.dense_select(scores, labels, 2, [0.5], 100, per_class=False)
    assert count.tolist() == [[100], [100]]
    assert torch.equal(cand[:, 0], torch.stack([torch.arange(100), torch.arange(5000, 5100)]).to(DEV))
    # exactly pre_max members, and one more
    scores = torch.linspace(0.0, 0.4, 9000, device=DEV)
    scores[torch.arange(0, 9000, 9000 // 64)[:64]] = 0.9
    for pre_max in (63, 64, 65):
        cnt = _check_select(scores, labels[:9000], 1, [0.5], pre_max, False)
        assert int(cnt[0, 0]) == min(pre_max, 64)
    # NaN without a threshold is no member either; -0.0 ties with +0.0, lower row first
    scores = torch.tensor([0.0, float("nan"), -0.0, -1.0, 0.0, float("-inf"), float("inf")], device=DEV)
    cand, count = ops.dense_select(scores, labels[:7], 1, None, 16, per_class=False)
    assert count.tolist() == [[6]] and cand[0, 0, :7].tolist() == [6, 0, 2, 4, 3, 5, -1]
    # two runs are bitwise equal
    gen = torch.Generator().manual_seed(3)
    scores = _scores("ties", 70001, gen).to(DEV)
    labels = torch.randint(1, 4, (70001,), generator=gen).to(DEV)
    first = ops.dense_select(scores, labels, 1, THRESH, 4097)
    second = ops.dense_select(scores, labels, 1, THRESH, 4097)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def _run_both(scores, labels, boxes, b, thresholds, pre_max, post_max, axis_aligned, per_class, margin=None):
    from spx import ops
    got = ops.dense_post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, pre_max, post_max,
                                 axis_aligned=axis_aligned, per_class=per_class)
    want = dref.post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, pre_max, post_max,
                             axis_aligned=axis_aligned, per_class=per_class,
                             margin=ref.EXACT_GRID_MARGIN if margin is None else margin)
    check_against(got, want)
    return got, want


FULL = {
    "rotated_per_class": dict(b=2, n=5000),
    "rotated_agnostic": dict(b=2, n=5000, per_class=False),
    "axis_aligned_per_class": dict(b=2, n=5000, axis_aligned=True),
    "axis_aligned_agnostic_post_4": dict(b=3, n=4097, axis_aligned=True, per_class=False, post_max=4),
    "pre_max_65": dict(b=2, n=5000, pre_max=65),
    "n63": dict(b=3, n=63),
    "n1": dict(b=2, n=1),
}


@pytest.mark.parametrize("name", list(FULL))
def test_full_op_matches_restatement(name):
    c = dict(FULL[name])
    b, n = c["b"], c["n"]
    axis_aligned, per_class = c.get("axis_aligned", False), c.get("per_class", True)
    thresholds = THRESH if per_class else [0.3]
    scores, labels, boxes = make_inputs(b, n, seed=len(name), grid=axis_aligned)
    got, want = _run_both(scores, labels, boxes, b, thresholds, c.get("pre_max", 4096), c.get("post_max", 500),
                          axis_aligned, per_class)
    if n >= 4097:
        assert want["suppressed"] > want["entered"] / 4
        if per_class:
            assert want["final_suppressed"] > 0          # survivors of different classes meet in the final stage
    count = got["count"].cpu().numpy()
    for f in range(b):
        k = int(count[f])
        assert bool((got["sel"][f, k:] == -1).all()) and bool((got["sel"][f, :k] >= f * n).all())
        assert bool((got["sel"][f, :k] < (f + 1) * n).all())
    # boxes with more than 7 columns are read by their stride
    wide = torch.cat([boxes, torch.full((b * n, 2), 7.0, device=DEV)], dim=1)
    from spx import ops
    again = ops.dense_post_process(scores, labels, wide, b, thresholds, NMS_THRESH, c.get("pre_max", 4096),
                                   c.get("post_max", 500), axis_aligned=axis_aligned, per_class=per_class)
    for key in got:
        assert torch.equal(got[key], again[key]), key


def _line_of_boxes(n, step):
    """n axis-aligned 2 x 1 boxes along x, `step` apart, scores descending with the row, all on the exact grid."""
    boxes = torch.zeros(n, 7)
    boxes[:, 0] = torch.arange(n) * step
    boxes[:, 3:6] = torch.tensor([2.0, 1.0, 1.0])
    scores = torch.linspace(0.99, 0.5, n)
    return scores.to(DEV), torch.ones(n, dtype=torch.int64, device=DEV), boxes.to(DEV)


@pytest.mark.parametrize("axis_aligned", [False, True])
def test_chain_identical_and_disjoint_boxes(axis_aligned):
    # a chain: neighbours overlap by a third, so every second box goes, across the 64-box words
    scores, labels, boxes = _line_of_boxes(300, 1.0)
    got, _ = _run_both(scores, labels, boxes, 1, [0.3], 4096, 500, axis_aligned, False)
    assert got["sel"][0, :150].tolist() == list(range(0, 300, 2)) and int(got["count"]) == 150
    # the same chain walked from the far end: the order comes from the scores, not from the rows
    got, _ = _run_both(scores.flip(0).contiguous(), labels, boxes, 1, [0.3], 4096, 500, axis_aligned, False)
    assert got["sel"][0, :150].tolist() == list(range(299, 0, -2))
    # identical boxes: one is kept, the one with the best score
    same = boxes[:1].repeat(200, 1)
    got, _ = _run_both(scores[:200].flip(0).contiguous(), labels[:200], same, 1, [0.3], 4096, 500, axis_aligned, False)
    assert int(got["count"]) == 1 and int(got["sel"][0, 0]) == 199
    # disjoint boxes: nothing is suppressed, the walk stops at post_max
    scores, labels, boxes = _line_of_boxes(300, 4.0)
    for post_max in (1, 64, 65, 500):
        got, want = _run_both(scores, labels, boxes, 1, [0.3], 4096, post_max, axis_aligned, False)
        assert want["suppressed"] == 0 and int(got["count"]) == min(post_max, 300)
        assert got["sel"][0, :min(post_max, 300)].tolist() == list(range(min(post_max, 300)))


def test_proposal_shapes_without_threshold():
    """One frame of 9000 candidates out of 9500 rows, raw logits, 512 kept; and 1024 / 100 over three frames."""
    scores, labels, boxes = make_inputs(1, 9500, seed=77)
    logits = torch.logit(scores)                               # negative and positive, distinct
    got, want = _run_both(logits, labels, boxes, 1, None, 9000, 512, False, False)
    assert int(got["count"]) > 100 and want["entered"] == 9000
    scores, labels, boxes = make_inputs(3, 2000, seed=78)
    got, want = _run_both(torch.logit(scores), labels, boxes, 3, None, 1024, 100, False, False)
    assert want["entered"] == 3 * 1024 and int(got["count"].min()) > 10


def test_agrees_with_point_post_process():
    from spx import ops
    for b, n, per_class, axis_aligned, pre_max, post_max in ((2, 4096, True, False, 4096, 500),
                                                             (3, 512, True, True, 64, 16),
                                                             (2, 70, False, False, 4096, 4),
                                                             (1, 1, True, False, 16, 8)):
        scores, labels, boxes = make_inputs(b, n, seed=n + b, grid=axis_aligned)
        thresholds = THRESH if per_class else [0.3]
        a = ops.point_post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, pre_max, post_max,
                                   axis_aligned=axis_aligned, per_class=per_class)
        d = ops.dense_post_process(scores, labels, boxes, b, thresholds, NMS_THRESH, pre_max, post_max,
                                   axis_aligned=axis_aligned, per_class=per_class)
        assert set(a) == set(d)
        for key in a:
            assert a[key].dtype == d[key].dtype and torch.equal(a[key], d[key]), key
    big = torch.zeros(4097, device=DEV)
    from spx import _lib
    with pytest.raises(_lib.SpxError, match="code -5"):        # §15 keeps its limit
        ops.point_post_process(big, big.long(), torch.zeros(4097, 7, device=DEV), 1, THRESH, NMS_THRESH, 16, 8)


def test_prefilled_outputs_are_overwritten_and_runs_repeat_bitwise():
    from spx import _lib, ops
    lib = _lib.load()
    b, n, pre_max, post_max = 3, 4097, 4096, 4
    scores, labels, boxes = make_inputs(b, n, seed=5)
    scores[n:2 * n] *= 0.25                                                # frame 1: count 0, all padding
    want = ops.dense_post_process(scores, labels, boxes, b, THRESH, NMS_THRESH, pre_max, post_max)
    second = ops.dense_post_process(scores, labels, boxes, b, THRESH, NMS_THRESH, pre_max, post_max)
    for key in want:
        assert torch.equal(want[key], second[key]), key
    cap = want["sel"].shape[1]
    assert cap == 12 and int(want["count"][1]) == 0 and int(want["count"].max()) > 0
    sel = torch.full((b, cap), -7, dtype=torch.int64, device=DEV)
    count = torch.full((b,), -7, dtype=torch.int32, device=DEV)
    ob = torch.full((b, cap, 7), float("nan"), device=DEV)
    osc = torch.full((b, cap), float("nan"), device=DEV)
    ol = torch.full((b, cap), -7, dtype=torch.int64, device=DEV)
    wsb = lib.spx_dense_post_process_ws_bytes(b, n, 3, pre_max, post_max)
    ws = torch.full((wsb,), 0xAB, dtype=torch.uint8, device=DEV)           # a dirty workspace
    p = lambda t: ctypes.c_void_p(t.data_ptr())    # noqa: E731
    lab32 = labels.int()
    rc = lib.spx_dense_post_process(p(scores), p(lab32), p(boxes), 7, b, n, _lib.f_arr(THRESH), 3, NMS_THRESH, pre_max,
                                    post_max, 0, 1, p(sel), p(count), p(ob), p(osc), p(ol), p(ws), wsb,
                                    ops._stream(scores))
    torch.cuda.synchronize()
    assert rc == 0
    for a, w in ((sel, want["sel"]), (count, want["count"]), (ob, want["boxes"]), (osc, want["scores"]),
                 (ol, want["labels"])):
        assert torch.equal(a, w)
    assert bool((sel[1] == -1).all()) and bool((ob[1] == 0).all()) and bool((ol[1] == 0).all())
    # the selection's outputs likewise
    cand = torch.full((b, 3, 100), -7, dtype=torch.int64, device=DEV)
    cnt = torch.full((b, 3), -7, dtype=torch.int32, device=DEV)
    wsb = lib.spx_dense_select_ws_bytes(b, n, 3, 100)
    ws = torch.full((wsb,), 0xAB, dtype=torch.uint8, device=DEV)
    rc = lib.spx_dense_select(p(scores), p(lab32), b, n, _lib.f_arr(THRESH), 3, 100, 1, p(cand), p(cnt), p(ws), wsb,
                              ops._stream(scores))
    torch.cuda.synchronize()
    want_cand, want_cnt = dref.select(scores, labels, b, THRESH, 100)
    assert rc == 0 and np.array_equal(cand.cpu().numpy(), want_cand) and np.array_equal(cnt.cpu().numpy(), want_cnt)


def test_captures_under_a_graph():
    from spx import ops
    b, n = 2, 70001
    scores, labels, boxes = make_inputs(b, n, seed=11)
    thresholds = [0.94, 0.93, 0.93]               # some 800 members per frame
    args = (b, thresholds, NMS_THRESH, 4096, 500)
    ops.dense_post_process(scores, labels, boxes, *args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.dense_post_process(scores, labels, boxes, *args)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.dense_post_process(scores, labels, boxes, *args)
    scores.copy_(scores.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    want = dref.post_process(scores, labels, boxes, *args)
    assert int(want["count"].min()) > 10
    check_against(captured, want)


# ------------------------------------------------------------------------------------------------------ detectors
def _tie_free_logits(shape, seed):
    """Distinct, well separated logits whose sigmoids are distinct too (checked on the device, where they are used);
    a seed that ties is replaced by the next one."""
    n = int(np.prod(shape))
    for s in range(seed, seed + 8):
        g = torch.Generator().manual_seed(s)
        logits = torch.linspace(-7.0, 2.5, n)[torch.randperm(n, generator=g)].view(shape).to(DEV)
        if torch.sigmoid(logits).unique().numel() == n:
            return logits
    raise AssertionError("no tie-free seed")


def _second():
    from test_gpu_model import _batch, _build
    _cfg, ds, model = _build(seed=9)
    model.to(DEV).eval()
    bd = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in _batch(ds).items()}
    return model, ds, bd


def _pillar():
    from test_gpu_pillar_vfe import _pointpillar
    _cfg, ds, model, _plain, batch, _vox = _pointpillar()
    return model.eval(), ds, dict(batch)


def _head_outputs(model, bd, seed):
    with torch.no_grad():
        out = dict(bd)
        for m in model.module_list:
            out = m(out)
    out["batch_cls_preds"] = _tie_free_logits(out["batch_cls_preds"].shape, seed)
    return out


def _post(model, out, fused, raw=False):
    cfg = model.model_cfg.POST_PROCESSING
    if fused is not None:
        cfg["FUSED"] = fused
    cfg["OUTPUT_RAW_SCORE"] = raw
    try:
        with torch.no_grad():
            return model.post_processing(dict(out))
    finally:
        cfg.pop("FUSED", None)
        cfg["OUTPUT_RAW_SCORE"] = False


def _same_preds(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("which", ["second", "pointpillar"])
def test_detector_fused_equals_default_path(which, monkeypatch):
    from spx import ops
    model, _ds, bd = _second() if which == "second" else _pillar()
    out = _head_outputs(model, bd, seed=4)
    assert out["batch_box_preds"].dim() == 3 and out["batch_box_preds"].shape[1] > ops.POST_PROCESS_MAX_N
    assert isinstance(model.model_cfg.POST_PROCESSING.SCORE_THRESH, list) == (which == "second")
    calls = []
    real = ops.dense_post_process
    monkeypatch.setattr(ops, "dense_post_process", lambda *a, **k: calls.append(1) or real(*a, **k))
    assert model._fused_post_plan(out) is None                    # FUSED absent: dense predictions keep the eager path
    default, rec_d = _post(model, out, None)
    assert not calls
    fused, rec_f = _post(model, out, True)
    assert len(calls) == 1
    assert sum(p["pred_boxes"].shape[0] for p in default) > 4
    _same_preds(fused, default)
    assert rec_f == rec_d and set(rec_f) == {"gt"} | {"%s_%s" % (p, t) for p in ("roi", "rcnn") for t in (0.3, 0.5, 0.7)}
    assert rec_f["gt"] > 0 and all(rec_f["roi_%s" % t] == 0 for t in (0.3, 0.5, 0.7))
    _same_preds(_post(model, out, True, raw=True)[0], _post(model, out, None, raw=True)[0])
    # a second stage's classes: the labels come from roi_labels
    g = torch.Generator().manual_seed(6)
    b, n = out["batch_box_preds"].shape[:2]
    staged = dict(out, has_class_labels=True, roi_labels=torch.randint(1, 4, (b, n), generator=g).to(DEV))
    fused2, _ = _post(model, staged, True)
    _same_preds(fused2, _post(model, staged, None)[0])
    assert any(not torch.equal(a["pred_labels"], c["pred_labels"]) for a, c in zip(fused2, fused))


def test_static_post_processing_of_dense_predictions_captures_and_replays():
    model, _ds, bd = _second()
    out = _head_outputs(model, bd, seed=14)
    with pytest.raises(NotImplementedError):
        model.post_processing_static(out)                         # FUSED absent
    cfg = model.model_cfg.POST_PROCESSING
    cfg["FUSED"] = True
    try:
        static_in = dict(out, batch_cls_preds=out["batch_cls_preds"].clone(), batch_box_preds=out["batch_box_preds"].clone())
        with torch.no_grad():
            first = {k: v.clone() for k, v in model.post_processing_static(static_in).items()}
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                model.post_processing_static(static_in)
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                captured = model.post_processing_static(static_in)
            static_in["batch_cls_preds"].copy_(_tie_free_logits(out["batch_cls_preds"].shape, seed=15))
            graph.replay()
            torch.cuda.synchronize()
            fresh = model.post_processing_static(static_in)
            pred_dicts, recall = model.post_processing(static_in)
    finally:
        cfg.pop("FUSED", None)
    assert set(captured) == set(fresh) == {"sel", "count", "pred_boxes", "pred_scores", "pred_labels", "layout_ok",
                                            "recalled", "num_gt"}
    for k in fresh:
        assert torch.equal(captured[k], fresh[k]), k
    assert bool(fresh["layout_ok"]) and int(fresh["count"].sum()) > 4 and not torch.equal(fresh["sel"], first["sel"])
    for i, p in enumerate(pred_dicts):
        assert torch.equal(p["pred_boxes"], fresh["pred_boxes"][i, :int(fresh["count"][i])])
    assert recall["gt"] == int(fresh["num_gt"].sum())


def _eager_forward(model, pts):
    with torch.no_grad():
        bd = {"points": pts, "batch_size": 2}
        for m in model.module_list:
            bd = m(bd)
    return bd


def _spread_head(model, shape, per_frame=300, seed=21):
    """A random-init class head gives every anchor a logit within 0.15 of -4.6, thousands of them equal, and the order
    torch.topk gives equal scores is unspecified.  A forward hook on the head therefore adds a fixed offset to its
    logits, in the eager model and in the captured graph alike: `per_frame` anchors of every frame are lifted on one
    class by 2.6 .. 5.6 in steps of 0.01 (scores of about 0.12 .. 0.73), everything else is pushed 20 below.  The rows
    over the threshold are then tie-free (asserted by the caller).  Returns the hook's handle."""
    g = torch.Generator().manual_seed(seed)
    b, n, c = shape
    offset = torch.full(shape, -20.0)
    for f in range(b):
        rows = torch.randperm(n, generator=g)[:per_frame]
        lift = torch.linspace(2.6, 5.6, per_frame)[torch.randperm(per_frame, generator=g)]
        offset[f, rows, torch.randint(0, c, (per_frame,), generator=g)] = lift
    offset = offset.to(DEV)

    def hook(_module, _inputs, out):
        out["batch_cls_preds"] = out["batch_cls_preds"] + offset
        return out

    return model.dense_head.register_forward_hook(hook)


@pytest.mark.parametrize("which", ["second", "pointpillar"])
def test_graphed_anchor_detector_replays_the_whole_forward(which):
    """One replay holds voxelisation through NMS and equals the eager model on the same points: the voxel count, the
    head outputs to 1e-5 (the vendor's dense convolutions repeat to ~1e-7 only), and the detections of eager
    model.post_processing -- the same boxes in the same order, labels exactly, scores and boxes to 1e-5 -- on a head whose
    scores over the threshold are tie-free (_spread_head, in both paths; asserted).  The replay's detections are also checked exactly
    against the restatement and the un-graphed fused path, both run on the replay's own head outputs."""
    from pcdet_amd.models.inference import GraphedAnchorDetector
    model, ds, _bd = _second() if which == "second" else _pillar()
    batches = [torch.from_numpy(ds.collate_batch([ds[i] for i in frames])["points"]).to(DEV) for frames in ((0, 1), (2, 3))]
    handle = _spread_head(model, tuple(_eager_forward(model, batches[0])["batch_cls_preds"].shape))
    try:
        runner = GraphedAnchorDetector(model, batch_size=2, max_points=9000)
        cfg = model.model_cfg.POST_PROCESSING
        assert "FUSED" not in cfg
        thresholds = cfg.SCORE_THRESH if isinstance(cfg.SCORE_THRESH, list) else [cfg.SCORE_THRESH]
        seen = []
        for pts in batches:
            out = runner(pts)
            preds, rec = runner.pred_dicts()
            assert rec == {} and len(preds) == 2
            # the eager model on the same points
            bd = _eager_forward(model, pts)
            assert int(out["counts"]["voxels"].item()) == bd["voxel_coords"].shape[0]
            assert out["batch_box_preds"].shape == bd["batch_box_preds"].shape
            assert float((out["batch_box_preds"] - bd["batch_box_preds"]).abs().max()) < 1e-5
            assert float((out["batch_cls_preds"] - bd["batch_cls_preds"]).abs().max()) < 1e-5
            best = torch.sigmoid(bd["batch_cls_preds"]).max(dim=-1)[0]
            for f in range(2):
                over = best[f][best[f] >= 0.1]
                assert over.numel() >= 5 and over.unique().numel() == over.numel()        # tie-free where it matters
            with torch.no_grad():
                eager_preds, _ = model.post_processing(bd)                # FUSED absent: the per-frame eager loop
            assert sum(p["pred_boxes"].shape[0] for p in eager_preds) > 0
            for p, e in zip(preds, eager_preds):
                assert p["pred_boxes"].shape == e["pred_boxes"].shape
                assert torch.equal(p["pred_labels"], e["pred_labels"])
                assert float((p["pred_scores"] - e["pred_scores"]).abs().max()) < 1e-5
                assert float((p["pred_boxes"] - e["pred_boxes"]).abs().max()) < 1e-5
            # exactly, on the replay's own head outputs
            scores, labels = torch.sigmoid(out["batch_cls_preds"]).max(dim=-1)
            want = dref.post_process(scores.reshape(-1), labels.reshape(-1) + 1, out["batch_box_preds"].reshape(-1, 7), 2,
                                     thresholds, cfg.NMS_CONFIG.NMS_THRESH, cfg.NMS_CONFIG.NMS_PRE_MAXSIZE,
                                     cfg.NMS_CONFIG.NMS_POST_MAXSIZE, per_class=isinstance(cfg.SCORE_THRESH, list))
            assert int(want["count"].sum()) > 0
            for i, p in enumerate(preds):
                k = int(want["count"][i])
                assert p["pred_boxes"].shape[0] == k
                assert np.array_equal(p["pred_boxes"].cpu().numpy(), want["boxes"][i, :k])
                assert np.array_equal(p["pred_scores"].cpu().numpy(), want["scores"][i, :k])
                assert np.array_equal(p["pred_labels"].cpu().numpy(), want["labels"][i, :k])
            _same_preds(preds, _post(model, {k: out[k] for k in ("batch_size", "batch_cls_preds", "batch_box_preds",
                                                                 "cls_preds_normalized")}, True)[0])
            seen.append(torch.cat([p["pred_boxes"] for p in preds]).clone())
        assert seen[0].shape != seen[1].shape or not torch.equal(seen[0], seen[1])
    finally:
        handle.remove()


@pytest.mark.parametrize("pre,post,candidate", [(1024, 100, False), (9000, 512, False), (1024, 100, True)])
def test_proposal_layer_fused_equals_the_loop_and_captures(pre, post, candidate):
    from pcdet_amd.config import AttrDict
    from pcdet_amd.models.roi_heads.roi_head_template import RoIHeadTemplate
    head = RoIHeadTemplate.__new__(RoIHeadTemplate)
    b, n = 2, 9500
    _scores, _labels, boxes = make_inputs(b, n, seed=31)
    boxes = torch.cat([boxes, torch.rand(b * n, 2, device=DEV)], dim=1).view(b, n, 9)       # 7 + C columns
    batch = dict(batch_size=b, batch_box_preds=boxes, batch_cls_preds=_tie_free_logits((b, n, 3), seed=32))
    if candidate:      # the products of two sigmoids must be tie-free too: the first seed for which they are
        best = torch.sigmoid(batch["batch_cls_preds"].max(dim=2)[0])
        for seed in range(33, 97):
            batch["candidate_score"] = _tie_free_logits((b, n), seed=seed)
            if (best * torch.sigmoid(batch["candidate_score"])).unique().numel() == b * n:
                break
    loop_cfg = AttrDict(NMS_TYPE="nms_gpu", MULTI_CLASSES_NMS=False, NMS_PRE_MAXSIZE=pre, NMS_POST_MAXSIZE=post,
                        NMS_THRESH=0.7)
    fused_cfg = AttrDict(dict(loop_cfg, FUSED=True))
    want = head.proposal_layer(dict(batch), loop_cfg)
    got = head.proposal_layer(dict(batch), fused_cfg)
    if candidate:
        s = torch.sigmoid(batch["batch_cls_preds"].max(dim=2)[0]) * torch.sigmoid(batch["candidate_score"])
        assert s.unique().numel() == s.numel()
    assert tuple(got["rois"].shape) == (b, post, 9) and got["has_class_labels"] is True
    for k in ("rois", "roi_scores", "roi_labels"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].view(torch.int32 if got[k].dtype == torch.float32 else got[k].dtype),
                           want[k].view(torch.int32 if want[k].dtype == torch.float32 else want[k].dtype)), k   # bits
    assert bool((got["roi_labels"] >= 1).all())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        head.proposal_layer(dict(batch), fused_cfg)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = head.proposal_layer(dict(batch), fused_cfg)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("rois", "roi_scores", "roi_labels"):
        assert torch.equal(captured[k], want[k]), k
