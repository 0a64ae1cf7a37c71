"""The fused point-head losses on the GPU (csrc/point_loss.hip, include/spx.h §17) against what the reference computes
(tests/golden/point_head_losses.npz, float64): losses and the gradients of their sum.

The tolerance is measured, not fixed: for each tensor e_fused = max |fused - golden| must stay within
max(4 * e_eager, 1e-6 * max |golden|), e_eager = max |float32 torch composition on the same device - golden|
(point_loss_ref.measured_bound).  Both errors are printed per tensor.  Also: every output element is written and the
rows the reference gives no gradient are exact zeros, two calls are bitwise equal, the SASA layer loss, the head's
get_loss_fused end to end on assigned labels, and graph capture (which fails on any host read)."""
import functools

import numpy as np
import pytest
import torch

import point_loss_ref as plr
import point_targets_ref as ptr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY = 12345.5
PAD = 64


def _check(name, fused, eager, golden):
    fused, eager = np.asarray(fused, np.float64), np.asarray(eager, np.float64)
    e_fused, e_eager = float(np.abs(fused - golden).max()), float(np.abs(eager - golden).max())
    bound = plr.measured_bound(e_eager, golden)
    print("%-22s e_fused %.3e  e_eager %.3e  bound %.3e  max|golden| %.3e" % (name, e_fused, e_eager, bound,
                                                                              float(np.abs(golden).max())))
    assert np.isfinite(fused).all(), name
    assert e_fused <= bound, (name, e_fused, e_eager, bound)


def _run(loss_fn, rd):
    """(components, total, gradients of total w.r.t. the four leaves) as float64 numpy."""
    total, parts = loss_fn(rd)
    leaves = [rd[plr.LEAF_KEYS[k]] for k in plr.LEAVES]
    grads = torch.autograd.grad(total, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for x, g in zip(leaves, grads)]
    return parts.double().cpu().numpy(), float(total.detach()), [g.double().cpu().numpy() for g in grads]


@functools.lru_cache(maxsize=None)
def _head():
    return plr.head().to(DEV)


@functools.lru_cache(maxsize=None)
def _eager(case):
    from pcdet_amd.models.dense_heads import point_losses
    h = _head()
    return _run(lambda rd: point_losses.head_loss_torch(rd, *plr.head_loss_args(h)), plr.ret_dict(case, torch.float32, DEV))


@pytest.mark.parametrize("case", plr.CASES)
def test_fused_matches_reference(case):
    from pcdet_amd.models.dense_heads import point_losses
    h = _head()
    g = plr.load(case)
    parts, total, grads = _run(lambda rd: point_losses.head_loss_fused(rd, *plr.head_loss_args(h)),
                               plr.ret_dict(case, torch.float32, DEV))
    e_parts, e_total, e_grads = _eager(case)
    print("case %s" % case)
    _check("losses", parts, e_parts, g["losses"])
    _check("total", total, e_total, g["losses"].sum())
    for name, got, eager in zip(plr.LEAVES, grads, e_grads):
        _check("d_" + name, got, eager, plr.grad(case, "sum", name))
    if case == "c":                              # no positive in the batch: the same path, zero box gradients
        assert all(np.isfinite(x).all() for x in grads)
        assert not grads[0].any() and not grads[2].any() and not grads[3].any()
        assert parts[0] == 0 and parts[2] == 0


def _raw_call(case):
    """spx_point_head_loss into canary-filled buffers with guard bands: nothing is pre-zeroed, so an element the op
    skips keeps the canary."""
    from spx import _lib, ops
    lib = _lib.load()
    rd = plr.ret_dict(case, torch.float32, DEV, leaves=False)
    n = rd["s_point_cls_labels"].shape[0]
    widths = {"losses": 3, "vote": n * 3, "cls": n * 3, "reg": n * 30, "box": n * 7}
    bufs = {k: torch.full((w + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV) for k, w in widths.items()}
    wsb = lib.spx_point_head_loss_ws_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    params = _lib.f_arr([1.0, 1.0, 0.1, 0.1, 0.1, 0.1, 1.0, 1.0, 1.0 / 9.0, 0.0, 1.0])
    keys = ("s_point_vote_coords", "s_point_cls_preds", "s_point_reg_preds", "s_point_box_preds", "point_cls_preds",
            "point_reg_preds", "point_box_preds", "vote_cls_labels", "vote_reg_labels", "s_point_cls_labels",
            "s_point_reg_labels", "s_point_box_labels")
    rc = lib.spx_point_head_loss(*[ops._ptr(rd[k]) for k in keys], n, 3, 12, params, 1, 1, 1,
                                 *[ops._ptr(bufs[k][PAD:]) for k in ("losses", "vote", "cls", "reg", "box")],
                                 ops._ptr(ws), wsb, ops._stream(ws))
    assert rc == 0
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert (t[:PAD] == CANARY).all() and (t[-PAD:] == CANARY).all(), k
    return rd, {k: bufs[k][PAD:-PAD].view(-1, widths[k] // n) if k != "losses" else bufs[k][PAD:-PAD] for k in bufs}


@pytest.mark.parametrize("case", plr.CASES)
def test_every_element_written_and_exact_zeros(case):
    rd, out = _raw_call(case)
    for k, t in out.items():
        assert torch.isfinite(t).all() and not (t == CANARY).any(), k
    labels, vote_labels = rd["s_point_cls_labels"], rd["vote_cls_labels"]
    assert not out["cls"][labels < 0].any()
    assert not out["reg"][labels <= 0].any() and not out["box"][labels <= 0].any()
    assert not out["vote"][vote_labels <= 0].any()
    if case != "c":
        assert out["cls"][labels >= 0].abs().min() > 0
        assert out["box"][labels > 0].abs().sum(dim=1).min() > 0 and out["vote"][vote_labels > 0].abs().sum(dim=1).min() > 0
    else:
        assert not out["reg"].any() and not out["box"].any() and not out["vote"].any()


def test_two_calls_are_bitwise_equal():
    first, second = _raw_call("b")[1], _raw_call("b")[1]
    for k in first:
        assert torch.equal(first[k], second[k]), k


# ------------------------------------------------------------------------------------------------- SASA layer loss

@pytest.mark.parametrize("case", ("a", "b"))                 # 74 and 513 rows
@pytest.mark.parametrize("func", ("BCE", "Focal"))
@pytest.mark.parametrize("s", (1, 3))
def test_seg_loss(case, func, s):
    """Against the reference's value where it is recorded; the reference cannot evaluate BCE with one score column and
    three classes, for which the float64 torch composition stands in."""
    from pcdet_amd.utils import loss_utils
    g = plr.load(case)
    sasa = loss_utils.PointSASALoss(func=func, layer_weights=[plr.SEG_LAYER_WEIGHT], extra_width=[1.0, 1.0, 1.0],
                                    set_ignore_flag=True, num_class=plr.NUM_CLASS)
    labels = torch.from_numpy(g["seg_labels"]).to(DEV)

    def run(dtype, fused):
        x = torch.from_numpy(g["seg_scores%d" % s]).to(DEV).to(dtype).requires_grad_(True)
        loss, = sasa.loss_forward([x], [labels], [None], [None], [None], fused=fused)
        assert loss.dim() == 0
        grad, = torch.autograd.grad(loss, x)
        return float(loss.detach()), grad.double().cpu().numpy()

    key = "seg_%s_s%d" % (func, s)
    if key in g:
        want, want_grad = float(g[key]), g[key + "_grad"]
    else:
        assert (func, s) == ("BCE", 1)
        want, want_grad = run(torch.float64, False)
    got, got_grad = run(torch.float32, True)
    eager, eager_grad = run(torch.float32, False)
    print("case %s %s S=%d" % (case, func, s))
    _check("seg loss", got, eager, np.asarray(want))
    _check("seg d_scores", got_grad, eager_grad, want_grad)
    assert (g["seg_labels"] == -1).sum() >= 4 and not got_grad[g["seg_labels"] < 0].any()


# ----------------------------------------------------------------------------------- the head's methods, end to end

def _assigned_ret_dict(seed, dtype=torch.float32):
    """B = 2, n = 37: labels from the head's own assignment ops on the GPU, random predictions around them."""
    h = _head()
    pts, gt, _ = ptr.make_case(5, 8, b=2, n=37, seed=seed)
    gt[:, 2, 0] += 500.0                       # the 5e-6 thin box: every point inside it sits on a centerness tie
    rows = pts.shape[0] * pts.shape[1]
    bs = np.repeat(np.arange(2, dtype=np.float32), 37)[:, None]
    points = torch.from_numpy(np.concatenate([bs, pts.reshape(-1, 3)], axis=1)).to(DEV)
    d_gt = torch.from_numpy(gt).to(DEV)
    stu = h.assign_stu_targets({"s_point_vote_coords": points, "gt_boxes": d_gt})
    tea = h.assign_targets({"point_vote_coords": points, "gt_boxes": d_gt})
    vote = h.assign_targets_simple(points, d_gt, extra_width=h.model_cfg.TARGET_CONFIG.VOTE_EXTRA_WIDTH,
                                   set_ignore_flag=False)
    assert torch.equal(stu["point_cls_labels"], tea["point_cls_labels"]) and (stu["point_cls_labels"] > 0).sum() >= 12
    gen = torch.Generator().manual_seed(100 + seed)

    def noisy(t, sigma):
        return (t.cpu() + torch.randn(t.shape, generator=gen) * sigma).to(DEV)

    seg_points = [points, points, points]
    seg_scores = [noisy(torch.zeros(rows, 1), 1.5), None, noisy(torch.zeros(rows, 1), 1.5)]
    l_labels, l_boxes, l_parts = h.loss_point_sasa(seg_points, seg_scores, d_gt)
    reg = noisy(stu["point_reg_labels"], 0.3)
    t_reg = noisy(tea["point_reg_labels"], 0.3)
    rd = {"s_point_vote_coords": points[:, 1:4].contiguous(), "vote_cls_labels": vote["point_cls_labels"],
          "vote_reg_labels": vote["point_reg_labels"],
          "s_point_cls_preds": noisy(torch.zeros(rows, 3), 1.5), "s_point_reg_preds": reg,
          "s_point_box_preds": noisy(h.box_coder.decode_torch(reg, points[:, 1:4])[:, :7], 0.05),
          "point_cls_preds": noisy(torch.zeros(rows, 3), 1.5), "point_reg_preds": t_reg,
          "point_box_preds": noisy(h.box_coder.decode_torch(t_reg, points[:, 1:4])[:, :7], 0.05),
          "s_point_cls_labels": stu["point_cls_labels"], "s_point_reg_labels": stu["point_reg_labels"],
          "s_point_box_labels": stu["point_box_labels"],
          "point_sasa_preds": seg_scores, "point_sasa_labels": l_labels, "point_sasa": seg_points,
          "point_sasa_boxes": l_boxes, "point_sasa_parts": l_parts}

    def cast(v):
        if isinstance(v, list):
            return [cast(x) for x in v]
        return v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v

    rd = {k: cast(v) for k, v in rd.items()}
    for key in plr.LEAF_KEYS.values():
        rd[key] = rd[key].clone().requires_grad_(True)
    return rd


def _head_run(method, rd):
    loss, tb = method(rd)
    loss.backward()
    grads = [rd[plr.LEAF_KEYS[k]].grad for k in plr.LEAVES]
    grads = [torch.zeros_like(rd[plr.LEAF_KEYS[k]]) if g is None else g for k, g in zip(plr.LEAVES, grads)]
    return float(loss.detach()), [g.double().cpu().numpy() for g in grads], tb


def test_get_loss_fused_end_to_end():
    """get_loss_fused on assigned labels against get_loss_torch on the same ret_dict; float64 get_loss_torch on the
    device stands where the golden values stand in the other tests."""
    h = _head()
    want, want_grads, want_tb = _head_run(h.get_loss_torch, _assigned_ret_dict(0, torch.float64))
    eager, eager_grads, eager_tb = _head_run(h.get_loss_torch, _assigned_ret_dict(0))
    got, got_grads, tb = _head_run(h.get_loss_fused, _assigned_ret_dict(0))
    print("end to end")
    _check("point_loss", got, eager, np.asarray(want))
    for name, a, b, c in zip(plr.LEAVES, got_grads, eager_grads, want_grads):
        _check("d_" + name, a, b, c)
    assert sorted(tb) == sorted(eager_tb) == ["point_loss_box", "point_loss_cls", "point_loss_sasa",
                                              "point_loss_sasa_layer_0", "point_loss_sasa_layer_2", "point_loss_vote",
                                              "point_pos_num", "vote_loss_reg"]
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and not v.requires_grad for v in tb.values())
    assert int(tb["point_pos_num"]) == int(eager_tb["point_pos_num"]) >= 12
    for k in tb:
        if k != "point_pos_num":
            _check("tb " + k, float(tb[k]), float(eager_tb[k]), np.asarray(float(want_tb[k])))


def test_graph_capture_and_replay_on_new_inputs():
    """Forward and backward captured after a warm-up on a side stream, replayed on new values: bitwise the uncaptured
    call.  Capture fails on any host read, so this is the no-sync check."""
    h = _head()
    rd, rd2 = _assigned_ret_dict(0), _assigned_ret_dict(1)
    leaves = [rd[plr.LEAF_KEYS[k]] for k in plr.LEAVES]

    def step():
        loss, tb = h.get_loss_fused(rd)
        return loss, torch.autograd.grad(loss, leaves), tb

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grads, tb = step()
    with torch.no_grad():
        for k, v in rd.items():
            if isinstance(v, torch.Tensor):
                v.copy_(rd2[k])
            else:
                for a, b in zip(v, rd2[k]):
                    if a is not None:
                        a.copy_(b)
    assert not torch.equal(rd["s_point_cls_labels"], _assigned_ret_dict(0)["s_point_cls_labels"])
    graph.replay()
    torch.cuda.synchronize()
    want_loss, want_tb = h.get_loss_fused(rd2)
    want_grads = torch.autograd.grad(want_loss, [rd2[plr.LEAF_KEYS[k]] for k in plr.LEAVES])
    assert torch.equal(loss, want_loss.detach())
    for a, b in zip(grads, want_grads):
        assert torch.equal(a, b)
    for k in tb:
        assert torch.equal(tb[k], want_tb[k]), k
