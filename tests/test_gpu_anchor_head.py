"""The anchor head's two fused HIP ops on the GPU, at the smallest shapes at which they can go wrong, against the plain
references of tests/anchor_head_ref.py (pinned to the reference project by tests/test_anchor_head_ref.py).

csrc/assign.hip (k_gt_keep, k_gt_max, k_assign): labels and weights exactly, no anchor left out; regression targets
within 1e-5 of float64 (a few ulp of logf and sqrtf at |target| < 8).  The inputs hold exact ties, thresholds equal to
an IoU's bit pattern, the only gt in row 255 of 256, anchor sets smaller than a block, frames without any overlap.

csrc/anchor_loss.hip (k_count_pos, k_anchor_loss, k_loss_final): for each loss and each gradient
e_fused = max |fused - float64| <= point_loss_ref.measured_bound(e_eager, float64), e_eager being the error of this
project's float32 torch composition on the same device and inputs.  Both are printed per tensor (pytest -s);
profiles/anchor_head_accuracy.log keeps the table of one run on an MI355X.  Elements the reference gives no weight are exact zeros; a target on a direction-bin
boundary falls in the reference's float32 bin.
"""
import numpy as np
import pytest
import torch

import anchor_head_ref as ahr
import point_loss_ref as plr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAD = 64
CANARY_F, CANARY_I = 12345.5, 0x5A5A5A5A


# ---------------------------------------------------------------------------------------------------- assignment

def _device_inputs(case):
    flat = torch.from_numpy(np.stack([a.reshape(-1, 7) for a in case["anchor_sets"]])).to(DEV)
    set_cls = torch.tensor([case["class_names"].index(n) for n in case["set_names"]], dtype=torch.int32, device=DEV)
    mt = torch.tensor(case["matched"], dtype=torch.float32, device=DEV)
    um = torch.tensor(case["unmatched"], dtype=torch.float32, device=DEV)
    return flat, set_cls, mt, um, torch.from_numpy(case["gt"]).to(DEV)


def _ops_assign(case):
    from spx import ops
    flat, set_cls, mt, um, gt = _device_inputs(case)
    return ops.assign_targets(flat, case["per_location"], gt, set_cls, len(case["class_names"]), mt, um)


def _check_assign(got, ref, what):
    labels, targets, weights = got
    assert labels.dtype == torch.int32 and targets.dtype == torch.float32 and weights.dtype == torch.float32
    labels, targets, weights = labels.cpu().numpy(), targets.cpu().numpy(), weights.cpu().numpy()
    assert labels.shape == ref["labels"].shape and targets.shape == ref["targets"].shape
    wrong = np.argwhere(labels != ref["labels"])
    assert wrong.size == 0, (what, wrong[:8], labels[labels != ref["labels"]][:8], ref["labels"][labels != ref["labels"]][:8])
    assert np.array_equal(weights, ref["weights"]), what
    err = float(np.abs(targets - ref["targets"]).max())
    print("%-22s anchors %6d  positives %4d  ignored %4d  target error %.2e" % (
        what, labels.size, (labels > 0).sum(), (labels < 0).sum(), err))
    assert err < 1e-5, (what, err)
    assert not targets[labels <= 0].any(), what


@pytest.fixture
def counted_assign(monkeypatch):
    """Counts the calls of spx.ops.assign_targets, to tell the fused path from the torch formulation."""
    from spx import ops
    calls, real = [], ops.assign_targets

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "assign_targets", wrapper)
    return calls


def test_fixture_head_edge_batch(counted_assign):
    """Three anchor sets of 2 560 anchors, 10 blocks each, so the per-gt maximum crosses blocks; five frames, M = 8."""
    head = ahr.fixture_head(DEV)
    out = head.target_assigner.assign_targets(head.anchors, torch.from_numpy(ahr.fixture_edge_batch()).to(DEV))
    assert len(counted_assign) == 1
    ref = ahr.fixture_ref()
    _check_assign((out["box_cls_labels"], out["box_reg_targets"], out["reg_weights"]), ref, "fixture head")
    # what the reference has to report for the batch to mean something
    matched = np.tile(np.repeat(np.array(ahr.FIXTURE_MATCHED), 2), ref["labels"].shape[1] // 6)[None, :]
    assert (ref["forced"] & (ref["labels"] > 0) & (ref["max_iou"] < matched)).sum() >= 1
    assert (ref["labels"] == -1).sum() >= 1
    assert ahr.threshold_margin(ref, ahr.FIXTURE_MATCHED, ahr.FIXTURE_UNMATCHED, 3, 2) > 1e-5


@pytest.mark.parametrize("name", ahr.SYNTH_CASES)
def test_synthetic_anchor_sets(name):
    case, ref = ahr.synth_case(name), ahr.synth_ref(name)
    _check_assign(_ops_assign(case), ref, name)
    if name == "tie":
        assert ref["forced_per_gt"][0][0].tolist() == [2]
    if name == "threshold":
        assert ref["labels"].reshape(3, 256, 2)[0, 40:42, 0].tolist() == [1, 1]
        assert ref["labels"].reshape(3, 256, 2)[1, 40:42, 1].tolist() == [-1, -1]


def test_more_than_256_gt_rows_take_the_torch_path(counted_assign):
    from spx import _lib, ops
    head = ahr.fixture_head(DEV)
    gt = torch.from_numpy(ahr.fixture_edge_batch(257)).to(DEV)
    out = head.target_assigner.assign_targets(head.anchors, gt)
    assert len(counted_assign) == 0
    _check_assign((out["box_cls_labels"], out["box_reg_targets"], out["reg_weights"]), ahr.fixture_ref(257), "M = 257")
    flat, per_loc, set_cls, mt, um = head.target_assigner._kernel_inputs(head.anchors)
    with pytest.raises(_lib.SpxError):
        ops.assign_targets(flat, per_loc, gt, set_cls, 3, mt, um)


def test_cached_workspace_is_reset_between_calls():
    """The per-gt maxima live in a cached workspace: a call must not see those of the call before it."""
    for name in ("last_row", "threshold", "tie", "last_row"):
        _check_assign(_ops_assign(ahr.synth_case(name)), ahr.synth_ref(name), name + " (shared workspace)")


def _raw_assign(name):
    """spx_assign_targets into canary-filled buffers with guard bands; nothing is pre-zeroed."""
    from spx import _lib, ops
    lib = _lib.load()
    case = ahr.synth_case(name)
    flat, set_cls, mt, um, gt = _device_inputs(case)
    n_sets, a, _ = flat.shape
    b, m = gt.shape[0], gt.shape[1]
    n = b * n_sets * a
    bufs = {"labels": torch.full((n + 2 * PAD,), CANARY_I, dtype=torch.int32, device=DEV),
            "targets": torch.full((n * 7 + 2 * PAD,), CANARY_F, dtype=torch.float32, device=DEV),
            "weights": torch.full((n + 2 * PAD,), CANARY_F, dtype=torch.float32, device=DEV)}
    wsb = lib.spx_assign_targets_ws_bytes(b, n_sets, m)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = lib.spx_assign_targets(ops._ptr(flat), n_sets, a, case["per_location"], ops._ptr(gt), b, m, ops._ptr(set_cls),
                                len(case["class_names"]), ops._ptr(mt), ops._ptr(um),
                                *[ops._ptr(bufs[k][PAD:]) for k in ("labels", "targets", "weights")], ops._ptr(ws), wsb,
                                ops._stream(ws))
    assert rc == 0
    torch.cuda.synchronize()
    for k, t in bufs.items():
        canary = CANARY_I if k == "labels" else CANARY_F
        assert (t[:PAD] == canary).all() and (t[-PAD:] == canary).all(), k
    return {k: t[PAD:-PAD] for k, t in bufs.items()}


@pytest.mark.parametrize("name", ("geometry", "first_argmax"))      # 2 x 510 anchors in 3 frames; 2 anchors
def test_every_output_element_written_and_no_guard_touched(name):
    out, ref = _raw_assign(name), ahr.synth_ref(name)
    assert not (out["labels"] == CANARY_I).any()
    assert not (out["targets"] == CANARY_F).any() and not (out["weights"] == CANARY_F).any()
    shape = ref["labels"].shape
    _check_assign((out["labels"].view(shape), out["targets"].view(*shape, 7), out["weights"].view(shape)), ref,
                  name + " (raw call)")


def test_assignment_two_calls_bitwise_equal():
    first, second = _raw_assign("geometry"), _raw_assign("geometry")
    for k in first:
        assert torch.equal(first[k], second[k]), k


# --------------------------------------------------------------------------------------------------------- losses

def _t(x):
    return None if x is None else torch.from_numpy(x).to(DEV)


def _fused(c):
    from spx import ops
    w = c["weights"]
    out = ops.anchor_loss(_t(c["cls"]), _t(c["box"]), _t(c["dir"]), _t(c["labels"]), _t(c["targets"]), _t(c["anchors"]),
                          c["dir_offset"], w[0], w[1], w[2], beta=c["beta"], alpha=c["alpha"])
    torch.cuda.synchronize()
    return out


def _np64(out):
    return [None if t is None else t.double().cpu().numpy() for t in out]


def _check(case, name, fused, eager, golden):
    e_fused, e_eager = float(np.abs(fused - golden).max()), float(np.abs(eager - golden).max())
    bound = plr.measured_bound(e_eager, golden)
    line = "%-16s %-9s e_fused %.3e  e_eager %.3e  bound %.3e  max|float64| %.3e" % (
        case, name, e_fused, e_eager, bound, float(np.abs(golden).max()))
    print(line)
    assert np.isfinite(fused).all(), (case, name)
    return None if e_fused <= bound else (case, name, e_fused, e_eager, bound)


@pytest.mark.parametrize("name", sorted(ahr.LOSS_CASES))
def test_fused_losses_within_measured_bound(name):
    c = ahr.loss_case(name)
    want = ahr.loss_case_ref(name)
    got = _np64(_fused(c))
    eager = ahr.torch_losses(c, torch.float32, DEV)
    misses = []
    for i, part in enumerate(("loss_cls", "loss_loc", "loss_dir")):
        misses.append(_check(name, part, got[0][i:i + 1], eager[0][i:i + 1], want[0][i:i + 1]))
    for part, a, b, w in zip(("dcls", "dbox", "ddir"), got[1:], eager[1:], want[1:]):
        assert (a is None) == (w is None)
        if a is not None:
            misses.append(_check(name, part, a, b, w))
    # elements the reference gives no weight: exact zeros
    labels, targets = c["labels"], c["targets"]
    assert not got[1][labels < 0].any(), "dcls at label -1"
    assert not got[2][labels <= 0].any(), "dbox at label <= 0"
    assert not got[2][np.isnan(targets)].any(), "dbox at NaN targets"
    if got[3] is not None:
        assert not got[3][labels <= 0].any(), "ddir at label <= 0"
    else:
        assert got[0][2] == 0
    if (labels > 0).any():                                   # and every positive anchor has a live box gradient
        assert np.abs(got[2][labels > 0]).sum(axis=-1).min() > 0
    assert not [m for m in misses if m], [m for m in misses if m]


@pytest.mark.parametrize("name", ("boundary_2", "boundary_4", "boundary_8"))
def test_direction_bin_on_a_boundary_is_the_reference_float32_bin(name):
    """ddir = (softmax - one_hot(bin)) * weight: its only negative entry of a positive anchor names the bin."""
    c = ahr.loss_case(name)
    rec = ahr.golden()["loss_%s_bins32" % name].astype(np.int64)
    ddir = _np64(_fused(c))[3]
    assert ((ddir < 0).sum(axis=-1) == 1).all()
    got = ddir.argmin(axis=-1)
    wrong = np.argwhere(got != rec)
    assert wrong.size == 0, (wrong[:8], got[got != rec][:8], rec[got != rec][:8])


def test_losses_two_calls_bitwise_equal():
    c = ahr.loss_case("a1026_l1")
    first, second = _fused(c), _fused(c)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------- the fixture head, end to end

def _head_step(head, feat, gt, loss_fn):
    x = feat.clone().requires_grad_(True)
    head.zero_grad()
    if feat.dtype == torch.float32:
        head({"spatial_features_2d": x, "gt_boxes": gt, "batch_size": gt.shape[0]})
    else:                              # forward() casts its input to float32: the same two steps without the cast
        head.forward_ret_dict = dict(zip(("cls_preds", "box_preds", "dir_cls_preds"), head._heads(x)))
        head.forward_ret_dict.update(head.assign_targets(gt_boxes=gt))
    loss, tb = loss_fn(head)
    loss.backward()
    parts = np.array([float(tb["rpn_loss_cls"]), float(tb["rpn_loss_loc"]), float(tb["rpn_loss_dir"])])
    grads = [p.grad.double().cpu().numpy() for p in (head.conv_cls.weight, head.conv_box.weight,
                                                     head.conv_dir_cls.weight, x)]
    return parts, grads


def test_fixture_head_end_to_end():
    """Forward, get_loss() and backward of the 32 x 40 head: the fused path against loss_ref on the same predictions and
    against the same head in float64 on the CPU; the float32 torch path of the same head measures the bound."""
    g = ahr.modules()
    head = ahr.fixture_head(DEV)
    feat, gt = torch.from_numpy(g["head_feat"]).to(DEV), torch.from_numpy(g["head_gt"]).to(DEV)
    parts, grads = _head_step(head, feat, gt, lambda h: h.get_loss())
    assert head._fused_loss_ok()
    fr = head.forward_ret_dict
    assert fr["box_cls_labels"].dtype == torch.int32
    assert np.array_equal(fr["box_cls_labels"].cpu().numpy(), g["head_box_cls_labels"])
    cfg, w = head.model_cfg, head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
    view = lambda key, n: fr[key].detach().cpu().numpy().reshape(2, -1, n)
    want_parts = ahr.loss_ref(view("cls_preds", 3), view("box_preds", 7), view("dir_cls_preds", 2),
                              fr["box_cls_labels"].cpu().numpy(), fr["box_reg_targets"].cpu().numpy(),
                              head._flat_anchors().reshape(-1, 7).cpu().numpy(), cfg.DIR_OFFSET, w["cls_weight"],
                              w["loc_weight"], w["dir_weight"], head.reg_loss_func.beta, head.cls_loss_func.alpha,
                              cfg.NUM_DIR_BINS)[0]
    e_parts, e_grads = _head_step(head, feat, gt, lambda h: h.get_loss_torch())
    head64 = ahr.fixture_head("cpu", torch.float64)
    _, want_grads = _head_step(head64, feat.double().cpu(), gt.double().cpu(), lambda h: h.get_loss_torch())
    assert np.array_equal(head64.forward_ret_dict["box_cls_labels"].numpy(), g["head_box_cls_labels"])
    misses = [_check("fixture head", n, parts[i:i + 1], e_parts[i:i + 1], want_parts[i:i + 1])
              for i, n in enumerate(("loss_cls", "loss_loc", "loss_dir"))]
    misses += [_check("fixture head", n, a, b, c) for n, a, b, c in
               zip(("d_conv_cls", "d_conv_box", "d_conv_dir", "d_features"), grads, e_grads, want_grads)]
    assert not [m for m in misses if m], [m for m in misses if m]


def test_graph_capture_of_assignment_and_loss():
    """Assignment and loss (with its gradients) captured in one graph on one stream, replayed twice on new gt boxes
    copied into the static input: bitwise the eager result.  Capture fails on any host read."""
    g = ahr.modules()
    head = ahr.fixture_head(DEV)
    with torch.no_grad():
        head({"spatial_features_2d": torch.from_numpy(g["head_feat"]).to(DEV), "batch_size": 2,
              "gt_boxes": torch.from_numpy(g["head_gt"]).to(DEV)})
    preds = {k: head.forward_ret_dict[k].detach().clone().requires_grad_(True)
             for k in ("cls_preds", "box_preds", "dir_cls_preds")}
    edge = torch.from_numpy(ahr.fixture_edge_batch()).to(DEV)
    static_gt = edge[[0, 1]].clone()

    def step(gt):
        head.forward_ret_dict = dict(preds)
        head.forward_ret_dict.update(head.assign_targets(gt_boxes=gt))
        loss, tb = head.get_loss()
        return (loss.detach(), head.forward_ret_dict["box_cls_labels"], head.forward_ret_dict["box_reg_targets"],
                tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb["rpn_loss_dir"]) + torch.autograd.grad(loss, list(preds.values()))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static_gt)
    torch.cuda.current_stream().wait_stream(side)
    assert head._fused_loss_ok()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(static_gt)
    seen = []
    for frames in ([2, 0], [3, 1]):
        static_gt.copy_(edge[frames])
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        want = step(edge[frames].clone())
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        seen.append(got[1])
    assert not torch.equal(seen[0], seen[1]) and int((seen[0] > 0).sum()) > 0
