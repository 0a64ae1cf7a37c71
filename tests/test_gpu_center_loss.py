"""The fused centre-head losses on the GPU (csrc/center_loss.hip, include/spx.h §22, spx.ops.center_head_loss,
CenterHead.get_loss_fused) against the float64 restatement (tests/center_loss_ref.py, itself pinned to the reference's
recorded values by tests/test_center_loss_ref.py).

Accuracy rule, per output tensor: e_fused = max |fused - float64| <= point_loss_ref.measured_bound(e_eager, float64),
e_eager being the error of this tree's float32 torch composition on the same device.  Both errors are printed (run with
-s) and appended to profiles/center_loss_accuracy.log.  Also: exact zeros outside the clamp and off the live cells,
bitwise reproducibility, dead slots that reach nothing, full definition of the outputs, the NaN-target rule, the head
level with one and two heads, graph capture with backward, and one CenterPoint train step."""
import functools
import os

import numpy as np
import pytest
import torch

import center_loss_ref as clr
import center_targets_ref as ctr
import point_loss_ref as plr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "center_loss_accuracy.log")
YAML = os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/centerpoint.yaml")


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _op(case):
    """The op's raw outputs (losses, reg_loss, d_hm, d_regs) as device tensors."""
    from spx import ops
    return ops.center_head_loss(_g(case["hm"]), _g(case["heatmap"]), [_g(r) for r in case["regs"]],
                                _g(case["target_boxes"]), _g(case["inds"]), _g(case["masks"]), case["code_weights"],
                                case["cls_weight"], case["loc_weight"])


def _as_dict(out):
    n = lambda v: v.detach().double().cpu().numpy()                              # noqa: E731
    return dict(losses=n(out[0]), reg_loss=n(out[1]), d_hm=n(out[2]), d_regs=[n(r) for r in out[3]])


def _bits(out):
    return [t.cpu().numpy().tobytes() for t in (out[0], out[1], out[2], *out[3])]


def _tensors(d):
    yield "losses", d["losses"]
    yield "reg_loss", d["reg_loss"]
    yield "d_hm", d["d_hm"]
    for i, r in enumerate(d["d_regs"]):
        yield "d_regs[%d]" % i, r


def _log(lines):
    print("\n".join(lines))
    try:
        with open(LOG, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    except OSError:
        pass


def _within_rule(name, fused, eager, golden):
    """Every (name, tensor) of the three dicts / lists of pairs under the accuracy rule; prints and logs both errors."""
    lines, bad = [], []
    for (key, f), (_, e), (_, g) in zip(fused, eager, golden):
        assert f.shape == g.shape == e.shape, key
        e_eager, e_fused = float(np.abs(e - g).max()), float(np.abs(f - g).max())
        bound = plr.measured_bound(e_eager, g)
        lines.append("%-12s %-24s max|golden| %.4e  e_eager %.3e  e_fused %.3e  bound %.3e"
                     % (name, key, float(np.abs(g).max()), e_eager, e_fused, bound))
        if not e_fused <= bound:
            bad.append(lines[-1])
    _log(lines)
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def _synthetic():
    return dict(clr.cases(), full_size=clr.full_size_case())


@functools.lru_cache(maxsize=None)
def _golden(name):
    return clr.restate_case(_synthetic()[name])


def _check(name, case=None, golden=None):
    case = _synthetic()[name] if case is None else case
    golden = _golden(name) if golden is None else golden
    out = _op(case)
    fused, eager = _as_dict(out), clr.composition(case, torch.float32, DEV)
    for key, t in _tensors(fused):
        assert np.isfinite(t).all(), key
    _within_rule(name, list(_tensors(fused)), list(_tensors(eager)), list(_tensors(golden)))
    return out, fused


def _off_live_cells_are_zero(case, fused):
    b, hw = case["hm"].shape[0], case["hm"].shape[2] * case["hm"].shape[3]
    live = np.zeros((b, hw), bool)
    for f in range(b):
        live[f, case["inds"][f][case["masks"][f] == 1]] = True
    for r in fused["d_regs"]:
        flat = r.reshape(b, r.shape[1], hw)
        assert not flat[np.broadcast_to(~live[:, None, :], flat.shape)].any()
        assert flat[np.broadcast_to(live[:, None, :], flat.shape)].any()


@pytest.mark.parametrize("empty", [False, True], ids=["targets", "no_positives"])
def test_golden_batch(empty):
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "center_head.npz")))
    case = clr.golden_case(gold, empty=empty)
    assert case["hm"].shape == (3, 3, 20, 24) and case["target_boxes"].shape == (3, 8, 8)
    golden = clr.restate_case(case)
    np.testing.assert_allclose(golden["losses"][0], gold["c/hm_empty/loss" if empty else "c/hm/loss"], rtol=1e-10)
    _check("golden_empty" if empty else "golden", case, golden)


def test_clamp_case():
    """+/-9.0 inside the clamp, +/-9.5, +/-20, +/-100 outside, on positive and on negative cells: d_hm exactly 0 at the
    outside cells, not 0 at the inside ones, everything finite."""
    _out, fused = _check("clamp")
    for ch in (0, 1):
        d = fused["d_hm"][0, ch].reshape(-1)[:8]
        assert [bool(v != 0) for v in d] == list(clr.CLAMP_INSIDE), (ch, d)


def test_duplicate_cells():
    """Two and three live slots on one cell, a prediction equal to its target: under the rule against the restatement
    (which sums the duplicates), exact zeros off the live cells and where the sign is 0, two calls bit for bit equal."""
    case = _synthetic()["dup"]
    out, fused = _check("dup")
    _off_live_cells_are_zero(case, fused)
    grads = np.concatenate(fused["d_regs"], axis=1)[1].reshape(8, -1)
    assert grads[3, case["inds"][1, 3]] == 0                    # prediction == target
    assert grads[1, case["inds"][1, 0]] == 0                    # + - 0 on the triple cell
    assert grads[0, case["inds"][1, 0]] != 0
    again = _op(case)
    assert again[2].data_ptr() != out[2].data_ptr()
    assert _bits(again) == _bits(out)


def test_dead_slots_reach_nothing():
    """Dead slots rewritten to cells live slots use, with targets of +/-1e30: every output bit for bit as before."""
    case = _synthetic()["dup"]
    other = clr.dead_rewritten(case)
    dead = case["masks"] == 0
    assert dead.any() and (other["inds"][dead] != case["inds"][dead]).any() and (other["inds"] < 20 * 24).all()
    assert np.abs(other["target_boxes"][dead]).min() >= 1e30
    assert _bits(_op(other)) == _bits(_op(case))


def test_all_dead_batch():
    """masks all 0 and no positive cell: reg_loss and every regression gradient exactly 0, the heatmap term from the
    -neg branch."""
    case = _synthetic()["all_dead"]
    out, fused = _check("all_dead")
    assert not fused["reg_loss"].any() and fused["losses"][1] == 0
    assert all(not r.any() for r in fused["d_regs"])
    assert fused["losses"][0] > 0 and _golden("all_dead")["losses"][0] > 0
    # the same through the composition's -neg_loss branch, written out
    p = np.clip(1 / (1 + np.exp(-case["hm"].astype(np.float64))), 1e-4, 1 - 1e-4)
    neg = (np.log(1 - p) * p ** 2 * (1 - case["heatmap"].astype(np.float64)) ** 4).sum()
    np.testing.assert_allclose(_golden("all_dead")["losses"][0], -neg * case["cls_weight"], rtol=1e-12)


@pytest.mark.parametrize("name", ["tail_tiny", "tail_odd", "vel"])
def test_tails(name):
    """H * W no multiple of the vector width, planes no multiple of the block; D = 10 with a vel map."""
    case = _synthetic()[name]
    _out, fused = _check(name)
    _off_live_cells_are_zero(case, fused)
    assert len(fused["d_regs"]) == (5 if name == "vel" else 4)


def test_full_size_planes():
    """B = 2, C = 3, 200 x 176, K = 500 with 40 live: the summation order at the workload's length."""
    case = _synthetic()["full_size"]
    assert case["hm"].shape == (2, 3, 200, 176) and case["inds"].shape == (2, 500) and int(case["masks"].sum()) == 80
    _out, fused = _check("full_size")
    _off_live_cells_are_zero(case, fused)


def test_outputs_prefilled_with_nan_come_back_defined(monkeypatch):
    """The op writes every element inside its own launches, the zeros of the regression gradients included, and reads
    no workspace word it has not written: allocations that hold NaN before the call change nothing."""
    case = _synthetic()["dup"]
    want = _bits(_op(case))
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_cuda:
            t.view(torch.uint8).fill_(0xFF)     # NaN as float, -1 as int
        return t

    from spx import ops
    ops._WS.clear()                             # the workspace is allocated (and poisoned) afresh
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: poison(real_empty(*a, **kw)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **kw: poison(real_empty_like(*a, **kw)))
    got = _op(case)
    monkeypatch.undo()
    for t in (got[0], got[1], got[2], *got[3]):
        assert torch.isfinite(t).all()
    assert _bits(got) == want


def test_nan_target_in_a_live_slot():
    """A corrupted label still surfaces: that column of reg_loss (and the weighted sum) is NaN, the other columns and the
    focal term are finite."""
    case = _synthetic()["dup"]
    case = dict(case, target_boxes=case["target_boxes"].copy())
    case["target_boxes"][0, 2, 5] = np.nan
    fused = _as_dict(_op(case))
    assert np.isnan(fused["reg_loss"][5]) and np.isfinite(np.delete(fused["reg_loss"], 5)).all()
    assert np.isnan(fused["losses"][1]) and np.isfinite(fused["losses"][0]) and np.isfinite(fused["d_hm"]).all()
    np.testing.assert_array_equal(np.delete(fused["reg_loss"], 5), np.delete(_as_dict(_op(_synthetic()["dup"]))["reg_loss"], 5))


# ------------------------------------------------------------------------------------------------------- the head level

def _head(names_each_head, fused):
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.models.dense_heads import CenterHead
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    head_cfg = cfg.MODEL.DENSE_HEAD
    head_cfg.CLASS_NAMES_EACH_HEAD = names_each_head
    head_cfg.TARGET_ASSIGNER_CONFIG.NUM_MAX_OBJS = 8
    if fused:
        head_cfg.LOSS_CONFIG.FUSED = True
    torch.manual_seed(3)
    return CenterHead(model_cfg=head_cfg, input_channels=32, num_class=3, class_names=list(cfg.CLASS_NAMES),
                      grid_size=np.array([192, 160, 40]), point_cloud_range=np.array(ctr.RANGE, np.float32),
                      voxel_size=list(ctr.VOXEL_SIZE), predict_boxes_when_training=False).to(DEV)


def _leaves(head, seed, batch=2):
    """Random head outputs as leaves: per head a dict hm / center / center_z / dim / rot."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for sep in head.heads_list:
        d = {}
        for name, spec in sep.sep_head_dict.items():
            t = torch.randn(batch, spec["out_channels"], ctr.H, ctr.W, generator=gen)
            d[name] = ((t * 1.5 - 2.0) if name == "hm" else t).to(DEV).requires_grad_(True)
        out.append(d)
    return out


def _loss_and_grads(head, pred_dicts, targets):
    head.forward_ret_dict = {"pred_dicts": pred_dicts, "target_dicts": targets}
    loss, tb = head.get_loss()
    names = [(i, k) for i, d in enumerate(pred_dicts) for k in d]
    grads = torch.autograd.grad(loss, [pred_dicts[i][k] for i, k in names])
    return loss, tb, dict(zip(names, grads))


@pytest.mark.parametrize("config", ["one_head", "two_heads"])
def test_head_level_fused_against_composition(config):
    """get_loss with LOSS_CONFIG.FUSED and the default composition from the same forward_ret_dict: the loss, every
    tb_dict value and the gradient w.r.t. every head output under the accuracy rule; the float64 golden is the
    composition on the CPU in double."""
    names = {"one_head": [["Car", "Pedestrian", "Cyclist"]], "two_heads": [["Car"], ["Pedestrian", "Cyclist"]]}[config]
    head = _head(names, fused=True)
    head.train()
    pred_dicts = _leaves(head, 21)
    targets = head.assign_targets(_g(ctr.cases()["two_heads"]["gt"]), feature_map_size=(ctr.H, ctr.W))
    assert all(int(m.sum()) > 0 for m in targets["masks"])
    f_loss, f_tb, f_grads = _loss_and_grads(head, pred_dicts, targets)
    head.model_cfg.LOSS_CONFIG.FUSED = False
    e_loss, e_tb, e_grads = _loss_and_grads(head, pred_dicts, targets)
    assert set(f_tb) == set(e_tb) == {"rpn_loss"} | {"%s_loss_head_%d" % (k, i) for k in ("hm", "loc")
                                                     for i in range(len(names))}
    assert f_loss.dim() == 0 and f_loss.requires_grad
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and not v.requires_grad for v in f_tb.values())

    weights = head.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
    order = list(head.separate_head_cfg.HEAD_ORDER)
    c = lambda t: t.detach().cpu().numpy()                                       # noqa: E731
    g_tb, g_grads = {}, {}
    for i, d in enumerate(pred_dicts):
        case = dict(hm=c(d["hm"]), heatmap=c(targets["heatmaps"][i]), regs=[c(d[k]) for k in order],
                    target_boxes=c(targets["target_boxes"][i]), inds=c(targets["inds"][i]), masks=c(targets["masks"][i]),
                    code_weights=list(weights["code_weights"]), cls_weight=weights["cls_weight"],
                    loc_weight=weights["loc_weight"])
        gold = clr.composition(case, torch.float64, "cpu")
        g_tb["hm_loss_head_%d" % i], g_tb["loc_loss_head_%d" % i] = gold["losses"]
        g_grads[(i, "hm")] = gold["d_hm"]
        g_grads.update({(i, k): g for k, g in zip(order, gold["d_regs"])})
    g_tb["rpn_loss"] = sum(g_tb.values())
    n = lambda t: np.asarray(c(t), np.float64)                                   # noqa: E731
    keys = sorted(g_tb)
    pairs = lambda tb, loss: [("loss", loss)] + [(k, np.asarray(tb[k])) for k in keys]   # noqa: E731
    fused = pairs({k: n(v) for k, v in f_tb.items()}, n(f_loss)) + [("d %s[%d]" % (k, i), n(f_grads[i, k])) for i, k in sorted(g_grads)]
    eager = pairs({k: n(v) for k, v in e_tb.items()}, n(e_loss)) + [("d %s[%d]" % (k, i), n(e_grads[i, k])) for i, k in sorted(g_grads)]
    golden = pairs(g_tb, np.asarray(g_tb["rpn_loss"])) + [("d %s[%d]" % (k, i), g_grads[i, k]) for i, k in sorted(g_grads)]
    _within_rule("head/" + config, fused, eager, golden)


def test_assign_targets_fused_loss_and_backward_capture_in_a_graph():
    """assign_targets + fused get_loss + backward to the head-output leaves under torch.cuda.graph (any host read fails
    the capture); a replay with other boxes in the static tensor gives, bit for bit, the loss and gradients of an eager
    fused call on those boxes."""
    head = _head([["Car", "Pedestrian", "Cyclist"]], fused=True)
    head.train()
    pred_dicts = _leaves(head, 22)
    leaves = [pred_dicts[0][k] for k in pred_dicts[0]]
    first, second = _g(ctr.cases()["two_heads"]["gt"]), _g(ctr.cases()["padding"]["gt"])
    static_gt = first.clone()

    def step(gt):
        targets = head.assign_targets(gt, feature_map_size=(ctr.H, ctr.W))
        head.forward_ret_dict = {"pred_dicts": pred_dicts, "target_dicts": targets}
        loss, _tb = head.get_loss()
        return loss, torch.autograd.grad(loss, leaves), targets["masks"][0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static_gt)                                     # warm-up: workspaces, autograd's lazy initialisation
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_loss, g_grads, g_masks = step(static_gt)
    static_gt.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    e_loss, e_grads, e_masks = step(second)
    f_loss, _f_grads, f_masks = step(first)
    assert int(g_masks.sum()) == int(e_masks.sum()) == 3 and int(f_masks.sum()) == 8
    assert torch.isfinite(e_loss) and f_loss.item() != e_loss.item()
    assert g_loss.view(torch.int32).item() == e_loss.detach().view(torch.int32).item()
    for g, e in zip(g_grads, e_grads):
        assert g.abs().sum() > 0 and torch.equal(g.view(torch.int32), e.view(torch.int32))


def test_centerpoint_train_step_with_fused_loss():
    """One CenterPoint train step with LOSS_CONFIG.FUSED on the reduced synthetic geometry: a finite loss, the tb_dict
    keys of the default path, a finite non-zero gradient on every dense-head parameter."""
    from pcdet_amd.config import AttrDict, cfg_from_yaml_file
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models import build_network
    cfg = cfg_from_yaml_file(YAML, AttrDict())
    cfg.MODEL.DENSE_HEAD.LOSS_CONFIG.FUSED = True
    ds = SyntheticDataset(cfg.DATA_CONFIG, cfg.CLASS_NAMES, True, cfg_id=0)
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, ds).to(DEV)
    batch = ds.collate_batch([ds[0], ds[1]])
    batch = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    model.train()
    model.zero_grad(set_to_none=True)
    ret, tb_dict, _disp = model(dict(batch))
    loss = ret["loss"]
    assert model.dense_head.model_cfg.LOSS_CONFIG.FUSED is True
    assert loss.dim() == 0 and torch.isfinite(loss)
    assert set(tb_dict) == {"loss_rpn", "hm_loss_head_0", "loc_loss_head_0", "rpn_loss"}
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in tb_dict.values())
    assert int(model.dense_head.forward_ret_dict["target_dicts"]["masks"][0].sum()) > 0
    loss.backward()
    for name, p in model.dense_head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
