"""Float64 numpy restatement of the centre head's losses and their gradients (csrc/center_loss.hip, include/spx.h §22):
the two weighted losses, the unweighted per-column reg_loss, d_hm w.r.t. the LOGIT in closed form and the regression
gradients with duplicate cells summed; the cases the tests run it on; and the project's own torch composition
(CenterHead.sigmoid + loss_utils, as CenterHead.get_loss chains them) on any device and dtype, to compare against."""
import numpy as np
import torch

import center_targets_ref as ctr

HEAD_CHANNELS = (2, 1, 3, 2)        # center, center_z, dim, rot (+ vel 2)
LO, HI = 1e-4, 1 - 1e-4


def restate(hm, heatmap, regs, target_boxes, inds, masks, code_weights, cls_weight=1.0, loc_weight=1.0):
    """hm, heatmap (B, C, H, W); regs: list of (B, d_i, H, W); target_boxes (B, K, D); inds, masks (B, K) ->
    dict(losses (2), reg_loss (D), d_hm, d_regs) in float64.  A slot with masks == 0 is never read."""
    x, gt = np.asarray(hm, np.float64), np.asarray(heatmap, np.float64)
    with np.errstate(over="ignore"):
        s = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    inside = (s >= LO) & (s <= HI)
    p = np.clip(s, LO, HI)
    q = 1 - p
    pos = gt == 1
    w = (1 - gt) ** 4
    term = np.where(pos, np.log(p) * q ** 2, np.log(q) * p ** 2 * w)
    # d term / d logit, with dp / dx = p q inside the clamp and 0 outside
    dterm = np.where(pos, q ** 2 * (q - 2 * p * np.log(p)), w * p ** 2 * (2 * q * np.log(q) - p)) * inside
    num_pos = max(int(pos.sum()), 1)
    hm_loss = -term.sum() / num_pos
    d_hm = -dterm / num_pos * cls_weight

    regs = [np.asarray(r, np.float64) for r in regs]
    pred_map = np.concatenate(regs, axis=1)
    b, d = pred_map.shape[:2]
    flat = pred_map.reshape(b, d, -1)
    cw = np.asarray(code_weights, np.float64)
    tb = np.asarray(target_boxes, np.float64)
    num = max(int((np.asarray(masks) == 1).sum()), 1)
    col_sum = np.zeros(d)
    grad = np.zeros_like(flat)
    for f in range(b):
        for k in range(tb.shape[1]):
            if masks[f, k] != 1:
                continue
            diff = flat[f, :, int(inds[f, k])] - tb[f, k]
            col_sum += np.abs(diff)
            grad[f, :, int(inds[f, k])] += np.sign(diff) * cw * loc_weight / num
    reg_loss = col_sum / num
    grad = grad.reshape(pred_map.shape)
    edges = np.cumsum([0] + [r.shape[1] for r in regs])
    return dict(losses=np.array([hm_loss * cls_weight, (reg_loss * cw).sum() * loc_weight]), reg_loss=reg_loss, d_hm=d_hm,
                d_regs=[grad[:, edges[i]:edges[i + 1]] for i in range(len(regs))])


def composition(case, dtype, device):
    """CenterHead.get_loss's chain for one head on `device` in `dtype`, with autograd: the same dict as restate, as
    float64 numpy arrays."""
    from pcdet_amd.utils import loss_utils
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)           # noqa: E731
    hm = t(case["hm"]).to(dtype).requires_grad_(True)
    regs = [t(r).to(dtype).requires_grad_(True) for r in case["regs"]]
    pred = torch.clamp(hm.sigmoid(), min=1e-4, max=1 - 1e-4)
    hm_loss = loss_utils.FocalLossCenterNet()(pred, t(case["heatmap"]).to(dtype)) * case["cls_weight"]
    reg_loss = loss_utils.RegLossCenterNet()(torch.cat(regs, dim=1), t(case["masks"]), t(case["inds"]),
                                             t(case["target_boxes"]).to(dtype))
    loc_loss = (reg_loss * t(np.asarray(case["code_weights"], np.float64)).to(dtype)).sum() * case["loc_weight"]
    (hm_loss + loc_loss).backward()
    n = lambda v: v.detach().double().cpu().numpy()                              # noqa: E731
    return dict(losses=np.array([n(hm_loss), n(loc_loss)]), reg_loss=n(reg_loss), d_hm=n(hm.grad),
                d_regs=[n(r.grad) for r in regs])


def restate_case(case):
    return restate(case["hm"], case["heatmap"], case["regs"], case["target_boxes"], case["inds"], case["masks"],
                   case["code_weights"], case["cls_weight"], case["loc_weight"])


def split_regs(pred_map, vel=False):
    ch = HEAD_CHANNELS + ((2,) if vel else ())
    edges = np.cumsum((0,) + ch)
    return [np.ascontiguousarray(pred_map[:, edges[i]:edges[i + 1]]) for i in range(len(ch))]


def _case(hm, heatmap, pred_map, tb, inds, masks, code_weights, cls_weight=1.0, loc_weight=2.0):
    return dict(hm=np.asarray(hm, np.float32), heatmap=np.asarray(heatmap, np.float32),
                regs=split_regs(np.asarray(pred_map, np.float32), vel=pred_map.shape[1] == 10),
                target_boxes=np.asarray(tb, np.float32), inds=np.asarray(inds, np.int64),
                masks=np.asarray(masks, np.int64), code_weights=[float(v) for v in code_weights],
                cls_weight=float(cls_weight), loc_weight=float(loc_weight))


def golden_targets(gold):
    """The recorded reference targets of the LOSS_CASES frames, head 0, stacked: heatmap (3, 3, H, W), target_boxes
    (3, 8, 8), inds, mask (3, 8)."""
    keys = [k[:-len("heatmap")] for name in ctr.LOSS_CASES for k in sorted(gold)
            if k.startswith("a/%s/h0/" % name) and k.endswith("heatmap")]
    return tuple(np.stack([gold[k + out] for k in keys]) for out in ("heatmap", "target_boxes", "inds", "mask"))


def golden_case(gold, empty=False):
    """c/logits, c/regs, c/weights and the LOSS_CASES targets (weights 1, as the fixture was recorded); empty: the all-zero
    heatmap of c/hm_empty (the num_pos == 0 branch)."""
    heat, tb, inds, mask = golden_targets(gold)
    return _case(gold["c/logits"], np.zeros_like(heat) if empty else heat, gold["c/regs"], tb, inds, mask,
                 gold["c/weights"], 1.0, 1.0)


def random_case(seed, b, c, h, w, k, live, d=8, dup=(), cls_weight=1.0, loc_weight=2.0):
    """A synthetic batch: Gaussian-looking heatmap values in [0, 1) with exact ones at the live cells of channel
    (slot % c), logits N(-2, 1.5), `live` live slots per frame on distinct cells, then for every (frame, slots) of `dup`
    the later slots moved onto the first one's cell.  Dead slots are zero-filled, as center_assign_targets leaves them."""
    rng = np.random.default_rng(seed)
    hm = rng.normal(-2.0, 1.5, size=(b, c, h, w)).astype(np.float32)
    heat = (rng.uniform(0, 1, size=(b, c, h, w)) ** 6 * 0.98).astype(np.float32)
    pred = rng.normal(0, 1, size=(b, d, h, w)).astype(np.float32)
    tb = np.zeros((b, k, d), np.float32)
    inds, masks = np.zeros((b, k), np.int64), np.zeros((b, k), np.int64)
    for f in range(b):
        cells = rng.permutation(h * w)[:live]
        inds[f, :live], masks[f, :live] = cells, 1
        tb[f, :live] = rng.normal(0, 1, size=(live, d)).astype(np.float32)
    for f, slots in dup:
        inds[f, list(slots[1:])] = inds[f, slots[0]]
    for f in range(b):
        for s in range(live):
            heat[f, s % c].reshape(-1)[inds[f, s]] = 1.0
    weights = [1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.2, 0.2, 0.75, 0.75][:d]
    return _case(hm, heat, pred, tb, inds, masks, weights, cls_weight, loc_weight)


CLAMP_LOGITS = (9.0, -9.0, 9.5, -9.5, 20.0, -20.0, 100.0, -100.0)
CLAMP_INSIDE = (True, True, False, False, False, False, False, False)


def clamp_case():
    """The logits of CLAMP_LOGITS on positive cells (channel 0, frame 0, cells 0 .. 7, heatmap 1) and on negative cells
    (channel 1, frame 0, cells 0 .. 7).  +/-9.0 lies inside the clamp (sigmoid(-9.0) ~ 1.23e-4), the others outside
    (sigmoid(-9.5) ~ 7.5e-5); logit(1e-4) ~ -9.2102, so float32 rounding cannot move any of them across the bound."""
    case = random_case(11, 2, 3, ctr.H, ctr.W, 8, 3)
    case["heatmap"][0, 0].reshape(-1)[:8] = 1.0
    assert (case["heatmap"][0, 1].reshape(-1)[:8] < 1).all()
    case["hm"][0, 0].reshape(-1)[:8] = CLAMP_LOGITS
    case["hm"][0, 1].reshape(-1)[:8] = CLAMP_LOGITS
    return case


DUP = ((0, (1, 4)), (1, (0, 2, 5)))     # frame 0: slots 1 and 4 share a cell; frame 1: slots 0, 2 and 5


def dup_case():
    """Two and three live slots of a frame on one cell; column 3 of frame 1's slot 3 predicts its target exactly (sign 0);
    on the triple cell column 0 has the signs +, +, - and column 1 the signs +, -, 0, so sums of mixed signs occur."""
    case = random_case(12, 2, 3, ctr.H, ctr.W, 8, 6, dup=DUP)
    pred = np.concatenate(case["regs"], axis=1)
    cell = lambda f, s: pred[f].reshape(8, -1)[:, case["inds"][f, s]]            # noqa: E731
    case["target_boxes"][1, 3, 3] = cell(1, 3)[3]
    v = cell(1, 0)
    case["target_boxes"][1, (0, 2, 5), 0] = v[0] - 1, v[0] - 2, v[0] + 1
    case["target_boxes"][1, (0, 2, 5), 1] = v[1] - 1, v[1] + 1, v[1]
    return case


def dead_rewritten(case):
    """The same case with every dead slot pointing at a cell a live slot of its frame uses, and a large finite target."""
    out = dict(case, inds=case["inds"].copy(), target_boxes=case["target_boxes"].copy())
    for f in range(out["inds"].shape[0]):
        live = np.flatnonzero(out["masks"][f] == 1)
        for n, s in enumerate(np.flatnonzero(out["masks"][f] == 0)):
            out["inds"][f, s] = out["inds"][f, live[n % len(live)]]
            out["target_boxes"][f, s] = 1e30 * (-1) ** n
    return out


def cases():
    """name -> case, the synthetic ones (the golden batch needs the fixture: golden_case)."""
    c = {"clamp": clamp_case(), "dup": dup_case()}
    c["all_dead"] = random_case(13, 2, 3, ctr.H, ctr.W, 8, 0)
    c["all_dead"]["heatmap"][:] = np.minimum(c["all_dead"]["heatmap"], 0.9)     # no positives either: the -neg branch
    c["tail_tiny"] = random_case(14, 1, 1, 7, 5, 1, 1)
    c["tail_odd"] = random_case(15, 5, 2, 47, 61, 9, 7, dup=((2, (0, 3)),))
    c["vel"] = random_case(16, 2, 3, ctr.H, ctr.W, 8, 5, d=10, dup=((0, (2, 3)),))
    return c


def full_size_case():
    """One full-size plane set: B = 2, C = 3, 200 x 176, K = 500 with 40 live: the summation order at the workload's length."""
    return random_case(17, 2, 3, 200, 176, 500, 40)
