"""The fast_cpc point head's fused eval tail (csrc/point_head.hip, include/spx.h §14), the head module and the 3DSSD
detector, on the GPU.

Ops: spx_point_vote and spx_point_head_predict against the float64 restatement (tests/point_head_ref.py) at the KITTI
and Waymo shapes and odd ones, every output element written, the decode against PointBinResidualCoder.decode_torch,
bitwise repeatability and graph capture.  Module: the head's eval forward on real backbone output against the literal
transcription of the reference forward on the same module.  Detector: eval forward to pred_dicts, post-processing
against a transcription of the reference's, and a checkpoint round trip.

Tolerances: an fp32 output y of a two-layer MLP differs from float64 by at most 2e-6 * A + 1e-6, where A is the
absolute sum sum|w . x| through both layers (the restatement returns it); ~256-term fp32 dot products stay well inside."""
import copy
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

import point_head_configs as phc
import point_head_ref as ref
from test_point_head_cpu import randomize

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BINS = 12
RANGE = [3.0, 3.0, 2.0]


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _params(seq):
    c1, bn, _, c2 = seq
    return (c1.weight, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.eps, c2.weight, c2.bias)


def _mlp(c_in, h, c_out, g):
    """A random Conv1d -> BN -> ReLU -> Conv1d stack (eval) on the GPU."""
    seq = torch.nn.Sequential(torch.nn.Conv1d(c_in, h, 1, bias=False), torch.nn.BatchNorm1d(h), torch.nn.ReLU(),
                              torch.nn.Conv1d(h, c_out, 1, bias=True))
    with torch.no_grad():
        seq[0].weight.copy_(torch.randn(seq[0].weight.shape, generator=g) * (2.0 / c_in) ** 0.5)
        seq[1].running_mean.copy_(torch.randn(h, generator=g) * 0.2)
        seq[1].running_var.copy_(torch.rand(h, generator=g) + 0.5)
        seq[1].weight.copy_(torch.rand(h, generator=g) + 0.5)
        seq[1].bias.copy_(torch.randn(h, generator=g) * 0.2)
        seq[3].weight.copy_(torch.randn(seq[3].weight.shape, generator=g) * (1.0 / h) ** 0.5)
        seq[3].bias.copy_(torch.randn(c_out, generator=g) * 0.1)
    return seq.eval().to(DEV)


class Case:
    def __init__(self, b, n, lo=0, hi=None, nc=3, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.b, self.n, self.lo, self.hi, self.nc = b, n, lo, (n if hi is None else hi), nc
        self.vote_mlp = _mlp(128, 128, 3, g)
        self.cls_mlps = [_mlp(256, 64, 1, g) for _ in range(nc)]
        self.reg_mlp = _mlp(256, 128, 6 + 2 * BINS, g)
        self.stat = (torch.rand(nc, 256, generator=g) * 1.5).to(DEV)
        self.vfeat = torch.randn(b, 128, n, generator=g).to(DEV)
        self.xyz = (torch.randn(b, n, 3, generator=g) * 20).to(DEV)
        nv = self.hi - self.lo
        self.feat = torch.relu(torch.randn(b, 256, nv, generator=g)).to(DEV)
        self.vxyz = (torch.randn(b * nv, 3, generator=g) * 20).to(DEV)

    def vote(self):
        from spx import ops
        return ops.point_vote(self.vfeat, self.xyz, self.lo, self.hi, _params(self.vote_mlp), RANGE)

    def predict(self, feat=None):
        from spx import ops
        return ops.point_head_predict(self.feat if feat is None else feat, self.stat, self.vxyz,
                                      [_params(m) for m in self.cls_mlps], _params(self.reg_mlp), BINS)

    def restated(self):
        v, v_abs = ref.vote(self.vfeat.cpu().numpy(), self.xyz.cpu().numpy(), self.lo, self.hi,
                            ref.mlp_params(self.vote_mlp), RANGE)
        p = ref.predict(self.feat.cpu().numpy(), self.stat.cpu().numpy(), self.vxyz.cpu().numpy(),
                        [ref.mlp_params(m) for m in self.cls_mlps], ref.mlp_params(self.reg_mlp), BINS)
        return v, v_abs, p


def _tol(a_abs):
    return 2e-6 * a_abs + 1e-6


SHAPES = {
    "kitti_b1": dict(b=1, n=512),
    "kitti_b2": dict(b=2, n=512),
    "kitti_b16": dict(b=16, n=512),
    "waymo_b4": dict(b=4, n=3072),
    "n1": dict(b=2, n=1),
    "n37": dict(b=3, n=37),
    "lo_gt_0": dict(b=2, n=100, lo=13, hi=77),
    "one_class": dict(b=2, n=45, nc=1),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_ops_match_float64_restatement(name):
    c = Case(seed=len(name), **SHAPES[name])
    vote = c.vote()
    cls, reg, box = c.predict()
    torch.cuda.synchronize()
    v_ref, v_abs, r = c.restated()
    v = vote.cpu().numpy()
    assert v.shape == v_ref.shape == (c.b, c.hi - c.lo, 3)
    assert np.all(np.abs(v - v_ref) <= _tol(v_abs) + 2e-6 * np.abs(v_ref))
    cls, reg, box = cls.cpu().numpy(), reg.cpu().numpy(), box.cpu().numpy()
    assert np.all(np.abs(cls - r["cls"]) <= _tol(r["cls_abs"]))
    assert np.all(np.abs(reg - r["reg"]) <= _tol(r["reg_abs"]))
    reg_tol = _tol(r["reg_abs"])
    assert np.all(np.abs(box[:, :3] - r["box"][:, :3]) <= reg_tol[:, :3] + 2e-6 * np.abs(r["box"][:, :3]))
    assert np.all(np.abs(box[:, 3:6] - r["box"][:, 3:6]) <= r["box"][:, 3:6] * (1.01 * reg_tol[:, 3:6] + 1e-6))
    # the heading: same bin wherever the float64 winner leads by more than the rounding error
    bins = r["reg"][:, 6:6 + BINS]
    top2 = np.sort(bins, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * reg_tol[:, 6:6 + BINS].max(axis=1)
    assert clear.mean() > 0.9
    step = 2 * np.pi / BINS
    res_tol = reg_tol[np.arange(len(r["bin"])), 6 + BINS + r["bin"]]
    assert np.all(np.abs(box[clear, 6] - r["box"][clear, 6]) <= step * (res_tol[clear] + 1e-6) + 1e-6)


def test_vote_clamps_and_propagates_nan():
    c = Case(b=2, n=64, seed=3)
    with torch.no_grad():
        c.vote_mlp[3].bias.copy_(torch.tensor([50.0, -50.0, 0.0]))
        c.vote_mlp[3].weight[2].zero_()
    vote = c.vote()
    off = (vote - c.xyz).cpu()
    assert torch.all((off[..., 0] - 3.0).abs() < 1e-4) and torch.all((off[..., 1] + 3.0).abs() < 1e-4)
    assert torch.all((off[..., 2] - 0.0).abs() < 1e-4)
    with torch.no_grad():
        c.vote_mlp[3].bias[2] = float("nan")
    vote = c.vote().cpu()
    assert torch.isnan(vote[..., 2]).all() and torch.isfinite(vote[..., :2]).all()


def test_nan_prefilled_outputs_are_fully_overwritten():
    from spx import _lib, ops
    lib = _lib.load()
    c = Case(b=3, n=37, lo=2, hi=35, seed=5)
    want_v = c.vote()
    want = c.predict()
    nv = c.hi - c.lo
    vote = torch.full((c.b, nv, 3), float("nan"), device=DEV)
    outs = [torch.full((c.b * nv, k), float("nan"), device=DEV) for k in (c.nc, 6 + 2 * BINS, 7)]
    vd, h, keep = ops._point_mlp(_params(c.vote_mlp), 128, 3, DEV)
    rc = lib.spx_point_vote(ctypes.c_void_p(c.vfeat.data_ptr()), ctypes.c_void_p(c.xyz.data_ptr()), c.b, 128, c.n,
                            c.lo, c.hi, ctypes.byref(vd), h, _lib.f_arr(RANGE), ctypes.c_void_p(vote.data_ptr()),
                            ops._stream(vote))
    assert rc == 0
    descs = [ops._point_mlp(_params(m), 256, 1, DEV) for m in c.cls_mlps]
    rd = ops._point_mlp(_params(c.reg_mlp), 256, 6 + 2 * BINS, DEV)
    arr = (_lib.PointMlp * c.nc)(*[d[0] for d in descs])
    rc = lib.spx_point_head_predict(ctypes.c_void_p(c.feat.data_ptr()), ctypes.c_void_p(c.stat.data_ptr()),
                                    ctypes.c_void_p(c.vxyz.data_ptr()), c.b, 256, nv, c.nc, arr, 64,
                                    ctypes.byref(rd[0]), 128, BINS, *[ctypes.c_void_p(o.data_ptr()) for o in outs],
                                    ops._stream(vote))
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(vote, want_v)
    for o, w in zip(outs, want):
        assert bool(torch.isfinite(o).all())
        assert torch.equal(o, w)


def test_unsupported_shapes_raise():
    from spx import _lib, ops
    c = Case(b=1, n=8, seed=6)
    g = torch.Generator().manual_seed(0)
    reg33 = _mlp(256, 128, 6 + 2 * 33, g)
    with pytest.raises(_lib.SpxError, match="code -3"):          # bins > 32
        ops.point_head_predict(c.feat, c.stat, c.vxyz, [_params(m) for m in c.cls_mlps], _params(reg33), 33)
    wide = _mlp(256, 160, 1, g)
    with pytest.raises(_lib.SpxError, match="code -3"):          # hidden width > 128
        ops.point_head_predict(c.feat, c.stat, c.vxyz, [_params(wide)] * 3, _params(c.reg_mlp), BINS)
    with pytest.raises(_lib.SpxError, match="code -3"):          # more than 8 classes
        ops.point_head_predict(c.feat, c.stat.repeat(3, 1), c.vxyz, [_params(c.cls_mlps[0])] * 9, _params(c.reg_mlp),
                               BINS)


def _ulp_diff(a, b):
    ai = a.contiguous().view(torch.int32).long()
    bi = b.contiguous().view(torch.int32).long()
    return (ai - bi).abs()


@pytest.mark.parametrize("ties", [False, True])
def test_kernel_box_is_the_coder_decode_of_its_reg(ties):
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    c = Case(b=4, n=512, seed=7)
    if ties:    # bins 3 and 7 (and, for the second half of the rows, all bins) get identical logits
        with torch.no_grad():
            w, bias = c.reg_mlp[3].weight, c.reg_mlp[3].bias
            w[6 + 7].copy_(w[6 + 3])
            bias[6 + 7] = bias[6 + 3] + 0.0
            bias[6 + 3] += 100.0
            bias[6 + 7] += 100.0
    cls, reg, box = c.predict()
    coder = PointBinResidualCoder(use_mean_size=False, angle_bin_num=BINS)
    want = coder.decode_torch(reg, c.vxyz, cls.argmax(-1) + 1)
    assert torch.equal(box[:, :3], want[:, :3])
    assert int(_ulp_diff(box[:, 3:6], want[:, 3:6]).max()) <= 2
    assert torch.equal(box[:, 6], want[:, 6])
    if ties:
        assert torch.equal(reg[:, 6 + 3], reg[:, 6 + 7])
        assert bool((reg[:, 6:6 + BINS].argmax(-1) == 3).all())
        step = np.float32(2 * np.pi / BINS)
        assert torch.equal(box[:, 6], (3.0 + reg[:, 6 + BINS + 3]) * step)


def test_repeat_runs_are_bitwise_equal_and_capture_replays():
    c = Case(b=16, n=512, seed=8)

    def step():
        return (c.vote(),) + c.predict()

    first = step()
    second = step()
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    with torch.no_grad():       # the replay reads the current inputs and weights through the captured pointers
        c.feat.mul_(0.5)
        c.reg_mlp[3].bias.add_(1.0)
    g.replay()
    torch.cuda.synchronize()
    eager = step()
    for a, b in zip(static, eager):
        assert torch.equal(a, b)
    assert not torch.equal(static[2], first[2])


# ------------------------------------------------------------------------------------------------------ module
def _frames(batch, n, seed=0):
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    out = []
    for i in range(batch):
        pts = syn.make_frame(1, i + seed)["points"][:, :4]
        out.append(pts[rng.choice(pts.shape[0], n, replace=pts.shape[0] < n)])
    return np.ascontiguousarray(np.stack(out).astype(np.float32))


def _points(batch, n, seed):
    pts = _frames(batch, n, seed)
    bidx = np.repeat(np.arange(batch, dtype=np.float32), n)[:, None]
    return _g(np.concatenate([bidx, pts.reshape(-1, 4)], axis=1))


def _clone_sp(sp):
    import spx
    return spx.SparseConvTensor(sp.features.detach().clone(), sp.indices.clone(), sp.spatial_shape, sp.batch_size)


def _net(seed=0):
    from pcdet_amd.models.detectors import build_detector
    torch.manual_seed(seed)
    net = build_detector(phc.model_cfg(), 3, phc.dataset())
    randomize(net.point_head, seed + 100)
    g = torch.Generator().manual_seed(seed + 200)
    with torch.no_grad():
        for m in net.backbone_3d.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return net.to(DEV).eval()


HEAD_KEYS = ("s_batch_index", "s_point_candidate_coords", "s_point_vote_coords", "s_point_cls_scores",
             "s_point_box_preds", "batch_cls_preds", "batch_box_preds", "batch_index")


def _head_pair(net, bd):
    """(fused head outputs, transcription outputs) from the same backbone output."""
    head = net.point_head
    b = bd["batch_size"]
    fused = head({k: (_clone_sp(v) if k == "s_last_sp_tensor" else v) for k, v in bd.items()})
    cand, vote_t, bidx = ref.transcribe_vote(head, bd["s_point_coords"], bd["s_point_features"], b)
    coords = bd["s_point_coords"][:, 1:4].view(b, -1, 3).contiguous()
    # the SA step sees the FUSED vote coordinates on both sides: a ball query at the radius edge must not decide the test
    vote_f = fused["s_point_vote_coords"][:, 1:4].reshape(b, -1, 3).contiguous()
    _, f, _, _, _, _, _, _ = head.S_VSA_module(xyz=coords, new_xyz=vote_f, features=bd["s_last_features"],
                                               sp_tensor=_clone_sp(bd["s_last_sp_tensor"]),
                                               centroids=bd["s_last_centroids"],
                                               centroid_voxel_idxs=bd["s_last_centroid_voxel_idxs"])
    f = head.s_shared_fc_layer(f)
    cls_t, reg_t, box_t, bbox_t = ref.transcribe_tail(head, f, vote_f.view(-1, 3))
    bflat = bidx.view(-1, 1)
    want = {"s_batch_index": bflat.squeeze(-1), "s_point_candidate_coords": torch.cat((bflat, cand.view(-1, 3)), -1),
            "s_point_vote_coords": torch.cat((bflat, vote_t.view(-1, 3)), -1),
            "s_point_cls_scores": torch.sigmoid(cls_t), "s_point_box_preds": box_t, "batch_cls_preds": cls_t,
            "batch_box_preds": bbox_t, "batch_index": bflat.squeeze(-1)}
    return fused, want, reg_t


def _close(a, b, tol):
    scale = b.abs().max().clamp_min(1.0)
    return float((a - b).abs().max()) <= tol * float(scale)


def _compare_head(fused, want, reg_t, head):
    for k in ("s_batch_index", "s_point_candidate_coords", "batch_index"):
        assert torch.equal(fused[k], want[k]), k
    assert fused["cls_preds_normalized"] is False
    assert _close(fused["s_point_vote_coords"], want["s_point_vote_coords"], 1e-5)
    for k in ("s_point_cls_scores", "batch_cls_preds"):
        assert _close(fused[k], want[k], 1e-4), k
    assert _close(head.forward_ret_dict["s_point_reg_preds"], reg_t, 1e-4)
    for k in ("s_point_box_preds", "batch_box_preds"):
        a, b = fused[k], want[k]
        assert _close(a[:, :6], b[:, :6], 1e-4), k
        same_bin = (reg_t[:, 6:18].argmax(-1) == head.forward_ret_dict["s_point_reg_preds"][:, 6:18].argmax(-1))
        assert float(same_bin.float().mean()) > 0.99
        assert _close(a[same_bin, 6], b[same_bin, 6], 1e-4), k
    for k in HEAD_KEYS:
        assert not fused[k].requires_grad, k


def test_head_eval_forward_matches_reference_transcription_and_follows_load_state_dict():
    net = _net(seed=1)
    with torch.no_grad():
        bd = net.backbone_3d({"batch_size": 2, "points": _points(2, 16384, seed=31)})
        fused, want, reg_t = _head_pair(net, dict(bd))
    assert fused["batch_cls_preds"].shape == (1024, 3) and fused["batch_box_preds"].shape == (1024, 7)
    _compare_head(fused, want, reg_t, net.point_head)
    first = fused["batch_box_preds"].clone()
    # new values through load_state_dict: the kernels read the module's tensors, nothing cached goes stale
    other = randomize(copy.deepcopy(net.point_head).cpu(), seed=77)
    net.point_head.load_state_dict(other.state_dict())
    with torch.no_grad():
        fused2, want2, reg2 = _head_pair(net, dict(bd))
    _compare_head(fused2, want2, reg2, net.point_head)
    assert not torch.equal(fused2["batch_box_preds"], first)


# ------------------------------------------------------------------------------------------------------ detector
def _ref_post_processing(model_cfg, num_class, batch_dict):
    """Transcription of the reference's Detector3DTemplate.post_processing (detector3d_template.py:207-349) for the
    fast_cpc settings: the batch_index branch, no MULTI_CLASSES_NMS, the fork's multi_thresh; recall records off."""
    from pcdet_amd.models.model_utils import model_nms_utils
    post_process_cfg = model_cfg.POST_PROCESSING
    pred_dicts = []
    for index in range(batch_dict['batch_size']):
        if batch_dict.get('batch_index', None) is not None:
            assert batch_dict['batch_box_preds'].shape.__len__() == 2
            batch_mask = (batch_dict['batch_index'] == index)
        else:
            assert batch_dict['batch_box_preds'].shape.__len__() == 3
            batch_mask = index
        box_preds = batch_dict['batch_box_preds'][batch_mask]
        cls_preds = batch_dict['batch_cls_preds'][batch_mask]
        src_cls_preds = cls_preds
        assert cls_preds.shape[1] in [1, num_class]
        if not batch_dict['cls_preds_normalized']:
            cls_preds = torch.sigmoid(cls_preds)
        cls_preds, label_preds = torch.max(cls_preds, dim=-1)
        label_preds = label_preds + 1
        selected, selected_scores = model_nms_utils.multi_thresh(
            box_scores=cls_preds, box_labels=label_preds, box_preds=box_preds, nms_config=post_process_cfg.NMS_CONFIG,
            score_thresh=post_process_cfg.SCORE_THRESH)
        if post_process_cfg.OUTPUT_RAW_SCORE:
            max_cls_preds, _ = torch.max(src_cls_preds, dim=-1)
            selected_scores = max_cls_preds[selected]
        pred_dicts.append({'pred_boxes': box_preds[selected], 'pred_scores': selected_scores,
                           'pred_labels': label_preds[selected]})
    return pred_dicts


def test_detector_eval_forward_post_processing_and_checkpoint_round_trip(tmp_path):
    net = _net(seed=2)
    points = _points(2, 16384, seed=41)
    with torch.no_grad():
        preds, recall = net({"batch_size": 2, "points": points.clone()})
        assert len(preds) == 2 and isinstance(recall, dict)
        for p in preds:
            assert p["pred_boxes"].shape[1] == 7 and p["pred_scores"].shape == p["pred_labels"].shape
        out = {"batch_size": 2, "points": points.clone()}
        for m in net.module_list:
            out = m(out)
    m0, m1 = out["batch_index"] == 0, out["batch_index"] == 1
    assert int(m0.sum()) == int(m1.sum()) == 512
    assert not torch.equal(out["batch_box_preds"][m0], out["batch_box_preds"][m1])     # the two frames differ
    # random-init logits sit near -4.6: replace them by distinct, well-separated values so NMS has work, and keep the
    # head's boxes; both post-processings get the same tensors
    g = torch.Generator().manual_seed(4)
    shape = out["batch_cls_preds"].shape
    logits = torch.linspace(-3.0, 4.0, shape.numel())[torch.randperm(shape.numel(), generator=g)].view(shape).to(DEV)
    out["batch_cls_preds"] = logits
    with torch.no_grad():
        got, _ = net.post_processing(dict(out))
        want = _ref_post_processing(net.model_cfg, net.num_class, dict(out))
    assert sum(p["pred_boxes"].shape[0] for p in got) > 0
    for a, b in zip(got, want):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(a[k], b[k]), k
    # checkpoint round trip through load_params_from_file
    path = os.path.join(str(tmp_path), "ckpt.pth")
    torch.save({"model_state": {k: v.cpu() for k, v in net.state_dict().items()}}, path)
    net2 = _net(seed=9).cpu()
    net2.load_params_from_file(path, logging.getLogger("point_head_test"), to_cpu=True)
    net2.to(DEV).eval()
    with torch.no_grad():
        preds2, _ = net2({"batch_size": 2, "points": points.clone()})
    for a, b in zip(preds, preds2):
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(a[k], b[k]), k
