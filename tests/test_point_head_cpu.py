"""The fast_cpc point head, its box coder and the 3DSSD detector without a GPU: state_dict keys against the reference
class, PointBinResidualCoder against values recorded from the reference coder, the float64 restatement of the fused
tail (tests/point_head_ref.py) against the literal transcription of the reference eval forward, and the host-side
argument checks of the two HIP entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import point_head_configs as phc
import point_head_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _head(dataset="kitti", seed=0):
    from pcdet_amd.models import dense_heads
    torch.manual_seed(seed)
    return dense_heads.__all__["PointHeadVoteSASAStatisticDistillation"](model_cfg=phc.head_cfg(dataset),
                                                                         **phc.head_kwargs())


def randomize(head, seed):
    """Random BN running statistics and affine, conv biases and a non-zero object_statistic_features (with the
    default zeros every class logit would equal its bias)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
            elif isinstance(m, torch.nn.Conv1d) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
        head.object_statistic_features.copy_(torch.rand(head.object_statistic_features.shape, generator=g) * 1.5)
    return head


@pytest.mark.parametrize("dataset", ["kitti", "waymo"])
def test_head_state_dict_keys_and_shapes_match_reference(dataset):
    want = json.load(open(os.path.join(GOLDEN, "point_head_state_keys.json")))[dataset]
    got = [[k, list(v.shape)] for k, v in _head(dataset).state_dict().items()]
    assert got == want


def test_detector_builds_from_config_with_only_backbone_and_head_state():
    from pcdet_amd.models.detectors import __all__ as detectors, build_detector
    net = build_detector(phc.model_cfg(), 3, phc.dataset())
    assert type(net) is detectors["3DSSD"]
    assert net.point_head is not None and net.dense_head is None
    keys = list(net.state_dict())
    assert all(k == "global_step" or k.startswith(("backbone_3d.", "point_head.")) for k in keys)
    want = json.load(open(os.path.join(GOLDEN, "point_head_state_keys.json")))["kitti"]
    assert [[k[len("point_head."):], list(v.shape)] for k, v in net.state_dict().items()
            if k.startswith("point_head.")] == want
    assert [type(m).__name__ for m in net.module_list] == ["VoxelPointNet2FSMSGDistillation",
                                                           "PointHeadVoteSASAStatisticDistillation"]


def test_training_mode_raises():
    from pcdet_amd.models.detectors import build_detector
    head = _head()
    head.train()
    with pytest.raises(NotImplementedError, match="training"):
        head({"batch_size": 1})
    net = build_detector(phc.model_cfg(), 3, phc.dataset())
    net.train()
    with pytest.raises(NotImplementedError, match="training"):
        net({"batch_size": 1})


@pytest.mark.parametrize("mean", [False, True])
def test_point_bin_coder_matches_reference_values(mean):
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    z = np.load(os.path.join(GOLDEN, "point_bin_coder.npz"))
    tag = "mean" if mean else "plain"
    coder = PointBinResidualCoder(use_mean_size=mean, angle_bin_num=12,
                                  mean_size=[[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])
    assert coder.code_size == 30
    cls = torch.from_numpy(z["classes"])
    enc = coder.encode_torch(torch.from_numpy(z["boxes"].copy()), torch.from_numpy(z["points"]), cls)
    np.testing.assert_array_equal(enc.numpy(), z["encode_" + tag])
    dec = coder.decode_torch(torch.from_numpy(z["enc"]), torch.from_numpy(z["points"]), cls)
    np.testing.assert_array_equal(dec.numpy(), z["decode_" + tag])
    # the recorded inputs cover tied bins: all-equal rows decode to bin 0, the two-way ties to the first of the two
    step = np.float32(2 * np.pi / 12)
    e = z["enc"]
    np.testing.assert_array_equal(dec.numpy()[:8, 6], (np.float32(0) + e[:8, 6 + 12]) * step)
    np.testing.assert_array_equal(dec.numpy()[8:16, 6], (np.float32(3) + e[8:16, 6 + 12 + 3]) * step)


def test_point_bin_coder_round_trip():
    from pcdet_amd.utils.box_coder_utils import PointBinResidualCoder
    coder = PointBinResidualCoder(use_mean_size=False, angle_bin_num=12)
    g = torch.Generator().manual_seed(3)
    boxes = torch.cat([torch.randn(50, 3, generator=g) * 20, torch.rand(50, 3, generator=g) * 4 + 0.2,
                       torch.rand(50, 1, generator=g) * 6.0], 1).double()
    pts = boxes[:, :3] + torch.randn(50, 3, generator=g).double()
    back = coder.decode_torch(coder.encode_torch(boxes.clone(), pts), pts)
    assert torch.allclose(back, boxes, atol=1e-9)


@pytest.mark.parametrize("b,n,lo,hi", [(2, 64, 0, 40), (3, 37, 5, 37), (1, 1, 0, 1)])
def test_restatement_matches_reference_transcription(b, n, lo, hi):
    head = randomize(_head(seed=b), seed=10 + n).double().eval()
    head.model_cfg.SAMPLE_RANGE = [lo, hi]
    g = torch.Generator().manual_seed(n)
    coords = torch.cat([torch.arange(b).repeat_interleave(n)[:, None].double(),
                        torch.randn(b * n, 3, generator=g).double() * 10], 1)
    pf = torch.randn(b * n, 128, generator=g).double()
    with torch.no_grad():
        cand, vote_t, bidx = ref.transcribe_vote(head, coords, pf, b)
        feat_ncw = pf.reshape(b, n, -1).permute(0, 2, 1).numpy()
        vote_r, _ = ref.vote(feat_ncw, coords[:, 1:4].reshape(b, n, 3).numpy(), lo, hi,
                             ref.mlp_params(head.s_vote_layers), head.s_vote_cfg.MAX_TRANSLATION_RANGE)
        np.testing.assert_allclose(vote_r, vote_t.numpy(), rtol=1e-12, atol=1e-12)
        assert torch.equal(cand, coords[:, 1:4].reshape(b, n, 3)[:, lo:hi])
        nv = hi - lo
        feats = torch.relu(torch.randn(b, 256, nv, generator=g).double())
        vflat = vote_t.reshape(-1, 3)
        cls_t, reg_t, box_t, bbox_t = ref.transcribe_tail(head, feats, vflat)
        r = ref.predict(feats.numpy(), head.object_statistic_features.numpy(), vflat.numpy(),
                        [ref.mlp_params(m) for m in head.s_cls_block], ref.mlp_params(head.s_reg_layers), 12)
    np.testing.assert_allclose(r["cls"], cls_t.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["reg"], reg_t.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(r["box"], box_t.numpy(), rtol=1e-10, atol=1e-10)
    assert torch.equal(box_t, bbox_t)
    # the statistic matters: with zero statistics every logit is the class block's output at x = 0
    assert np.ptp(r["cls"][:, 0]) > 1e-3 or r["cls"].shape[0] == 1


def test_entry_points_validate_arguments_without_gpu():
    from spx import _lib
    lib = _lib.load()
    mlp = _lib.PointMlp()
    rng = _lib.f_arr([3.0, 3.0, 2.0])
    p = ctypes.c_void_p(16)
    # shapes this build has no kernel for: SPX_ERR_UNSUPPORTED
    assert lib.spx_point_vote(p, p, 2, 512, 512, 0, 512, ctypes.byref(mlp), 128, rng, p, None) == -3
    assert lib.spx_point_vote(p, p, 2, 128, 512, 0, 512, ctypes.byref(mlp), 256, rng, p, None) == -3
    cls = (_lib.PointMlp * 9)()
    assert lib.spx_point_head_predict(p, p, p, 2, 256, 512, 9, cls, 64, ctypes.byref(mlp), 128, 12, p, p, p,
                                      None) == -3
    assert lib.spx_point_head_predict(p, p, p, 2, 256, 512, 3, cls, 64, ctypes.byref(mlp), 128, 33, p, p, p,
                                      None) == -3
    # null parameter pointers, a bad column range: SPX_ERR_INVALID_ARG, before any launch
    assert lib.spx_point_vote(p, p, 2, 128, 512, 0, 512, ctypes.byref(mlp), 128, rng, p, None) == -1
    assert lib.spx_point_vote(p, p, 2, 128, 512, 10, 600, ctypes.byref(mlp), 128, rng, p, None) == -1
    assert lib.spx_point_head_predict(p, p, p, 2, 256, 512, 3, cls, 64, ctypes.byref(mlp), 128, 12, p, p, p,
                                      None) == -1
    # nothing to do is not an error
    assert lib.spx_point_vote(None, None, 0, 128, 512, 0, 512, ctypes.byref(mlp), 128, rng, None, None) == 0
