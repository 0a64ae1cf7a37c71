"""spx.ops.roi_grid_pool_bev (csrc/roi_grid_pool.hip, include/spx.h §25) against the float64 restatement
tests/proposal_targets_ref.roi_grid_pool, itself pinned to the reference's SECONDHead.roi_grid_pool by
tests/test_roi_head_ref.py.

Accuracy rule, per case: e_op = max |op - float64| <= 4 * e_torch, e_torch being the error of the float32 torch composition
(SECONDHead.roi_grid_pool_torch: affine_grid + grid_sample) on the same device against the same values.  Both errors are
printed (run with -s) and appended to profiles/roi_grid_pool_accuracy.log.  Shapes: a 5 x 7 map, C = 3 / 64 / 65 (below,
at and one past the 64-channel LDS tile of the channels_last path), G = 1 / 2 / 7 (an even G * G is padded to an odd LDS
row), N = 1 / 130, dense NCHW and channels_last.  RoIs (proposal_targets_ref.pool_rois): axis-aligned inside, 30 degrees,
heading +-pi, straddling each border, wholly outside, zero extent, the padding row, then random ones."""
import functools
import os

import numpy as np
import pytest
import torch

import proposal_targets_ref as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "roi_grid_pool_accuracy.log")
GEOM = (P.POOL["min_x"], P.POOL["min_y"], P.POOL["step_x"], P.POOL["step_y"])


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(c, n):
    return P.pool_rois(n, seed=n), P.pool_features(c, seed=c)


@functools.lru_cache(maxsize=None)
def _want(c, g, n):
    rois, feat = _inputs(c, n)
    return P.roi_grid_pool(rois, feat, g, *GEOM)


def _features(feat, layout):
    t = _g(feat)
    if layout == "channels_last":
        t = t.contiguous(memory_format=torch.channels_last)
        assert t.stride(1) == 1
    return t


def _op(rois, feat, g, d_n=None):
    from spx import ops
    return ops.roi_grid_pool_bev(rois, feat, g, *GEOM, d_n=d_n)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("n", [1, 130])
@pytest.mark.parametrize("g", [1, 2, 7])
@pytest.mark.parametrize("c", [3, 64, 65])
def test_op_matches_float64_restatement(c, g, n, layout):
    from pcdet_amd.models.roi_heads import SECONDHead
    rois, feat = _inputs(c, n)
    want = _want(c, g, n)
    d_rois, d_feat = _g(rois), _features(feat, layout)
    got = _op(d_rois, d_feat, g)
    assert got.shape == (2 * n, c, g, g) and got.dtype == torch.float32 and got.is_contiguous()
    eager = SECONDHead.roi_grid_pool_torch(d_rois, d_feat, g, *GEOM)
    e_op = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    e_torch = float(np.abs(eager.cpu().numpy().astype(np.float64) - want).max())
    line = "c %-3d g %d n %-3d %-13s e_op %.3e  e_torch %.3e  max|f64| %.3e" % (c, g, n, layout, e_op, e_torch,
                                                                              float(np.abs(want).max()))
    print("\n" + line)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(line + "\n")
    except OSError:
        pass
    assert e_op <= 4 * e_torch, line
    outside = P.taps_all_outside(rois, P.POOL["h"], P.POOL["w"], g, *GEOM)           # (2 n, G, G)
    zeros = got.cpu().numpy()[np.broadcast_to(outside[:, None], want.shape)]
    assert (zeros == 0).all()
    if n > 1:
        assert outside.any() and not outside.all() and np.abs(want).max() > 0.5


def test_named_rois_do_what_they_are_there_for():
    rois = P.pool_rois(130)
    out = P.taps_all_outside(rois, P.POOL["h"], P.POOL["w"], 7, *GEOM)
    assert not out[0].any() and not out[1].all()            # inside: every cell has a tap on the map
    assert out[8].all() and out[9].all()                    # wholly outside
    for k in (4, 5, 6, 7):                                  # straddling a border: some cells on, some off the map
        assert out[k].any() and not out[k].all(), k
    want = _want(3, 7, 130)
    assert np.ptp(want[10].reshape(3, -1), axis=1).max() == 0      # zero extent: every sample at the centre
    np.testing.assert_allclose(want[2], want[3], atol=1e-6)          # heading +pi and -pi: the same grid


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_live_count_leaves_zero_rows(layout):
    rois, feat = _inputs(65, 130)
    d_rois, d_feat = _g(rois), _features(feat, layout)
    full = _op(d_rois, d_feat, 7)
    for live in (0, 131, 260, 400):
        d_n = torch.tensor([live], dtype=torch.int64, device=DEV)
        poisoned = d_rois.clone()
        poisoned.view(-1, 7)[min(live, 260):] = float("nan")         # dead RoIs are not read
        got = _op(poisoned, d_feat, 7, d_n=d_n)
        k = min(live, 260)
        assert torch.equal(got[:k].view(torch.int32), full[:k].view(torch.int32))
        assert not got[k:].view(torch.int32).any()


def test_strided_views_and_extra_roi_columns():
    rois, feat = _inputs(64, 130)
    want = _want(64, 2, 130)
    wide = np.concatenate([rois, np.full((2, 130, 2), 7.0, np.float32)], 2)            # (B, N, 9): 7 + C columns
    big = _g(np.pad(feat, ((0, 0), (0, 3), (0, 2), (0, 1))))                           # a view into a larger map
    got = _op(_g(wide), big[:, :64, :5, :7], 2)
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_two_runs_and_graph_replay_are_bitwise_equal(layout):
    rois, feat = _inputs(65, 130)
    other = P.pool_rois(130, seed=77)
    d_feat = _features(feat, layout)
    static = _g(rois)
    a, b = _op(static, d_feat, 7), _op(static, d_feat, 7)
    assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.int32), b.view(torch.int32))
    eager_other = _op(_g(other), d_feat, 7)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _op(static, d_feat, 7)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _op(static, d_feat, 7)
    static.copy_(_g(other))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager_other.view(torch.int32))
    assert not torch.equal(out.view(torch.int32), a.view(torch.int32))


def test_no_gradient_is_declared():
    rois, feat = _inputs(3, 1)
    d_feat = _features(feat, "nchw").requires_grad_(True)
    assert not _op(_g(rois), d_feat, 2).requires_grad
