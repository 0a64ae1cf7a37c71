"""pointnet2_batch HIP kernels (csrc/pointnet2.hip) against the float32 numpy restatement (tests/pointnet2_ref.py):
indices and counts bit-exact, forwards exact, backwards deterministic and close to float64 torch."""
import numpy as np
import pytest
import torch

import pointnet2_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _pu():
    from pcdet_amd.ops.pointnet2.pointnet2_batch import pointnet2_utils as pu
    return pu


def _frames(batch, n, seed=0):
    """KITTI-shaped synthetic frames, n points each sampled with replacement when a frame has fewer."""
    from pcdet_amd.datasets import synthetic as syn
    rng = np.random.default_rng(seed)
    out = []
    for i in range(batch):
        pts = syn.make_frame(1, i)["points"][:, :3]
        out.append(pts[rng.choice(pts.shape[0], n, replace=pts.shape[0] < n)])
    return np.ascontiguousarray(np.stack(out).astype(np.float32))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def kitti():
    xyz = _frames(4, 16384)
    idx = ref.furthest_point_sample(4096, xyz=xyz)
    return xyz, idx


def test_dfps_kitti_shape(kitti):
    xyz, want = kitti
    got = _pu().furthest_point_sample(_g(xyz), 4096)
    assert got.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_pu().farthest_point_sample(_g(xyz), 4096).cpu().numpy(), want)


def test_sfps_kitti_shape(kitti):
    xyz, idx = kitti
    sub = np.take_along_axis(xyz, idx[..., None].astype(np.int64), axis=1)
    w = np.random.default_rng(1).uniform(size=sub.shape[:2]).astype(np.float32)
    w[:, ::7] = 0.0                                            # clamped to 1e-12 in the ranking
    want = ref.furthest_point_sample(512, xyz=sub, weights=w)
    got = _pu().furthest_point_sample_weights(_g(sub), _g(w), 512)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 100, 1000, 1024, 1500, 4096])
def test_fps_lattice_ties(n):
    rng = np.random.default_rng(n)
    xyz = rng.integers(0, 3, size=(2, n, 3)).astype(np.float32)
    w = rng.integers(0, 3, size=(2, n)).astype(np.float32)
    for npoint in sorted({1, min(n, 7), n, n + 3}):
        got = _pu().furthest_point_sample(_g(xyz), npoint).cpu().numpy()
        assert np.array_equal(got, ref.furthest_point_sample(npoint, xyz=xyz)), (n, npoint)
        got = _pu().furthest_point_sample_weights(_g(xyz), _g(w), npoint).cpu().numpy()
        assert np.array_equal(got, ref.furthest_point_sample(npoint, xyz=xyz, weights=w)), (n, npoint)


def test_fps_matrix_forms():
    pu = _pu()
    xyz = _frames(2, 4096, seed=3)
    mat = pu.calc_dist_matrix_for_sampling(_g(xyz))
    m = mat.cpu().numpy()
    want = ref.furthest_point_sample(512, matrix=m)
    assert np.array_equal(pu.furthest_point_sample_matrix(mat, 512).cpu().numpy(), want)
    assert np.array_equal(pu.furthest_point_sample_with_dist(mat, 512).cpu().numpy(), want)
    w = np.random.default_rng(4).uniform(size=(2, 4096)).astype(np.float32)
    got = pu.furthest_point_sample_with_weighted_dist(mat, _g(w), 512).cpu().numpy()
    assert np.array_equal(got, ref.furthest_point_sample(512, matrix=m, weights=w))


def test_fps_general_path_waymo_size():
    rng = np.random.default_rng(5)
    xyz = (rng.uniform(-75, 75, size=(1, 163840, 3)) * np.array([1, 1, 0.04])).astype(np.float32)
    got = _pu().furthest_point_sample(_g(xyz), 512).cpu().numpy()
    assert np.array_equal(got, ref.furthest_point_sample(512, xyz=xyz))
    w = rng.uniform(size=(1, 163840)).astype(np.float32)
    got = _pu().furthest_point_sample_weights(_g(xyz), _g(w), 64).cpu().numpy()
    assert np.array_equal(got, ref.furthest_point_sample(64, xyz=xyz, weights=w))


@pytest.fixture(scope="module")
def bq_data(kitti):
    xyz, idx = kitti
    xyz = xyz[:2]
    centres = np.take_along_axis(xyz, idx[:2, :512, None].astype(np.int64), axis=1)
    off = (centres + np.float32(0.05)).astype(np.float32)
    return xyz, centres, off


@pytest.mark.parametrize("r_in,r_out", [(0.0, 0.2), (0.2, 0.4), (0.4, 0.8), (0.0, 200.0), (0.0, 0.0)])
def test_ball_query(bq_data, r_in, r_out):
    pu = _pu()
    xyz, centres, off = bq_data
    for c in (centres, off):
        want_cnt, want_idx = ref.ball_query(xyz, c, 32, r_out, r_in=r_in)
        if r_in == 0.0:
            cnt, idx = pu.ball_query(r_out, 32, _g(xyz), _g(c))
        else:
            cnt, idx = pu.ball_query_dilated(r_in, r_out, 32, _g(xyz), _g(c))
        assert np.array_equal(cnt.cpu().numpy(), want_cnt)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
    if r_out == 200.0:
        assert (want_cnt == 32).all()


def test_ball_query_empty_shells_on_points(bq_data):
    xyz, centres, _ = bq_data
    cnt, idx = _pu().ball_query_dilated(1e-3, 2e-3, 8, _g(xyz), _g(centres))
    want_cnt, want_idx = ref.ball_query(xyz, centres, 8, 2e-3, r_in=1e-3)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt) and np.array_equal(idx.cpu().numpy(), want_idx)
    assert (want_cnt == 0).any()


def test_three_nn(bq_data):
    xyz, centres, off = bq_data
    for known in (centres, off, centres[:, :2]):
        d, idx = _pu().three_nn(_g(xyz[:, :4096]), _g(known))
        want_d2, want_idx = ref.three_nn(xyz[:, :4096], known)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        assert np.array_equal(d.cpu().numpy(), np.sqrt(torch.from_numpy(want_d2)).numpy())


def _index_add_ref(grad_out, idx, n, weight=None):
    """float64 torch scatter-add: grad_out (B, C, E) over flat idx (B, E) [* weight (B, E)] -> (B, C, n)."""
    g = grad_out.double()
    if weight is not None:
        g = g * weight.double()[:, None, :]
    out = torch.zeros(g.shape[0], g.shape[1], n, dtype=torch.float64, device=g.device)
    for b in range(g.shape[0]):
        out[b].index_add_(1, idx[b].long(), g[b])
    return out


def _check_bwd(got, want):
    tol = 1e-6 * max(1.0, float(want.abs().max()))
    assert float((got.double() - want).abs().max()) <= tol


def test_grouping_and_gather(bq_data):
    pu = _pu()
    xyz, centres, _ = bq_data
    _, idx = pu.ball_query(0.8, 32, _g(xyz), _g(centres))
    feats = torch.randn(2, 4, xyz.shape[1], device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    f = feats.clone().requires_grad_(True)
    out = pu.grouping_operation(f, idx)
    assert out.shape == (2, 4, 512, 32)
    assert np.array_equal(out.detach().cpu().numpy(), ref.group_points(feats.cpu().numpy(), idx.cpu().numpy()))
    go = torch.randn_like(out)
    g1, = torch.autograd.grad(out, f, go)
    g2, = torch.autograd.grad(pu.grouping_operation(f, idx), f, go)
    assert torch.equal(g1, g2)
    _check_bwd(g1, _index_add_ref(go.reshape(2, 4, -1), idx.reshape(2, -1), xyz.shape[1]))

    gidx = _pu().furthest_point_sample(_g(xyz), 512)
    out = pu.gather_operation(f, gidx)
    assert np.array_equal(out.detach().cpu().numpy(), ref.group_points(feats.cpu().numpy(), gidx.cpu().numpy()))
    go = torch.randn_like(out)
    g1, = torch.autograd.grad(out, f, go)
    g2, = torch.autograd.grad(pu.gather_operation(f, gidx), f, go)
    assert torch.equal(g1, g2)
    _check_bwd(g1, _index_add_ref(go, gidx, xyz.shape[1]))


def test_three_interpolate(bq_data):
    pu = _pu()
    xyz, centres, _ = bq_data
    dist, idx = pu.three_nn(_g(xyz[:, :4096]), _g(centres))
    recip = 1.0 / (dist + 1e-8)
    weight = (recip / recip.sum(dim=2, keepdim=True)).contiguous()
    feats = torch.randn(2, 8, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    f = feats.clone().requires_grad_(True)
    out = pu.three_interpolate(f, idx, weight)
    want = ref.three_interpolate(feats.cpu().numpy(), idx.cpu().numpy(), weight.cpu().numpy())
    assert np.array_equal(out.detach().cpu().numpy(), want)
    go = torch.randn_like(out)
    g1, = torch.autograd.grad(out, f, go)
    g2, = torch.autograd.grad(pu.three_interpolate(f, idx, weight), f, go)
    assert torch.equal(g1, g2)
    want_g = _index_add_ref(go.repeat_interleave(3, dim=2), idx.reshape(2, -1), 512, weight.reshape(2, -1))
    _check_bwd(g1, want_g)


def test_sa_like_chain_forward_backward():
    """FPS -> gather -> QueryAndGroupDilated -> 1x1 conv / BN / ReLU -> max-pool -> three_nn / three_interpolate back
    to the input points, against the same chain in float64 torch on the restatement's indices."""
    pu = _pu()
    xyz = _frames(2, 2048, seed=7)
    torch.manual_seed(0)
    feats = torch.randn(2, 6, 2048, dtype=torch.float64)
    conv = torch.nn.Conv2d(9, 16, 1).double()
    bn = torch.nn.BatchNorm2d(16).double()

    def chain(x, f, fps_idx, ball_idx, nn_idx, lib):
        if lib:
            new_xyz = pu.gather_operation(x.transpose(1, 2).contiguous(), fps_idx).transpose(1, 2).contiguous()
            _, grouped, _ = pu.QueryAndGroupDilated(0.2, 1.6, 16)(x, new_xyz, f)
        else:
            gx = lambda t, i: torch.stack([t[b][:, i[b].long()] for b in range(t.shape[0])])
            new_xyz = gx(x.transpose(1, 2), fps_idx).transpose(1, 2)
            gxyz = gx(x.transpose(1, 2), ball_idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
            grouped = torch.cat([gxyz, gx(f, ball_idx)], dim=1)
        h = torch.relu(bn(conv(grouped))).max(dim=3)[0]                    # (B, 16, 256)
        if lib:
            dist, nn_i = pu.three_nn(x, new_xyz)
        else:
            nn_i = nn_idx
            d2 = torch.stack([((x[b][:, None, :] - new_xyz[b][nn_i[b].long()]) ** 2).sum(-1) for b in range(2)])
            dist = torch.sqrt(d2)
        recip = 1.0 / (dist + 1e-8)
        w = recip / recip.sum(dim=2, keepdim=True)
        if lib:
            return pu.three_interpolate(h, nn_i, w.contiguous())
        return torch.stack([(h[b][:, nn_i[b].long()] * w[b][None]).sum(-1) for b in range(2)])

    fps_idx = ref.furthest_point_sample(256, xyz=xyz)
    centres = np.take_along_axis(xyz, fps_idx[..., None].astype(np.int64), axis=1)
    _, ball_idx = ref.ball_query(xyz, centres, 16, 1.6, r_in=0.2)
    _, nn_idx = ref.three_nn(xyz, centres)

    conv.to(DEV).float(), bn.to(DEV).float()
    fg = feats.float().to(DEV).requires_grad_(True)
    out = chain(_g(xyz), fg, pu.furthest_point_sample(_g(xyz), 256), None, None, True)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    out.backward(go.float().to(DEV))
    g_lib = (fg.grad.double().cpu(), conv.weight.grad.double().cpu())
    conv.zero_grad()
    conv.cpu().double(), bn.cpu().double()
    fd = feats.clone().requires_grad_(True)
    out_ref = chain(torch.from_numpy(xyz).double(), fd, torch.from_numpy(fps_idx), torch.from_numpy(ball_idx),
                    torch.from_numpy(nn_idx), False)
    out_ref.backward(go)
    assert float((out.detach().double().cpu() - out_ref.detach()).abs().max()) <= 1e-4 * max(1.0, float(out_ref.abs().max()))
    for got, want in zip(g_lib, (fd.grad, conv.weight.grad)):
        assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


def test_graph_capture_replay():
    pu = _pu()
    xyz = _g(_frames(2, 4096, seed=9))
    feats = torch.randn(2, 4, 4096, device=DEV, generator=torch.Generator(DEV).manual_seed(3))

    def step():
        idx = pu.furthest_point_sample(xyz, 512)
        centres = pu.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        cnt, bidx = pu.ball_query_dilated(0.2, 0.8, 32, xyz, centres)
        return idx, cnt, bidx, pu.grouping_operation(feats, bidx)

    eager = step()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                      # warm the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, static):
        assert torch.equal(a, b)
