"""CPU suite: tests/sparse_conv_ref.py (the float64 / int64 reference of spx_conv_gemm and spx_conv_wgrad and its table
builders) against DENSE torch convolutions and their autograd, in float64 on a tiny grid, and against the committed
tests/golden/dense_conv_*.npz.  This is what entitles tests/test_gpu_sparse_conv_edges.py to treat it as the truth.
"""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_conv_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "dense_conv_*.npz")))

BATCH, SHAPE, CIN, COUT = 2, (6, 7, 5), 3, 4
RTOL = 1e-12            # float64 on both sides: round-off of another summation order only

# (submanifold, kernel, stride, padding)
CASES = [(True, (3, 3, 3), (1, 1, 1), (1, 1, 1)), (True, (3, 1, 1), (1, 1, 1), (1, 0, 0)),
         (True, (1, 3, 3), (1, 1, 1), (0, 1, 1)), (True, (1, 1, 1), (1, 1, 1), (0, 0, 0)),
         (False, (3, 3, 3), (2, 2, 2), (1, 1, 1)), (False, (3, 1, 1), (2, 1, 1), (0, 0, 0))]


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    err = float(np.abs(a - b).max()) if a.size else 0.0
    assert err <= rtol * max(1.0, float(np.abs(b).max()) if b.size else 1.0), err


def _dense_case(subm, k, s, p, seed):
    """Dense float64 conv3d over the scattered voxels, with autograd: everything the sparse contracts must reproduce."""
    rng = np.random.default_rng(seed)
    cells = BATCH * int(np.prod(SHAPE))
    lin = np.sort(rng.choice(cells, 40, replace=False))
    coords = np.stack(np.unravel_index(lin, (BATCH,) + SHAPE), 1).astype(np.int32)
    feat = rng.standard_normal((coords.shape[0], CIN))
    w = rng.standard_normal((COUT,) + k + (CIN,))
    x = torch.zeros((BATCH, CIN) + SHAPE, dtype=torch.float64)
    x[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]] = torch.from_numpy(feat)
    x.requires_grad_(True)
    wt = torch.from_numpy(w).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
    y = F.conv3d(x, wt, None, s, p)
    if subm:
        fwd, bwd = R.subm_table(coords, SHAPE, k)
        out_coords = coords
        assert tuple(y.shape[2:]) == SHAPE
    else:
        out_coords, fwd, bwd, oshape = R.strided_table(coords, SHAPE, k, s, p)
        assert list(y.shape[2:]) == oshape
        # the active output set is exactly where the dense result can be non-zero, in ascending order
        hit = np.zeros((BATCH,) + tuple(oshape), bool)
        hit[tuple(out_coords.T)] = True
        assert float(y.detach().abs().amax(1)[torch.from_numpy(~hit)].max()) == 0.0
        assert np.array_equal(out_coords, np.argwhere(hit))
    oc = out_coords
    dout = rng.standard_normal((oc.shape[0], COUT))
    dy = torch.zeros_like(y)
    dy[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]] = torch.from_numpy(dout)
    y.backward(dy)
    out = y.detach()[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]].numpy()
    dfeat = x.grad[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]].numpy()
    dw = wt.grad.permute(0, 2, 3, 4, 1).contiguous().numpy()
    return dict(feat=feat, w=w, fwd=fwd, bwd=bwd, dout=dout, out=out, dfeat=dfeat, dw=dw)


def _w_dgrad(w):
    """The weight as the data-gradient gemm takes it: channel axes swapped, [cin, K, cout]."""
    w3 = w.reshape(w.shape[0], -1, w.shape[-1])
    return np.ascontiguousarray(w3.transpose(2, 1, 0))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_reference_equals_dense_conv3d_and_autograd(case):
    subm, k, s, p = CASES[case]
    d = _dense_case(subm, k, s, p, 100 + case)
    K = int(np.prod(k))
    assert d["fwd"].shape[0] == K and (d["fwd"] >= 0).any()
    _close(R.gemm(d["feat"], d["w"], d["fwd"]), d["out"])
    _close(R.gemm(d["dout"], _w_dgrad(d["w"]), d["bwd"]), d["dfeat"])
    if subm:
        _close(R.gemm(d["dout"], _w_dgrad(d["w"]), d["fwd"], flip_k=True), d["dfeat"])
    _close(R.wgrad(d["feat"], d["dout"], d["fwd"], d["w"].shape), d["dw"])
    # the live count: rows beyond it contribute nothing and are not produced
    live = d["fwd"].shape[1] - 3
    part = R.gemm(d["feat"], d["w"], d["fwd"], n_live=live)
    _close(part[:live], d["out"][:live])
    assert np.isnan(part[live:]).all()
    dy = d["dout"].copy()
    dy[live:] = 0.0                           # dout rows beyond the live count must not matter
    _close(R.wgrad(d["feat"], d["dout"], d["fwd"], d["w"].shape, n_live=live),
           R.wgrad(d["feat"], dy, d["fwd"], d["w"].shape))


def test_epilogue_and_integer_path():
    """scale / shift / ReLU, and integer-valued inputs: accumulated in int64, equal to the float64 evaluation, with
    abs_bound() bounding every |partial sum|."""
    rng = np.random.default_rng(5)
    K, n, n_src, cs, cd = 5, 33, 20, 6, 7
    pair = R.random_table(K, n, n_src, 0.4, rng, empty_offsets=(2,))
    assert (pair[2] == -1).all() and pair.max() < n_src and pair.min() == -1
    src = rng.integers(-2, 3, (n_src, cs)).astype(np.float32)
    w = rng.integers(-2, 3, (cd, K, cs)).astype(np.float32)
    scale = rng.choice([0.5, 1.0, 2.0, 4.0], cd)
    shift = rng.integers(-3, 4, cd).astype(np.float64)
    plain = R.gemm(src, w, pair)
    assert np.array_equal(plain, np.rint(plain))
    want = np.zeros((n, cd))
    for k in range(K):
        for o in range(n):
            if pair[k, o] >= 0:
                want[o] += w[:, k, :].astype(np.float64) @ src[pair[k, o]].astype(np.float64)
    assert np.array_equal(plain, want)
    assert np.array_equal(R.gemm(src, w, pair, scale=scale, shift=shift, relu=True), np.maximum(want * scale + shift, 0))
    flipped = R.gemm(src, w, pair, flip_k=True)
    assert np.array_equal(flipped, R.gemm(src, w[:, ::-1, :], pair))
    b = R.abs_bound("gemm", src, w, pair)
    assert np.abs(plain).max() <= b <= K * cs * 4
    assert R.abs_bound("gemm", src, w, pair, scale=scale, shift=shift, relu=True) == \
        (b * scale.max() + np.abs(shift).max()) / 0.5 and scale.min() == 0.5
    dout = rng.integers(-2, 3, (n, cd)).astype(np.float32)
    dw = R.wgrad(src, dout, pair, (cd, K, cs))
    want = np.zeros((cd, K, cs))
    for k in range(K):
        for o in range(n):
            if pair[k, o] >= 0:
                want[:, k, :] += np.outer(dout[o], src[pair[k, o]])
    assert np.array_equal(dw, want) and (dw[:, 2, :] == 0).all()
    assert np.abs(dw).max() <= R.abs_bound("wgrad", src, dout, pair, (cd, K, cs)) <= n * 4
    # dead rows poisoned with NaN are never read; padding stays inside [-1, n_src)
    wide = R.embed_table(pair[:, :20], n_src, rng, cap=n, ld=n + 37)
    assert wide.shape == (K, n + 37) and np.array_equal(wide[:, :20], pair[:, :20])
    assert wide.min() >= -1 and wide.max() < n_src
    dn = dout.copy()
    dn[20:] = np.nan
    assert np.array_equal(R.wgrad(src, dn, wide[:, :n], (cd, K, cs), n_live=20),
                          R.wgrad(src, dout[:20], pair[:, :20], (cd, K, cs)))
    rows = R.random_table(K, 200, n_src, 1.0, rng, rows=(136, 200))
    assert (rows[:, :136] == -1).all() and (rows[:, 136:] >= 0).all()


@pytest.mark.parametrize("path", FIXTURES)
def test_reference_on_golden_dense_conv(path, orc):
    """The committed dense-F.conv3d vectors (float32), at the bars of test_oracle_golden.py; the table builders give the
    oracle's tables entry for entry."""
    d = np.load(path)
    k, s, p = [int(v) for v in d["k"]], [int(v) for v in d["s"]], [int(v) for v in d["p"]]
    shape = [int(v) for v in d["shape"]]
    if d["subm"]:
        fwd, bwd = R.subm_table(d["idx"], shape, k)
        assert np.array_equal(fwd, orc.subm_rulebook(d["idx"], d["shape"], d["k"])[0])
    else:
        out_idx, fwd, bwd, oshape = R.strided_table(d["idx"], shape, k, s, p)
        assert np.array_equal(out_idx, d["out_idx"]) and oshape == [int(v) for v in d["out_spatial"]]
        _oi, o_fwd, o_bwd, _cnt, _os = orc.conv_rulebook(d["idx"], d["shape"], d["k"], d["s"], d["p"])
        assert np.array_equal(fwd, o_fwd) and np.array_equal(bwd, o_bwd)
    assert np.abs(R.gemm(d["feat"], d["w"], fwd) - d["out"]).max() < 2e-6
    assert np.abs(R.gemm(d["dout"], _w_dgrad(d["w"]), bwd) - d["dfeat"]).max() < 5e-6
    if d["subm"]:
        assert np.abs(R.gemm(d["dout"], _w_dgrad(d["w"]), fwd, flip_k=True) - d["dfeat"]).max() < 5e-6
    assert np.abs(R.wgrad(d["feat"], d["dout"], fwd, d["w"].shape) - d["dw"]).max() < 2e-5
