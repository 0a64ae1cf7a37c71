"""The float64 restatement of gather-project (tests/group_project_ref.py) against a literal transcription of what the
reference does before its first 1x1 conv: gather, subtract the centre, cat xyz and features, zero empty balls, conv."""
import numpy as np
import pytest

import group_project_ref as gp


def _literal(F, Wf, Wx, xyz, ctr, idx, empty, batch):
    """gather -> subtract -> cat -> mask -> Conv2d(k=1), one column at a time in float64."""
    m, s = idx.shape
    npoint = m // batch
    parts = []
    if Wx is not None:
        parts.append(Wx)
    if Wf is not None:
        parts.append(Wf)
    W = np.concatenate(parts, axis=1).astype(np.float64)
    y = np.zeros((batch, W.shape[0], npoint, s))
    for q in range(m):
        bi, p = divmod(q, npoint)
        for j in range(s):
            r = idx[q, j]
            chans = []
            if Wx is not None:
                chans.append(xyz[r].astype(np.float64) - ctr[q].astype(np.float64))
            if Wf is not None:
                chans.append(F[r].astype(np.float64))
            col = np.concatenate(chans)
            if empty[q]:
                col = np.zeros_like(col)
            y[bi, :, p, j] = W @ col
    return y


@pytest.mark.parametrize("form", ["both", "wf_only", "wx_only"])
def test_forward_matches_literal_composition(form):
    rng = np.random.default_rng(3)
    c = gp.make_case(rng, batch=2, n=40, npoint=6, nsample=5, c_in=4, c_out=7, empty_frac=0.3)
    Wx = None if form == "wf_only" else c["W"][:, :3]
    Wf = None if form == "wx_only" else c["W"][:, 3:]
    F = None if form == "wx_only" else c["F"]
    assert c["empty"].any() and not c["empty"].all()
    got = gp.forward(F, Wf, Wx, c["xyz"], c["ctr"], c["idx"], c["empty"], 2)
    want = _literal(F, Wf, Wx, c["xyz"], c["ctr"], c["idx"], c["empty"], 2)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert np.all(got.transpose(0, 2, 1, 3)[c["empty"].reshape(2, 6)] == 0.0)


@pytest.mark.parametrize("form", ["both", "wf_only", "wx_only"])
def test_backward_matches_finite_differences_of_literal(form):
    rng = np.random.default_rng(4)
    c = gp.make_case(rng, batch=2, n=12, npoint=3, nsample=4, c_in=2, c_out=3, empty_frac=0.34)
    F = None if form == "wx_only" else c["F"].astype(np.float64)
    Wf = None if form == "wx_only" else c["W"][:, 3:].astype(np.float64)
    Wx = None if form == "wf_only" else c["W"][:, :3].astype(np.float64)
    dy = rng.standard_normal((2, 3, 3, 4))
    dF, dWf, dWx = gp.backward(dy, F, Wf, Wx, c["xyz"], c["ctr"], c["idx"], c["empty"])

    def loss(args):
        return float((_literal(args["F"], args["Wf"], args["Wx"], c["xyz"], c["ctr"], c["idx"], c["empty"], 2)
                      * dy).sum())

    eps = 1e-6
    base = {"F": F, "Wf": Wf, "Wx": Wx}
    for name, got in (("F", dF), ("Wf", dWf), ("Wx", dWx)):
        arr = base[name]
        if arr is None:
            assert got is None
            continue
        num = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            hi, lo = arr.copy(), arr.copy()
            hi[i] += eps
            lo[i] -= eps
            num[i] = (loss({**base, name: hi}) - loss({**base, name: lo})) / (2 * eps)
        np.testing.assert_allclose(got, num, rtol=1e-6, atol=1e-6, err_msg=name)


def test_rows_of_empty_balls_get_no_gradient():
    rng = np.random.default_rng(5)
    c = gp.make_case(rng, batch=1, n=20, npoint=4, nsample=3, c_in=2, c_out=2, empty_frac=0.0)
    c["empty"][:] = [True, False, True, False]
    c["idx"][0] = 7                        # row 7 is only seen by the empty query 0
    c["idx"][1:] = np.where(c["idx"][1:] == 7, 8, c["idx"][1:])
    dy = rng.standard_normal((1, 2, 4, 3))
    dF, _, _ = gp.backward(dy, c["F"], c["W"][:, 3:], c["W"][:, :3], c["xyz"], c["ctr"], c["idx"], c["empty"])
    assert np.all(dF[7] == 0.0)
