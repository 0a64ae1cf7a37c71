"""float64 numpy restatement of spx_group_project / spx_group_project_bwd (include/spx.h §13).

Queries m = b * npoint + p, slots s, source rows r = idx[m, s] (global); a column is empty when empty[m] is set.
  y[b, o, p, s]  = empty ? 0 : P[r, o] + sum_j Wx[o, j] * (xyz[r, j] - ctr[m, j]),   P = F · Wf^T
  dP[r, o]       = sum of dy[b, o, p, s] over the non-empty columns with idx = r
  dF = dP · Wf,  dWf = dP^T · F,  dWx[o, j] = sum over non-empty columns of dy * (xyz[r, j] - ctr[m, j])
Either of (F, Wf) and Wx may be None."""
import numpy as np


def _cols(idx, empty, n_src):
    m, s = idx.shape
    live = np.ones((m, s), dtype=bool)
    if empty is not None:
        live &= ~np.asarray(empty, dtype=bool)[:, None]
    live &= (idx >= 0) & (idx < n_src)
    return live


def forward(F, Wf, Wx, xyz, ctr, idx, empty, batch):
    """-> y (B, Cout, npoint, S) float64."""
    idx = np.asarray(idx, dtype=np.int64)
    n_src = (F if F is not None else xyz).shape[0]
    live = _cols(idx, empty, n_src)
    r = np.where(live, idx, 0)
    m, s = idx.shape
    c_out = (Wf if Wf is not None else Wx).shape[0]
    y = np.zeros((m, s, c_out))
    if Wf is not None:
        P = np.asarray(F, np.float64) @ np.asarray(Wf, np.float64).T
        y += P[r]
    if Wx is not None:
        rel = np.asarray(xyz, np.float64)[r] - np.asarray(ctr, np.float64)[:, None, :]
        y += rel @ np.asarray(Wx, np.float64).T
    y[~live] = 0.0
    npoint = m // batch
    return y.reshape(batch, npoint, s, c_out).transpose(0, 3, 1, 2).copy()


def backward(dy, F, Wf, Wx, xyz, ctr, idx, empty):
    """dy (B, Cout, npoint, S) -> dF, dWf, dWx (None where the term is absent), float64."""
    idx = np.asarray(idx, dtype=np.int64)
    n_src = (F if F is not None else xyz).shape[0]
    live = _cols(idx, empty, n_src)
    b, c_out, npoint, s = dy.shape
    g = np.asarray(dy, np.float64).transpose(0, 2, 3, 1).reshape(b * npoint, s, c_out) * live[..., None]
    dF = dWf = dWx = None
    if Wf is not None:
        dP = np.zeros((n_src, c_out))
        np.add.at(dP, np.where(live, idx, 0).ravel(), g.reshape(-1, c_out))
        dF = dP @ np.asarray(Wf, np.float64)
        dWf = dP.T @ np.asarray(F, np.float64)
    if Wx is not None:
        rel = np.asarray(xyz, np.float64)[np.where(live, idx, 0)] - np.asarray(ctr, np.float64)[:, None, :]
        dWx = np.einsum("mso,msj->oj", g, rel)
    return dF, dWf, dWx


def make_case(rng, batch, n, npoint, nsample, c_in, c_out, empty_frac=0.1, extent=70.0, radius=3.2):
    """Random inputs at a ball-query-like layout: centres inside the cloud, neighbours within `radius` of them."""
    xyz = rng.uniform(-extent, extent, size=(batch * n, 3)).astype(np.float32)
    centre_rows = np.stack([rng.choice(n, npoint, replace=False) + bi * n for bi in range(batch)]).reshape(-1)
    ctr = (xyz[centre_rows] + rng.uniform(-radius, radius, size=(batch * npoint, 3))).astype(np.float32)
    local = rng.integers(0, n, size=(batch * npoint, nsample))
    idx = (local + (np.arange(batch * npoint) // npoint * n)[:, None]).astype(np.int32)
    empty = rng.random(batch * npoint) < empty_frac
    F = rng.standard_normal((batch * n, c_in)).astype(np.float32)
    W = (rng.standard_normal((c_out, 3 + c_in)) / np.sqrt(3 + c_in)).astype(np.float32)
    return dict(F=F, W=W, xyz=xyz, ctr=ctr, idx=idx, empty=empty)
