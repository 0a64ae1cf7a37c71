"""Plain numpy restatement of the sparse-convolution contracts of include/spx.h §4 (no GPU, no library).

    gemm  : out[o]          = sum_k src[pair[k][o]] . W_kk          kk = K-1-k when flip_k, else k
            then  y = out * scale + shift (both optional), ReLU if asked
    wgrad : dw[co][k][ci]   = sum_{o < n_live} dout[o, co] * feat[pair[k][o], ci]

Weights are in the parameter layout w[Cout][K][Cin] (any [Cout, kz, ky, kx, Cin] is flattened), tables are [K][n] int32
with -1 = no pair.  Everything is accumulated in float64 — or in int64 when every input is integer-valued: with small
integers all products and partial sums stay below 2^24, float32 arithmetic is then exact in ANY summation order, and a
kernel has to reproduce the integer result bit for bit (abs_bound() gives the quantity to check that precondition with).

Table builders: subm_table / strided_table derive the tables from voxel coordinates through a Python dict (no hashing
tricks, no sorting tricks); random_table makes synthetic ones (the kernels only need pair[k][o] in [-1, n_src));
embed_table places a table in a wider and / or longer buffer.  Padding and dead entries are ALWAYS random indices inside
[-1, n_src), and callers poison dead feature rows with NaN: a kernel that reads what it must not read fails an assertion
instead of reading out of bounds.
"""
import itertools

import numpy as np


# ------------------------------------------------------------------------------------------ arithmetic

def _w3(w):
    w = np.asarray(w)
    return w.reshape(w.shape[0], -1, w.shape[-1])


def _integer_valued(*arrs):
    for a in arrs:
        if a is None:
            continue
        a = np.asarray(a, np.float64)
        a = a[np.isfinite(a)]                      # NaN marks dead rows; they are never gathered (asserted below)
        if a.size and not np.array_equal(a, np.rint(a)):
            return False
    return True


def _matmul(a, b, exact_int):
    """a @ b in float64.  exact_int: the operands are integers; the float64 product is then exact (asserted: length *
    max|a| * max|b|, a bound on every partial sum, is below 2^53) and is returned as int64, i.e. the int64 matmul without
    numpy's slow integer loop."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all(), "a live pair reads a dead (NaN) row: the TEST's table is wrong"
    c = a @ b
    if not exact_int:
        return c
    if a.size and b.size:
        assert a.shape[1] * float(np.abs(a).max()) * float(np.abs(b).max()) < 2.0 ** 53
    return np.rint(c).astype(np.int64)


def gemm(src, w, pair, flip_k=False, scale=None, shift=None, relu=False, n_live=None):
    """spx_conv_gemm.  src [n_src, c_src]; w [c_dst, K, c_src] (the forward call; for a data gradient pass the weight
    with its channel axes swapped, w.transpose(2, 1, 0) for a 3-D w); pair [K, n_dst].  Returns float64 [n_dst, c_dst];
    rows at or beyond n_live are NaN (the kernel does not write them)."""
    src = np.asarray(src)
    w = _w3(w)
    pair = np.asarray(pair)
    K, n = pair.shape
    assert w.shape[1] == K and w.shape[2] == src.shape[1]
    live = n if n_live is None else int(n_live)
    exact = _integer_valued(src, w)
    acc = np.zeros((live, w.shape[0]), np.int64 if exact else np.float64)
    for k in range(K):
        kk = K - 1 - k if flip_k else k
        ids = pair[k, :live]
        o = np.nonzero(ids >= 0)[0]
        if o.size:
            assert int(ids[o].max()) < src.shape[0]
            acc[o] += _matmul(src[ids[o]], w[:, kk, :].T, exact)
    y = acc.astype(np.float64)
    if scale is not None:
        y = y * np.asarray(scale, np.float64)
    if shift is not None:
        y = y + np.asarray(shift, np.float64)
    if relu:
        y = np.maximum(y, 0.0)
    out = np.full((n, w.shape[0]), np.nan)
    out[:live] = y
    return out


def wgrad(feat, dout, pair, wshape, n_live=None):
    """spx_conv_wgrad.  feat [n_src, cin]; dout [n_out, cout]; pair [K, n_out]; returns float64 of shape wshape
    ([cout, ..., cin])."""
    feat = np.asarray(feat)
    dout = np.asarray(dout)
    pair = np.asarray(pair)
    K, n = pair.shape
    cout, cin = int(wshape[0]), int(wshape[-1])
    assert int(np.prod(wshape[1:-1], dtype=np.int64)) == K and feat.shape[1] == cin and dout.shape[1] == cout
    live = n if n_live is None else int(n_live)
    exact = _integer_valued(feat, dout)
    dw = np.zeros((cout, K, cin), np.int64 if exact else np.float64)
    for k in range(K):
        ids = pair[k, :live]
        o = np.nonzero(ids >= 0)[0]
        if o.size:
            assert int(ids[o].max()) < feat.shape[0]
            dw[:, k, :] = _matmul(dout[o].T, feat[ids[o]], exact)
    return dw.astype(np.float64).reshape(tuple(wshape))


def abs_bound(op, *args, **kw):
    """Largest sum of |a||b| any output element of the case accumulates: abs_bound("gemm", src, w, pair, ...) or
    abs_bound("wgrad", feat, dout, pair, wshape, ...), same arguments as gemm / wgrad.  For a gemm with an epilogue the
    bound is taken after it (sum * max|scale| + max|shift|) and counted in units of the finest scale (0.5 doubles it), so
    that  abs_bound < 2**24  is the one precondition under which float32 evaluation in any order is exact."""
    if op == "wgrad":
        feat, dout, pair, wshape = args
        r = wgrad(np.abs(feat), np.abs(dout), pair, wshape, **kw)
        return float(r.max()) if r.size else 0.0
    assert op == "gemm"
    src, w, pair = args
    scale, shift = kw.pop("scale", None), kw.pop("shift", None)
    kw.pop("relu", None)
    live = pair.shape[1] if kw.get("n_live") is None else int(kw["n_live"])
    r = gemm(np.abs(src), np.abs(w), pair, **kw)[:live]
    b = float(r.max()) if r.size else 0.0
    unit = 1.0
    if scale is not None:
        s = np.abs(np.asarray(scale, np.float64))
        b *= float(s.max())
        while not np.array_equal(s / unit, np.rint(s / unit)):
            unit /= 2.0
            assert unit > 2.0 ** -30, "scale is not a dyadic rational"
    if shift is not None:
        b += float(np.abs(shift).max())
    return b / unit


# ------------------------------------------------------------------------------------------ tables from coordinates

def _offsets(ksize):
    return list(itertools.product(*(range(int(k)) for k in ksize)))          # k = (kz * KY + ky) * KX + kx


def out_shape_of(shape, ksize, stride, pad):
    return [(int(i) + 2 * int(p) - int(k)) // int(s) + 1 for i, k, s, p in zip(shape, ksize, stride, pad)]


def subm_table(coords, shape, ksize):
    """Submanifold convolution (outputs = inputs, stride 1, padding k // 2).  coords [n, 4] int (batch, z, y, x).
    Returns (forward table, backward table), each [K, n] int32: forward[k][o] = the row at coords[o] + offset_k - k // 2;
    the backward table is the forward one read at K-1-k (what flip_k does inside the kernel)."""
    coords = np.asarray(coords)
    where = {tuple(int(v) for v in c): i for i, c in enumerate(coords)}
    offs = _offsets(ksize)
    pair = np.full((len(offs), coords.shape[0]), -1, np.int32)
    for o, (b, z, y, x) in enumerate(coords):
        for k, (kz, ky, kx) in enumerate(offs):
            p = (int(z) + kz - ksize[0] // 2, int(y) + ky - ksize[1] // 2, int(x) + kx - ksize[2] // 2)
            if all(0 <= p[a] < shape[a] for a in range(3)):
                pair[k, o] = where.get((int(b),) + p, -1)
    return pair, pair[::-1].copy()


def strided_table(coords, shape, ksize, stride, pad):
    """Regular sparse convolution: output site q is active when some input p = q * stride - pad + offset_k exists.
    Returns (out_coords [m, 4] ascending in (batch, z, y, x), forward table [K, m], backward table [K, n], out_shape):
    forward[k][o] = the input row at out_coords[o] * stride - pad + offset_k, backward[k][i] = the output row o with
    forward[k][o] == i."""
    coords = np.asarray(coords)
    oshape = out_shape_of(shape, ksize, stride, pad)
    offs = _offsets(ksize)
    hits = {}                                                                  # (b, qz, qy, qx) -> [(k, input row)]
    for i, (b, z, y, x) in enumerate(coords):
        p = (int(z), int(y), int(x))
        for k, off in enumerate(offs):
            t = [p[a] + pad[a] - off[a] for a in range(3)]
            if any(t[a] % stride[a] for a in range(3)):
                continue
            q = tuple(t[a] // stride[a] for a in range(3))
            if all(0 <= q[a] < oshape[a] for a in range(3)):
                hits.setdefault((int(b),) + q, []).append((k, i))
    sites = sorted(hits)
    fwd = np.full((len(offs), len(sites)), -1, np.int32)
    bwd = np.full((len(offs), coords.shape[0]), -1, np.int32)
    for o, site in enumerate(sites):
        for k, i in hits[site]:
            assert fwd[k, o] == -1 and bwd[k, i] == -1
            fwd[k, o] = i
            bwd[k, i] = o
    return np.array(sites, np.int32).reshape(-1, 4), fwd, bwd, oshape


# ------------------------------------------------------------------------------------------ synthetic tables

def random_table(K, n_dst, n_src, density, rng, empty_offsets=(), rows=None):
    """[K, n_dst] int32: each entry is a pair with probability `density` (a uniformly random source row in [0, n_src)),
    else -1.  empty_offsets: table rows left without any pair.  rows = (lo, hi): pairs only in columns [lo, hi)."""
    pair = rng.integers(0, max(int(n_src), 1), size=(K, n_dst)).astype(np.int32)
    keep = rng.random((K, n_dst)) < density
    if n_src <= 0:
        keep[:] = False
    for k in empty_offsets:
        keep[k] = False
    if rows is not None:
        keep[:, :rows[0]] = False
        keep[:, rows[1]:] = False
    pair[~keep] = -1
    return pair


def embed_table(pair, n_src, rng, cap=None, ld=None):
    """The table as a kernel may meet it: columns [n, cap) are dead (the live count stays n) and the leading dimension is
    ld >= cap (default cap; the wide case of the tests is ld = n + 37).  Every entry outside the table proper is a random
    value in [-1, n_src) — in-range garbage, never an index that could be followed out of bounds."""
    K, n = pair.shape
    cap = n if cap is None else int(cap)
    ld = cap if ld is None else int(ld)
    assert n <= cap <= ld
    buf = rng.integers(-1, max(int(n_src), 1), size=(K, ld)).astype(np.int32)
    if n_src <= 0:
        buf[:] = -1
    buf[:, :n] = pair
    return buf
