"""spx_conv_gemm, spx_conv_gemm_balanced and spx_conv_wgrad against tests/sparse_conv_ref.py at the sizes where their
work splits, kernel choices and index arithmetic change (tests/test_sparse_conv_ref.py pins the reference itself to dense
float64 convolutions).

Integer data: features / gradients / weights drawn from {-2..2}, scales from {0.5, 1, 2, 4}, integer shifts.  Every
product and partial sum is then an integer (or a half) far below 2^24 — asserted per case on the CPU with abs_bound() —
so float32 MFMA / FMA arithmetic is exact in ANY summation order and the kernels must equal the int64 reference bit for
bit, whatever split, plan, live count or schedule they pick.  Float data is compared at the two bars of
test_gpu_kernels.py: 2e-5 (gemm) and 1e-4 (wgrad) times max(1, max|ref|).

Tables are synthetic (the kernels only need pair[k][o] in [-1, n_src)); padding columns and dead tails hold random
in-range indices and dead feature rows NaN, so a kernel that reads what it must not fails an assertion here.
"""
import numpy as np
import pytest
import torch

import sparse_conv_ref as R

pytestmark = pytest.mark.gpu

TOL_GEMM = 2e-5       # test_gpu_kernels.py: TOL
TOL_WGRAD = 1e-4      # test_gpu_kernels.py: test_conv_fwd_dgrad_wgrad_vs_oracle
EXACT = 2 ** 24
KVOLS = (1, 3, 9, 25, 27, 32)


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _ints(rng, *shape):
    return rng.integers(-2, 3, shape).astype(np.float32)


def _dn(live):
    return torch.tensor([int(live)], dtype=torch.int64, device=_dev())


def _equal(got, ref, what):
    """Bit equality with the integer reference (float32 -> float64 is exact)."""
    got = got.detach().cpu().double().reshape(-1)
    ref = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64)).reshape(-1)
    if not torch.equal(got, ref):
        bad = torch.nonzero(~(got == ref)).reshape(-1)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at flat index %d: got %r, want %r"
                             % (what, bad.numel(), ref.numel(), i, float(got[i]), float(ref[i])))


def _each(values, case):
    """case(v) for EVERY v, then one assertion naming all that failed (a loop that stops at its first failure hides which
    sizes are affected)."""
    failed = []
    for v in values:
        try:
            case(v)
        except AssertionError as e:
            failed.append(str(e).splitlines()[0])
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(values), "\n".join(failed))


def _close(got, ref, tol, what):
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= tol * scale, "%s: max|err| %.3e > %.1e * %.3g" % (what, err, tol, scale)


# ------------------------------------------------------------------------------------------ weight gradient

def _wgrad_case(pair, n_src, cin, cout, rng, cap=None, ld=None, src_live=None, d_n=None, counts=False, data=_ints,
                what=""):
    """One spx_conv_wgrad call on `pair` [K, live] embedded in a [K, ld] buffer with `cap` columns of capacity; rows of
    feat at or beyond src_live and rows of dout at or beyond live are NaN.  Returns (dw, reference, the call's arguments)."""
    from spx import ops
    K, live = pair.shape
    cap = live if cap is None else cap
    src_live = n_src if src_live is None else src_live
    buf = R.embed_table(pair, n_src, rng, cap=cap, ld=ld)
    feat, dout = data(rng, n_src, cin), data(rng, cap, cout)
    feat[src_live:] = np.nan
    dout[live:] = np.nan
    wshape = (cout, K, cin)
    ref = R.wgrad(feat, dout, buf[:, :cap], wshape, n_live=live)
    if data is _ints:
        assert R.abs_bound("wgrad", feat, dout, buf[:, :cap], wshape, n_live=live) < EXACT
    if cap > live and d_n is None:
        d_n = _dn(live)
    args = (_t(feat), _t(dout), _t(buf), buf.shape[1], cap, wshape)
    cnt = ops.wgrad_counts(args[2], buf.shape[1], K, cap, d_n) if counts else None
    dw = ops.conv_wgrad(*args, d_n_out=d_n, counts=cnt)
    if data is _ints:
        _equal(dw, ref, "wgrad %s K=%d live=%d cap=%d ld=%d %dx%d" % (what, K, live, cap, buf.shape[1], cin, cout))
    return dw, ref, (args, d_n)


# 4 = pairs per MFMA step, 64 = rows per count group, 256 = rows per batch, 512 = eight eighths of one group each, 513 =
# eighths 5-7 empty and eighth 4 one ragged group, 2304 = first n with more blocks than offsets per XCD
WGRAD_ROWS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2303, 2304, 2305, 5000)


@pytest.mark.parametrize("cin,cout,rows", [(16, 16, WGRAD_ROWS), (64, 64, (1, 5, 64, 65, 256, 257, 512, 513, 2304, 2305))])
def test_wgrad_int_row_counts(cin, cout, rows):
    rng = np.random.default_rng(1000 + cin)
    _each(rows, lambda n: _wgrad_case(R.random_table(27, n, n, 0.3, rng), n, cin, cout, rng, what="rows"))


@pytest.mark.parametrize("n", [513, 5000])
def test_wgrad_int_table_shapes(n):
    rng = np.random.default_rng(2000 + n)
    K = 27
    _, ref, _ = _wgrad_case(R.random_table(K, n, n, 0.3, rng, empty_offsets=(13,)), n, 16, 16, rng, what="empty offset")
    assert not ref[:, 13, :].any() and ref[:, 12, :].any()
    dw, ref, _ = _wgrad_case(R.random_table(K, n, n, 0.0, rng), n, 16, 16, rng, what="no pair")
    assert not ref.any() and int(torch.count_nonzero(dw)) == 0
    _wgrad_case(R.random_table(K, n, n, 0.3, rng, rows=(0, 64)), n, 16, 16, rng, what="first 64 rows")
    _wgrad_case(R.random_table(K, n, n, 0.3, rng, rows=(n - 64, n)), n, 16, 16, rng, what="last 64 rows")
    dense = R.random_table(K, n, n, 1.0, rng)
    assert (dense >= 0).all()
    _wgrad_case(dense, n, 16, 16, rng, what="dense")


def test_wgrad_int_pair_carry():
    """K = 1, n = 16, exactly 1..9 pairs: a final partial step of 1-3 pairs after zero, one and two full steps."""
    rng = np.random.default_rng(3000)

    def case(npairs):
        pair = np.full((1, 16), -1, np.int32)
        cols = rng.choice(16, npairs, replace=False)
        pair[0, cols] = rng.integers(0, 16, npairs)
        assert int((pair >= 0).sum()) == npairs
        _, ref, _ = _wgrad_case(pair, 16, 16, 16, rng, what="%d pairs" % npairs)
        assert ref.any()

    _each(range(1, 10), case)


def test_wgrad_int_kernel_volumes():
    from spx import _lib, ops
    rng = np.random.default_rng(4000)
    n = 1000
    for K in KVOLS:
        _wgrad_case(R.random_table(K, n, n, 0.3, rng), n, 16, 16, rng, what="kvol")
    pair = _t(R.random_table(33, n, n, 0.3, rng))
    with pytest.raises(_lib.SpxError, match=r"invalid argument.*\(code -1\)"):
        ops.conv_wgrad(_t(_ints(rng, n, 16)), _t(_ints(rng, n, 16)), pair, n, n, (16, 33, 16))


WGRAD_EXACT = [(16, 128), (128, 16), (32, 64), (128, 128)]
WGRAD_RAGGED = [(1, 1), (4, 16), (5, 16), (7, 9), (24, 48), (48, 24), (80, 96), (96, 80), (100, 36), (128, 127)]


@pytest.mark.parametrize("cin,cout", WGRAD_EXACT + WGRAD_RAGGED)
def test_wgrad_int_channel_pairs(cin, cout):
    rng = np.random.default_rng(5000 + 131 * cin + cout)
    n = 1000
    for K in (3, 27):
        _wgrad_case(R.random_table(K, n, n, 0.3, rng), n, cin, cout, rng, what="channels")


def test_wgrad_int_source_rows_and_wide_table():
    rng = np.random.default_rng(6000)
    n, K = 1000, 27
    for n_src in (3 * n, n // 3):
        _wgrad_case(R.random_table(K, n, n_src, 0.3, rng), n_src, 16, 16, rng, what="n_src=%d" % n_src)
    for n in (513, 1000):
        _wgrad_case(R.random_table(K, n, n, 0.3, rng), n, 16, 16, rng, ld=n + 37, what="wide")


@pytest.mark.parametrize("cap", [513, 5000])
def test_wgrad_int_live_count(cap):
    """d_n_out below the capacity: the dead tail of the table is in-range garbage, dead rows of feat and dout are NaN."""
    rng = np.random.default_rng(7000 + cap)
    for live in (0, 1, 64, 500, cap - 1, cap):
        pair = R.random_table(27, live, live, 0.3, rng)
        dw, ref, _ = _wgrad_case(pair, cap, 16, 16, rng, cap=cap, src_live=live, d_n=_dn(live), what="live")
        if live == 0:
            assert int(torch.count_nonzero(dw)) == 0 and not bool(torch.isnan(dw).any())
    # the same with the table in a wider buffer
    _wgrad_case(R.random_table(27, 500, 500, 0.3, rng), cap, 16, 16, rng, cap=cap, ld=cap + 37, src_live=500, what="live+wide")


@pytest.mark.parametrize("with_dn", [False, True])
def test_wgrad_counts_passed_in(with_dn):
    """counts = ops.wgrad_counts(...) is the same computation as counts = None, bit for bit, and repeatable."""
    from spx import ops
    rng = np.random.default_rng(8000)
    for cap, cin, cout, data in ((513, 16, 16, _ints), (5000, 16, 16, _ints), (5000, 64, 64, _floats)):
        live = cap - 77 if with_dn else cap
        pair = R.random_table(27, live, live, 0.3, rng)
        dw, ref, (args, d_n) = _wgrad_case(pair, cap, cin, cout, rng, cap=cap, src_live=live, counts=True, data=data)
        assert (d_n is not None) == with_dn
        pair_t, ld = args[2], args[3]
        cnt = ops.wgrad_counts(pair_t, ld, 27, cap, d_n)
        for counts in (None, cnt, None, cnt):
            assert torch.equal(dw, ops.conv_wgrad(*args, d_n_out=d_n, counts=counts))
        _close(dw, ref, TOL_WGRAD, "counts")


def test_wgrad_int_preshifted_split():
    """A dense K = 27 table of 160 000 rows: each row-eighth holds 540 000 >= 2^19 pairs, the smallest case in which the
    proportional split works on pre-shifted counts."""
    rng = np.random.default_rng(9000)
    n = 160000
    pair = R.random_table(27, n, n, 1.0, rng)
    assert (n + 7) // 8 * 27 >= 2 ** 19
    _wgrad_case(pair, n, 16, 16, rng, what="pre-shifted")


def _floats(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _abs_floats(rng, *shape):
    return np.abs(rng.standard_normal(shape)).astype(np.float32)          # the sign pattern after a ReLU


@pytest.mark.parametrize("cin,cout", [(64, 64), (80, 96)])
@pytest.mark.parametrize("n", [513, 5000])
def test_wgrad_float(n, cin, cout):
    rng = np.random.default_rng(10000 + n + cin)
    for K in (3, 27, 32):
        for data in (_floats, _abs_floats):
            dw, ref, _ = _wgrad_case(R.random_table(K, n, n, 0.3, rng), n, cin, cout, rng, data=data)
            _close(dw, ref, TOL_WGRAD, "wgrad float K=%d n=%d %s" % (K, n, data.__name__))


# ------------------------------------------------------------------------------------------ gemm

def _w_dgrad(w):
    return np.ascontiguousarray(w.transpose(2, 1, 0))


def _gemm_case(src, w, buf, n_dst, flip=False, live=None, scale=None, shift=None, relu=False, plan_fn=None, what="",
               tol=None):
    """One spx_conv_gemm (or, with plan_fn, spx_conv_gemm_balanced) call: src [n_src, cs], w [cd, K, cs], table buf
    [K, ld] with n_dst columns of capacity.  Integer data: bit equality (tol None); float data: tol * max(1, max|ref|)."""
    from spx import ops
    cd, K, cs = w.shape
    ref = R.gemm(src, w, buf[:, :n_dst], flip_k=flip, scale=scale, shift=shift, relu=relu, n_live=live)
    if tol is None:
        assert R.abs_bound("gemm", src, w, buf[:, :n_dst], flip_k=flip, scale=scale, shift=shift, n_live=live) < EXACT
    d_n = None if live is None else _dn(live)
    kw = dict(flip_k=flip, d_n_dst=d_n, relu=relu,
              scale=None if scale is None else _t(np.asarray(scale, np.float32)),
              shift=None if shift is None else _t(np.asarray(shift, np.float32)))
    wp = ops.pack_weight(_t(w), 0)
    pair_t = _t(buf)
    if plan_fn is None:
        out = ops.conv_gemm(_t(src), wp, cd, K, pair_t, buf.shape[1], n_dst, **kw)
    else:
        plan = ops.conv_plan(pair_t, buf.shape[1], K, n_dst, d_n)
        out = ops.conv_gemm_balanced(_t(src), wp, cd, K, pair_t, buf.shape[1], n_dst, plan, **kw)
    nl = n_dst if live is None else live
    what = "gemm %s K=%d n=%d live=%d ld=%d %dx%d flip=%d" % (what, K, n_dst, nl, buf.shape[1], cs, cd, flip)
    if tol is None:
        _equal(out[:nl], ref[:nl], what)
    else:
        _close(out[:nl], ref[:nl], tol, what)
    return out, ref


GEMM_SM = [(16, 16), (32, 64)]                                # k_conv_mfma_sm
GEMM_MFMA = [(64, 64), (128, 128), (16, 128), (128, 16)]      # k_conv_mfma
GEMM_ROWS = [(4, 16), (8, 32), (5, 16)]                       # k_conv_valu_rows
GEMM_VALU = [(7, 9), (48, 24), (4, 64), (16, 8)]              # k_conv_valu
GEMM_N = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
ONE_PER_KERNEL = [(16, 16), (64, 64), (5, 16), (7, 9)]


@pytest.mark.parametrize("cs,cd", GEMM_SM + GEMM_MFMA + GEMM_ROWS + GEMM_VALU)
def test_gemm_int_sizes_volumes_flip(cs, cd):
    """Every n x K x flip_k on arbitrary tables (n_src != n_dst): the offset walk and the flipped weight index."""
    rng = np.random.default_rng(11000 + 131 * cs + cd)
    for n in GEMM_N:
        n_src = n + 3
        src = _ints(rng, n_src, cs)
        for K in KVOLS:
            w = _ints(rng, cd, K, cs)
            pair = R.random_table(K, n, n_src, 0.3, rng)
            for flip in (False, True):
                _gemm_case(src, w, pair, n, flip=flip, what="random")


@pytest.mark.parametrize("cs,cd", ONE_PER_KERNEL)
def test_gemm_int_coordinate_tables(cs, cd):
    """Tables built from voxel coordinates: the data gradient of a submanifold conv through flip_k on the (symmetric)
    forward table equals the one through the backward table; a strided conv forward and through its backward table."""
    rng = np.random.default_rng(12000 + cs)
    batch, shape = 2, (8, 9, 7)
    lin = np.sort(rng.choice(batch * int(np.prod(shape)), 300, replace=False))
    coords = np.stack(np.unravel_index(lin, (batch,) + shape), 1).astype(np.int32)
    n = coords.shape[0]
    for ksize in ((3, 3, 3), (3, 1, 1), (1, 3, 3), (1, 1, 1), (1, 5, 5)):
        fwd, bwd = R.subm_table(coords, shape, ksize)
        K = fwd.shape[0]
        w = _ints(rng, cd, K, cs)
        _gemm_case(_ints(rng, n, cs), w, fwd, n, what="subm fwd")
        dout = _ints(rng, n, cd)
        a, ref_a = _gemm_case(dout, _w_dgrad(w), fwd, n, flip=True, what="subm dgrad flip")
        b, ref_b = _gemm_case(dout, _w_dgrad(w), bwd, n, what="subm dgrad bwd table")
        assert torch.equal(a, b) and np.array_equal(ref_a, ref_b)
    for ksize, stride, pad in (((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0))):
        oc, fwd, bwd, _ = R.strided_table(coords, shape, ksize, stride, pad)
        m, K = oc.shape[0], fwd.shape[0]
        w = _ints(rng, cd, K, cs)
        _gemm_case(_ints(rng, n, cs), w, fwd, m, what="strided fwd")
        _gemm_case(_ints(rng, m, cd), _w_dgrad(w), bwd, n, what="strided dgrad")


@pytest.mark.parametrize("cs,cd", ONE_PER_KERNEL)
def test_gemm_int_epilogue(cs, cd):
    """y = acc * scale + shift, ReLU: rows without a pair give exactly relu(shift), and so does a table of -1 only."""
    rng = np.random.default_rng(13000 + cs)
    n = 257
    for K in (3, 27):
        src, w = _ints(rng, n, cs), _ints(rng, cd, K, cs)
        scale = rng.choice([0.5, 1.0, 2.0, 4.0], cd).astype(np.float32)
        shift = rng.integers(-3, 4, cd).astype(np.float32)
        shift[0], shift[-1] = -2.0, 3.0
        pair = R.random_table(K, n, n, 0.3, rng)
        pair[:, 100:140] = -1
        pair[:, n - 1] = -1
        for sc, sh, relu in ((scale, shift, True), (scale, shift, False), (scale, None, False), (None, shift, True)):
            out, _ = _gemm_case(src, w, pair, n, scale=sc, shift=sh, relu=relu, what="epilogue")
            rest = np.zeros(cd, np.float32) if sh is None else (np.maximum(sh, 0) if relu else sh)
            want = torch.from_numpy(rest).to(out.device)
            assert torch.equal(out[100:140], want.expand(40, cd)) and torch.equal(out[n - 1], want)
        none = np.full((K, n), -1, np.int32)
        out, _ = _gemm_case(src, w, none, n, scale=scale, shift=shift, relu=True, what="all -1")
        assert torch.equal(out, torch.from_numpy(np.maximum(shift, 0)).to(out.device).expand(n, cd))
        out, _ = _gemm_case(src, w, none, n, what="all -1, no epilogue")
        assert int(torch.count_nonzero(out)) == 0


@pytest.mark.parametrize("cs,cd", ONE_PER_KERNEL + [(128, 128)])
def test_gemm_int_wide_table_and_live_count(cs, cd):
    """pair_ld > n_dst, and d_n_dst below n_dst: rows below the live count equal the reference (dead table columns are
    in-range garbage, dead source rows NaN); rows at or beyond it are not asserted."""
    rng = np.random.default_rng(14000 + cs)
    K = 27
    for n in (65, 300):
        src, w = _ints(rng, n + 5, cs), _ints(rng, cd, K, cs)
        pair = R.random_table(K, n, n + 5, 0.3, rng)
        for flip in (False, True):
            _gemm_case(src, w, R.embed_table(pair, n + 5, rng, ld=n + 37), n, flip=flip, what="wide")
    cap = 300
    for live in (1, 17, 64, 255, cap - 1, cap):
        src = _ints(rng, cap, cs)
        src[live:] = np.nan
        pair = R.random_table(K, live, live, 0.3, rng)
        for ld in (cap, cap + 37):
            buf = R.embed_table(pair, cap, rng, cap=cap, ld=ld)
            for flip in (False, True):
                _gemm_case(src, w, buf, cap, flip=flip, live=live, what="live")
    sc, sh = np.full(cd, 2.0, np.float32), np.full(cd, 1.0, np.float32)
    _gemm_case(src, w, buf, cap, live=cap, scale=sc, shift=sh, relu=True, what="live + epilogue")


def test_gemm_refuses_kernel_volume_33():
    from spx import _lib, ops
    rng = np.random.default_rng(15000)
    n = 64
    pair = _t(R.random_table(33, n, n, 0.3, rng))
    wp = torch.zeros(33 * 16 * 16, device=_dev())
    with pytest.raises(_lib.SpxError, match=r"invalid argument.*\(code -1\)"):
        ops.conv_gemm(_t(_ints(rng, n, 16)), wp, 16, 33, pair, n, n)


@pytest.mark.parametrize("cs,cd", [(64, 64), (128, 128)])
def test_gemm_balanced_int_volumes(cs, cd):
    """spx_conv_gemm_balanced at K != 27 (spx_conv_gemm_ring is tied to spx_conv_gemm bit for bit at these volumes by
    test_gpu_ring.py, so this pins it as well)."""
    from spx import ops
    rng = np.random.default_rng(16000 + cs)
    n = 5000
    src = _ints(rng, n, cs)
    for K in (1, 3, 9, 25):
        w = _ints(rng, cd, K, cs)
        pair = R.random_table(K, n, n, 0.3, rng)
        for flip in (False, True):
            _gemm_case(src, w, pair, n, flip=flip, plan_fn=ops.conv_plan, what="balanced")


@pytest.mark.parametrize("cs,cd", [(64, 64), (7, 9)])
def test_gemm_float(cs, cd):
    rng = np.random.default_rng(17000 + cs)
    n = 1000
    src = _floats(rng, n, cs)
    for K in (1, 3, 9, 25, 32):
        w = _floats(rng, cd, K, cs)
        pair = R.random_table(K, n, n, 0.3, rng)
        for flip in (False, True):
            _gemm_case(src, w, pair, n, flip=flip, tol=TOL_GEMM, what="float")
