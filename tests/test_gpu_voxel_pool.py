"""spx_voxel_pool_* (include/spx.h §27, csrc/voxel_pool.hip) on the device against the numpy restatement
(tests/voxel_pool_ref.py).

Exact cases: coordinates on a half-integer lattice and f, A, b, dout in small integers make every value and every sum an
integer multiple of 0.5 below 2^24, so float32 holds them exactly whatever the summation order (asserted per case); out,
arg, df, dA, db and the moments must then equal the int64 restatement bit for bit.

Float cases, per output tensor: e_fused = max |op - float64| <= point_loss_ref.measured_bound(e_eager, float64), i.e.
4 x the error of the float32 torch composition on the same device with a floor of 1e-6 of the tensor's largest magnitude.
The gradients' float64 values replay the op's own arg, so a near-tie cannot become a gradient mismatch; arg itself must
agree with float64 wherever float64 decides clearly (voxel_pool_ref.decided_pairs).  The measured errors are printed and
appended to profiles/voxel_pool_accuracy.log."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import point_loss_ref as plr
import voxel_pool_ref as vpr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "voxel_pool_accuracy.log")
EXACT = float(1 << 24)


def _g(a, dtype=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if dtype is None else a.astype(dtype)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------------------------------------- exact cases
#        name            M     C   S   n_src  kind
CASES = (("one",          1,    1,  1,   1,   "none_empty"),
         ("odd",          63,   33, 17,  300, "mixed"),
         ("two_blocks",   257,  32, 16,  300, "mixed"),
         ("large",        2049, 64, 16,  300, "mixed"),
         ("one_slot",     2049, 96, 1,   300, "none_empty"),
         ("one_source",   257,  1,  17,  1,   "mixed"),
         ("all_empty",    63,   64, 16,  300, "all_empty"),
         ("one_row",      2049, 32, 16,  300, "one_row"),
         ("negative",     257,  33, 16,  300, "negative"),
         ("ties",         257,  32, 16,  300, "ties"),
         ("nan_unread",   257,  32, 16,  300, "nan"))


@functools.lru_cache(maxsize=None)
def _exact_case(name):
    """Integer data (coordinates doubled) and the int64 restatement, computed once and shared (never written to)."""
    _, m, c, s, n_src, kind = [k for k in CASES if k[0] == name][0]
    rng = np.random.default_rng(sum(map(ord, name)))
    live_rows = 150 if kind == "nan" else n_src
    idx, empty = vpr.random_lists(rng, m, s, live_rows, p_empty=0.0 if kind in ("none_empty", "one_row") else 0.2)
    if kind == "all_empty":
        empty[:] = True
        idx[:] = 0
    if kind == "one_row":
        idx[:] = 7
    lim = 8 if kind == "negative" else 40
    xyz2 = rng.integers(-lim, lim + 1, size=(n_src, 3))
    new2 = rng.integers(-lim, lim + 1, size=(m, 3))
    f = rng.integers(-8, 9, size=(n_src, c))
    a = rng.integers(-3, 4, size=(c, 3))
    b = rng.integers(-4, 5, size=(c,))
    dout = rng.integers(-5, 6, size=(m, c))
    if kind == "negative":                           # |A . d| <= 3 * 3 * 16 = 144 < 200
        f = -200 - np.abs(f)
        b = -1 - np.abs(b)
    if kind == "ties":                               # rows 2 k and 2 k + 1 are twins: distinct rows, equal values
        xyz2[1::2] = xyz2[0::2]
        f[1::2] = f[0::2]
    out2, arg = vpr.max_fwd(2 * f, xyz2, new2, idx, empty, a, 2 * b, dtype=np.int64)
    df, da2, db = vpr.max_bwd(dout, arg, idx, empty, xyz2, new2, n_src, dtype=np.int64)
    mom = vpr.moments(xyz2, new2, idx, empty, dtype=np.int64)
    # exactness in float32: every value and every partial sum is a multiple of 0.5 whose double stays below 2^24
    v2 = vpr.values(2 * f, xyz2, new2, idx, empty, a, 2 * b, dtype=np.int64)
    d2 = np.abs(vpr.offsets(xyz2, new2, idx, empty, np.int64)).max() if m else 0
    assert 2 * np.abs(v2).max() < EXACT and 2 * (np.abs(a).sum(axis=1).max() * d2 + 2 * np.abs(b).max()) < EXACT
    assert 2 * np.abs(dout).sum(axis=0).max() * max(int(d2), 1) < EXACT
    return dict(m=m, c=c, s=s, n_src=n_src, kind=kind, idx=idx, empty=empty, xyz2=xyz2, new2=new2, f=f, a=a, b=b,
                dout=dout, out2=out2, arg=arg, df=df, da2=da2, db=db, mom=mom)


def _device_inputs(case):
    """float32 device copies; for the nan case, NaN in every source row no live list reaches and garbage (in-range) lists
    in the empty queries."""
    xyz, f, idx = case["xyz2"] / 2.0, case["f"].astype(np.float64), case["idx"].copy()
    if case["kind"] == "nan":
        xyz, f = xyz.copy(), f.copy()
        xyz[150:] = np.nan
        f[150:] = np.nan
        rng = np.random.default_rng(1)
        idx[case["empty"]] = rng.integers(150, case["n_src"], size=(int(case["empty"].sum()), case["s"]))
        assert case["empty"].any()
    return dict(f=_g(f, np.float32), xyz=_g(xyz, np.float32), new_xyz=_g(case["new2"] / 2.0, np.float32),
                idx=_g(idx, np.int32), empty=_g(case["empty"], np.uint8), a=_g(case["a"], np.float32),
                b=_g(case["b"], np.float32), dout=_g(case["dout"], np.float32))


def _raw_run(case, t):
    """The three entry points through the C ABI on buffers pre-filled with NaN / a sentinel."""
    from spx import _lib, ops
    lib = _lib.load()
    m, c, s, n_src = case["m"], case["c"], case["s"], case["n_src"]
    out = torch.full((m, c), float("nan"), device=DEV)
    arg = torch.full((m, c), -77, dtype=torch.int32, device=DEV)
    df = torch.full((n_src, c), float("nan"), device=DEV)
    da = torch.full((c, 3), float("nan"), device=DEV)
    db = torch.full((c,), float("nan"), device=DEV)
    mom = torch.full((9,), float("nan"), dtype=torch.float64, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wsb = max(lib.spx_voxel_pool_moments_ws_bytes(m, s), lib.spx_voxel_pool_max_bwd_ws_bytes(c, n_src, m, s))
    ws = ops.workspace(DEV, wsb)
    assert lib.spx_voxel_pool_moments(_p(t["xyz"]), _p(t["new_xyz"]), _p(t["idx"]), _p(t["empty"]), n_src, m, s, _p(mom),
                                      _p(ws), wsb, stream) == 0
    assert lib.spx_voxel_pool_max_fwd(_p(t["f"]), _p(t["xyz"]), _p(t["new_xyz"]), _p(t["idx"]), _p(t["empty"]), _p(t["a"]),
                                      _p(t["b"]), c, n_src, m, s, _p(out), _p(arg), stream) == 0
    assert lib.spx_voxel_pool_max_bwd(_p(t["dout"]), _p(arg), _p(t["idx"]), _p(t["empty"]), _p(t["xyz"]), _p(t["new_xyz"]),
                                      c, n_src, m, s, _p(df), _p(da), _p(db), _p(ws), wsb, stream) == 0
    torch.cuda.synchronize()
    return dict(out=_n(out), arg=_n(arg), df=_n(df), da=_n(da), db=_n(db), mom=_n(mom))


@pytest.mark.parametrize("name", [k[0] for k in CASES])
def test_exact_cases_bit_for_bit(name):
    case = _exact_case(name)
    got = _raw_run(case, _device_inputs(case))
    assert np.array_equal(got["arg"], case["arg"])
    assert np.array_equal(got["out"].astype(np.float64) * 2, case["out2"])
    assert np.array_equal(got["df"].astype(np.float64), case["df"])
    assert np.array_equal(got["da"].astype(np.float64) * 2, case["da2"])
    assert np.array_equal(got["db"].astype(np.float64), case["db"])
    assert np.array_equal(got["mom"][:3] * 2, case["mom"][:3]) and np.array_equal(got["mom"][3:] * 4, case["mom"][3:])
    kind = case["kind"]
    pointed = np.zeros(case["n_src"], dtype=bool)
    pointed[np.unique(case["idx"][~case["empty"]])] = True
    assert not got["df"][~pointed].any()                       # rows nothing points at: written, and zero
    if kind in ("all_empty", "negative"):
        assert not got["df"].any()
    if kind == "negative":
        assert not got["out"].any() and (got["arg"] == -1).all() and not got["da"].any() and not got["db"].any()
    if kind == "all_empty":
        assert np.array_equal(got["out"], np.broadcast_to(np.maximum(case["b"], 0), got["out"].shape))
        assert not got["mom"].any() and not got["da"].any()
    if kind == "one_row":
        assert not np.delete(got["df"], 7, axis=0).any() and got["df"][7].any()
    if kind == "ties":                                         # some winner has a twin later in its list
        idx, arg = case["idx"], case["arg"]
        mm, cc = np.nonzero((arg >= 0) & ~case["empty"][:, None])
        win = idx[mm, arg[mm, cc]]
        assert ((idx[mm] == (win ^ 1)[:, None]) & (np.arange(case["s"])[None, :] > arg[mm, cc][:, None])).any()


# --------------------------------------------------------------------------------------------------------- float cases
@functools.lru_cache(maxsize=None)
def _float_gold(c, seed):
    case = vpr.float_case(c, seed)
    out, arg = vpr.max_fwd(case["f"], case["xyz"], case["new_xyz"], case["idx"], case["empty"], case["a"], case["b"])
    return case, out, arg, vpr.decided_pairs(case)


def _eager(t):
    """The float32 torch composition with the same affine map: gather, mask, offsets, add, ReLU, max."""
    f = t["f"].clone().requires_grad_(True)
    a = t["a"].clone().requires_grad_(True)
    b = t["b"].clone().requires_grad_(True)
    rows, empty = t["idx"].long(), t["empty"].bool()[:, None, None]
    d = (t["xyz"][rows] - t["new_xyz"][:, None, :]).masked_fill(empty, 0)
    v = f[rows].masked_fill(empty, 0) + (d @ a.t() + b)
    out = torch.relu(v).max(dim=1).values
    out.backward(t["dout"])
    return out.detach(), f.grad, a.grad, b.grad


@pytest.mark.parametrize("c,seed", vpr.FLOAT_CASES)
def test_float_accuracy_against_float64(c, seed):
    from spx import ops
    case, out64, arg64, decided = _float_gold(c, seed)
    t = {k: _g(v, np.uint8 if k == "empty" else None) for k, v in case.items()}
    f = t["f"].clone().requires_grad_(True)
    a = t["a"].clone().requires_grad_(True)
    b = t["b"].clone().requires_grad_(True)
    out, arg = ops.voxel_pool_max(f, t["xyz"], t["new_xyz"], t["idx"], t["empty"], a, b, return_arg=True)
    out.backward(t["dout"])
    mom = ops.voxel_pool_moments(t["xyz"], t["new_xyz"], t["idx"], t["empty"])
    e_out, e_df, e_da, e_db = _eager(t)
    arg_op = _n(arg)
    # the gradients' float64 values replay the op's winners and its out > 0 mask
    df64, da64, db64 = vpr.max_bwd(case["dout"], arg_op, case["idx"], case["empty"], case["xyz"], case["new_xyz"],
                                   case["f"].shape[0])
    rows = (("out", out, e_out, out64), ("df", f.grad, e_df, df64), ("dA", a.grad, e_da, da64), ("db", b.grad, e_db, db64))
    lines, checks = [], []
    for name, fused, eager, gold in rows:
        e_f = float(np.abs(_n(fused).astype(np.float64) - gold).max())
        e_e = float(np.abs(_n(eager).astype(np.float64) - gold).max())
        bound = plr.measured_bound(e_e, gold)
        lines.append("C %-3d %-4s e_fused %.3e  e_eager %.3e  bound %.3e  max|f64| %.3e" % (c, name, e_f, e_e, bound,
                                                                                          float(np.abs(gold).max())))
        checks.append((name, e_f, bound))
    agree = arg_op == arg64
    lines.append("C %-3d arg  undecided pairs %.4f %%  disagreeing decided pairs %d" % (
        c, 100.0 * (1.0 - decided.mean()), int((~agree & decided).sum())))
    d = vpr.offsets(case["xyz"], case["new_xyz"], case["idx"], case["empty"], np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    mom64 = vpr.moments(case["xyz"], case["new_xyz"], case["idx"], case["empty"])
    mom_abs = np.array([np.abs(q).sum() for q in (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)])
    rel = np.abs(_n(mom) - mom64) / mom_abs
    lines.append("C %-3d moments  max |op - f64| / sum |terms| %.3e" % (c, float(rel.max())))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    for name, e_f, bound in checks:
        assert e_f <= bound, (name, e_f, bound)
    assert agree[decided].all()
    assert 1.0 - decided.mean() <= 0.01
    assert float(rel.max()) <= 1e-12


# --------------------------------------------------------------------------------------------- reproducibility, capture
def _step(t, f, dout):
    from spx import ops
    mom = ops.voxel_pool_moments(t["xyz"], t["new_xyz"], t["idx"], t["empty"])
    out, arg = ops.voxel_pool_max_fwd(f, t["xyz"], t["new_xyz"], t["idx"], t["empty"], t["a"], t["b"])
    df, da, db = ops.voxel_pool_max_bwd(dout, arg, t["xyz"], t["new_xyz"], t["idx"], t["empty"], f.shape[0])
    return mom, out, arg, df, da, db


def test_two_runs_are_bit_equal():
    from spx import ops
    case = _float_gold(*vpr.FLOAT_CASES[0])[0]
    t = {k: _g(v, np.uint8 if k == "empty" else None) for k, v in case.items()}
    runs = []
    for _ in range(2):
        f = t["f"].clone().requires_grad_(True)
        a = t["a"].clone().requires_grad_(True)
        b = t["b"].clone().requires_grad_(True)
        out = ops.voxel_pool_max(f, t["xyz"], t["new_xyz"], t["idx"], t["empty"], a, b)
        out.backward(t["dout"])
        runs.append((out.detach(), f.grad, a.grad, b.grad, ops.voxel_pool_moments(t["xyz"], t["new_xyz"], t["idx"], t["empty"])))
        ops.workspace(DEV, 1).fill_(0xA5)                      # the next run may not depend on what the last one left
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_forward_and_backward_capture_and_replay():
    case = _float_gold(*vpr.FLOAT_CASES[0])[0]
    t = {k: _g(v, np.uint8 if k == "empty" else None) for k, v in case.items()}
    f, dout = t["f"].clone(), t["dout"].clone()
    _step(t, f, dout)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(t, f, dout)                                      # warm the workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = _step(t, f, dout)
    f.copy_(torch.roll(t["f"], 3, dims=0) * 1.5)               # other values through the static buffers
    dout.copy_(torch.roll(t["dout"], 5, dims=0) - 0.25)
    g.replay()
    torch.cuda.synchronize()
    eager = _step(t, f, dout)
    for x, y in zip(static, eager):
        assert torch.equal(x, y)
