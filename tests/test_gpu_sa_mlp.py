"""spx_sa_mlp2_max (include/spx.h §28, csrc/sa_mlp.hip) on the device against the float64 restatement
(tests/sa_mlp_ref.py).

Exact cases: small-integer data make every product and every partial sum an integer below 2^24 (asserted per case from
absolute values), so float32 holds them whatever the order of summation and the op must equal the restatement bit for
bit.  They pin the MFMA operand maps (all-distinct W2 with C1 != C2), the accumulator row map and the cross-lane max (the
winner of channel o in row o % S), the empty-ball rule, and lists that repeat the first hit, point at row N - 1 or lie
outside [0, N).

Float cases: per case, max |op - float64| <= 4 x max |float32 torch composition on the same device - float64|.  Both
errors are printed and appended to profiles/sa_mlp_accuracy.log."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sa_mlp_ref as smr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "sa_mlp_accuracy.log")
WEIGHTS = ("Wx", "a1", "b1", "W2", "a2", "b2")


def _g(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(DEV)


def _n(t):
    return t.detach().cpu().numpy()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _device_inputs(case):
    t = dict(P=_g(case["P"]), xyz=_g(case["xyz"]), new_xyz=_g(case["new_xyz"]), idx=_g(case["idx"], np.int32),
             empty=_g(case["empty"], np.uint8))
    t.update({k: _g(case[k]) for k in WEIGHTS})
    return t


def _raw_run(case, t):
    """Through the C ABI on an output pre-filled with NaN: every element must be written."""
    from spx import _lib
    lib = _lib.load()
    c2, c1 = case["W2"].shape
    m, s = case["idx"].shape
    out = torch.full((m, c2), float("nan"), device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.spx_sa_mlp2_max(_p(t["P"]), _p(t["xyz"]), _p(t["new_xyz"]), _p(t["idx"]), _p(t["empty"]), _p(t["Wx"]),
                             _p(t["a1"]), _p(t["b1"]), _p(t["W2"]), _p(t["a2"]), _p(t["b2"]), c1, c2,
                             case["xyz"].shape[0], m, s, _p(out), stream)
    assert rc == 0
    torch.cuda.synchronize()
    return _n(out)


def _op(t, **over):
    from spx import ops
    a = dict(t, **over)
    return ops.sa_mlp2_max(a["P"], a["xyz"], a["new_xyz"], a["idx"], a["empty"].bool(), a["Wx"], a["a1"], a["b1"], a["W2"],
                           a["a2"], a["b2"])


# --------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("key", smr.exact_case_names(), ids=smr.case_id)
def test_exact_cases_bit_for_bit(key):
    case = smr.exact_case(key)
    t = _device_inputs(case)
    got = _raw_run(case, t)
    assert got.dtype == np.float32 and got.shape == case["out"].shape
    bad = np.argwhere(got.astype(np.float64) != case["out"])
    assert bad.size == 0, (smr.case_id(key), bad[:5], got[tuple(bad[0])], case["out"][tuple(bad[0])])
    assert np.array_equal(_n(_op(t)), got)                                   # the tensor-level op is the same call


def test_empty_mask_none_and_mask_of_zeros_agree():
    case = smr.exact_case(("p_none", 64, 16, 16, 65, 40))
    t = _device_inputs(case)
    from spx import ops
    zeros = torch.zeros_like(t["empty"])
    a = ops.sa_mlp2_max(None, t["xyz"], t["new_xyz"], t["idx"], None, *[t[k] for k in WEIGHTS])
    b = ops.sa_mlp2_max(None, t["xyz"], t["new_xyz"], t["idx"], zeros.bool(), *[t[k] for k in WEIGHTS])
    ref = smr.sa_mlp2_max(None, case["xyz"], case["new_xyz"], case["idx"], None, *[case[k] for k in WEIGHTS])
    assert np.array_equal(_n(a), _n(b)) and np.array_equal(_n(a).astype(np.float64), ref)


# --------------------------------------------------------------------------------------------------------- refusals
def test_unsupported_shapes_and_grad_are_refused_by_name():
    from spx import _lib
    t = _device_inputs(smr.exact_case(("mixed", 16, 16, 16, 3, 40)))
    z = lambda *s: torch.zeros(*s, device=DEV)                                # noqa: E731
    with pytest.raises(_lib.SpxError, match=r"C1 = 24"):
        _op(t, P=z(40, 24), Wx=z(24, 3), a1=z(24), b1=z(24), W2=z(16, 24))
    with pytest.raises(_lib.SpxError, match=r"S = 8"):
        _op(t, idx=t["idx"][:, :8])
    with pytest.raises(_lib.SpxError, match=r"C2 = 48"):
        _op(t, W2=z(48, 16), a2=z(48), b2=z(48))
    with pytest.raises(_lib.SpxError, match=r"W2 requires grad"):
        _op(t, W2=t["W2"].clone().requires_grad_())
    with pytest.raises(_lib.SpxError, match=r"P requires grad"):
        _op(t, P=t["P"].clone().requires_grad_())
    with pytest.raises(_lib.SpxError, match=r"do not match"):
        _op(t, a1=z(32))
    with pytest.raises(_lib.SpxError, match=r"fp32"):
        _op(t, P=t["P"].double())


# --------------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", [k[0] for k in smr.FLOAT_CASES])
def test_float_accuracy_against_float64(name):
    case = smr.float_case(name)
    f32 = {k: _g(case[k]) for k in ("features", "xyz", "new_xyz", "Wf", "Wx", "W2", "a1", "b1", "a2", "b2")}
    idx, empty = _g(case["idx"], np.int32), _g(case["empty"], np.bool_)
    bn1, bn2 = [_g(v) for v in case["bn1"]], [_g(v) for v in case["bn2"]]
    with torch.no_grad():
        eager = smr.composition(f32["features"], f32["xyz"], f32["new_xyz"], idx, empty, f32["Wf"], f32["Wx"], bn1,
                                f32["W2"], bn2)
        from spx import ops
        fused = ops.sa_mlp2_max(f32["features"] @ f32["Wf"].t(), f32["xyz"], f32["new_xyz"], idx, empty, f32["Wx"],
                                f32["a1"], f32["b1"], f32["W2"], f32["a2"], f32["b2"])
    e_eager = float(np.abs(_n(eager).astype(np.float64) - case["out"]).max())
    e_fused = float(np.abs(_n(fused).astype(np.float64) - case["out"]).max())
    line = "%-12s max|out| %.3e  eager %.3e  fused %.3e  ratio %.2f" % (
        name, float(np.abs(case["out"]).max()), e_eager, e_fused, e_fused / max(e_eager, 1e-300))
    print(line)
    with open(LOG, "a") as fh:
        fh.write(line + "\n")
    assert e_eager > 0 and e_fused <= 4.0 * e_eager, line


# --------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_are_bit_equal():
    case = smr.float_case("roi_grid_0")
    t = {k: _g(case[k]) for k in ("xyz", "new_xyz") + WEIGHTS}
    t.update(P=_g(case["features"] @ case["Wf"].T), idx=_g(case["idx"], np.int32), empty=_g(case["empty"], np.uint8))
    a = _op(t)
    b = _op(t)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_graph_capture_and_replay_with_changed_idx():
    case = smr.exact_case(("mixed", 64, 64, 32, 65, 40))
    other = smr.exact_case(("negative_l1", 64, 64, 32, 65, 40))              # the same shapes, other lists
    t = _device_inputs(case)
    empty = t["empty"].bool()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _op(t, empty=empty)                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _op(t, empty=empty)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_n(out).astype(np.float64), case["out"])
    t["idx"].copy_(_g(other["idx"], np.int32))
    empty.copy_(_g(other["empty"], np.bool_))
    graph.replay()
    torch.cuda.synchronize()
    fresh = _op(t, empty=empty)
    want = smr.sa_mlp2_max(case["P"], case["xyz"], case["new_xyz"], other["idx"], other["empty"],
                           *[case[k] for k in WEIGHTS])
    assert torch.equal(out, fresh) and np.array_equal(_n(out).astype(np.float64), want)
    assert not np.array_equal(want, case["out"])
