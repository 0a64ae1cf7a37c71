"""The float64 restatement of spx_sa_mlp2_max (tests/sa_mlp_ref.py) equals the composition it replaces — grouped tensor,
Conv2d, eval BatchNorm2d, ReLU, Conv2d, BatchNorm2d, ReLU, max — on every exact case and every float case, the empty-ball
rule included.  CPU, float64."""
import numpy as np
import pytest
import torch

import sa_mlp_ref as smr


def _t(a, dtype=torch.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _composition_of_exact(case):
    """P enters the composition as features with Wf = identity; BatchNorms whose eval fold is (a, b)."""
    c1 = case["Wx"].shape[0]
    feats = _t(case["P"])
    wf = None if feats is None else torch.eye(c1, dtype=torch.float64)
    bn1 = [_t(v) for v in smr.identity_bn(case["a1"], case["b1"])]
    bn2 = [_t(v) for v in smr.identity_bn(case["a2"], case["b2"])]
    return smr.composition(feats, _t(case["xyz"]), _t(case["new_xyz"]), _t(case["idx"], torch.int64),
                           _t(case["empty"], torch.bool), wf, _t(case["Wx"]), bn1, _t(case["W2"]), bn2).numpy()


@pytest.mark.parametrize("key", smr.exact_case_names(), ids=smr.case_id)
def test_restatement_equals_composition_on_exact_cases(key):
    case = smr.exact_case(key)
    ref = _composition_of_exact(case)
    assert ref.shape == case["out"].shape == (key[4], key[2])
    scale = max(1.0, float(np.abs(case["out"]).max()))
    assert np.abs(ref - case["out"]).max() <= 1e-12 * scale


@pytest.mark.parametrize("name", [k[0] for k in smr.FLOAT_CASES])
def test_restatement_equals_composition_on_float_cases(name):
    case = smr.float_case(name)
    ref = smr.composition(_t(case["features"]), _t(case["xyz"]), _t(case["new_xyz"]), _t(case["idx"], torch.int64),
                          _t(case["empty"], torch.bool), _t(case["Wf"]), _t(case["Wx"]), [_t(v) for v in case["bn1"]],
                          _t(case["W2"]), [_t(v) for v in case["bn2"]]).numpy()
    assert case["empty"].any() and not case["empty"].all()
    assert np.abs(ref - case["out"]).max() <= 1e-12 * max(1.0, float(np.abs(case["out"]).max()))


def test_empty_ball_is_not_a_zero_row():
    """An empty ball runs the MLP over zero columns: relu(a2 * (W2 relu(b1)) + b2), which is not 0 in general; a row of
    idx outside [0, N) is such a column too, and a list made only of them equals an empty ball."""
    key = ("all_empty", 16, 32, 16, 65, 40)
    case = smr.exact_case(key)
    expect = np.maximum(case["a2"] * (case["W2"] @ np.maximum(case["b1"], 0)) + case["b2"], 0)
    assert expect.max() > 0 and np.array_equal(case["out"], np.tile(expect, (65, 1)))
    outside = np.full((65, 16), 40, np.int32)
    outside[::2] = -1
    args = [case[k] for k in ("Wx", "a1", "b1", "W2", "a2", "b2")]
    got = smr.sa_mlp2_max(case["P"], case["xyz"], case["new_xyz"], outside, np.zeros(65, bool), *args)
    assert np.array_equal(got, case["out"])
    assert np.array_equal(_composition_of_exact(dict(case, idx=outside, empty=np.zeros(65, bool))), case["out"])


def test_cases_cover_what_they_claim():
    names = smr.exact_case_names()
    assert {k[1:4] for k in names} == set(smr.SHAPES)
    assert {(k[4], k[5]) for k in names if k[0] == "mixed"} == {(m, n) for m in smr.MS for n in smr.NS}
    assert {k[0] for k in names} == set(smr.KINDS)
    mixed = smr.exact_case(("mixed", 64, 64, 16, 65, 40))
    idx, empty = mixed["idx"], mixed["empty"]
    assert empty.any() and not empty.all()
    assert (idx == 39).any() and ((idx < 0) | (idx >= 40)).any()
    live = idx[~empty]
    assert any((row[1:] == row[0]).any() for row in live)                         # slots that repeat the first hit
    d = smr.exact_case(("distinct_w2", 16, 32, 16, 65, 40))["W2"]
    assert d.shape == (32, 16) and np.unique(d).size == d.size
    neg = smr.exact_case(("negative_l1", 32, 32, 32, 65, 40))
    assert (neg["b1"][1::2] > 0).all() and (neg["P"][:, 0::2] < -100).all()
    assert smr.exact_case(("p_none", 64, 16, 16, 65, 40))["P"] is None
