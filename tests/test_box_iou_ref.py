"""The float64 references of tests/box_iou_ref.py, checked without a GPU: against closed forms, against exact convex
clipping, for invariance under rigid motion and heading wraps; the input conditions of the families (share of
margin-unstable pairs, NMS threshold gaps); and the fp32 C oracle against the reference, which is where the tolerance
of the GPU test (box_iou_ref.TOL) is measured.  Run with -s to see the figures (profiles/box_iou_accuracy.log)."""
import functools

import numpy as np
import pytest

import box_iou_ref as R

NMS_LO, NMS_HI = 0.05, 0.5


@functools.lru_cache(maxsize=None)
def family(name):
    """-> (a, b, iou, overlap, clearance) of a family, computed once."""
    a, b = R.FAMILIES[name]()
    iou, clear = R.iou_ref(a, b)
    overlap, _ = R.iou_ref(a, b, overlap_only=True)
    return a, b, iou, overlap, clear


@functools.lru_cache(maxsize=None)
def nms_case(n):
    """-> (boxes, iou, clearance, threshold, half gap) of the rotated NMS draw of n boxes."""
    x = R.nms_boxes(n)
    iou, clear = R.iou_ref(x, x)
    thresh, half = R.gap_threshold(iou, NMS_LO, NMS_HI)
    return x, iou, clear, thresh, half


def test_families_are_fp32_and_small():
    assert set(R.family_key(k) for k in R.FAMILIES) == set(R.TOL) == set(R.UNSTABLE_CAP)
    for name, fam in R.FAMILIES.items():
        a, b = fam()
        assert a.dtype == b.dtype == np.float32 and a.shape[1] == b.shape[1] == 7, name
        assert 0 < a.shape[0] <= 256 and 0 < b.shape[0] <= 256, name
        a2, b2 = fam()
        assert np.array_equal(a, a2) and np.array_equal(b, b2), name             # fixed seeds


def test_reference_reproduces_closed_forms():
    """On the ideal boxes (float64, before the turned headings are rounded to fp32) to 1e-12."""
    a, b = R._grid_axis64()
    assert np.abs(R.overlap_ref(a, b)[0] - R.closed_form("grid_axis")[1]).max() < 1e-12
    touching = (R.axis_overlap(a, b) == 0) & (R.axis_overlap(a + [0, 0, 0, 2 * R.GRID, 2 * R.GRID, 0, 0], b) > 0)
    nested = R.axis_overlap(a, b) == (b[:, 3] * b[:, 4])[None]
    assert touching.sum() > 20 and nested.sum() > 20 and (R.axis_overlap(a, b) > 0).sum() > 1000
    for name, ideal in (("identical", R._identical64), ("octagon", R._octagon64)):
        a, b = ideal()
        known, area = R.closed_form(name)
        got, clear = R.overlap_ref(a, b)
        assert known.all() and np.abs(got - area).max() < 1e-12, name
        assert R.stable(clear).all(), name
    a, b = R._octagon64()
    cnt = R.vertex_count_ref(a, b).diagonal()
    assert (cnt[:64] == 8).all() and (cnt[64:] == 4).all()                       # crossings only, no corner inside
    # and the IoU of a box with itself, its half and a box four times its size
    box = np.array([[1.0, 2.0, 0, 4.0, 2.0, 1, 0.3]])
    half = np.array([[1.0 + np.cos(0.3), 2.0 + np.sin(0.3), 0, 2.0, 2.0, 1, 0.3]])
    big = np.array([[1.0, 2.0, 0, 8.0, 4.0, 1, 0.3 + np.pi]])
    assert abs(R.iou_ref(box, box)[0][0, 0] - 1.0) < 1e-12
    assert abs(R.iou_ref(box, half)[0][0, 0] - 0.5) < 1e-12
    assert abs(R.iou_ref(box, big)[0][0, 0] - 0.25) < 1e-12


def test_closed_forms_hold_for_the_fp32_boxes_within_the_stated_input_error():
    for name in R.FAMILIES:
        cf = R.closed_form(name)
        if cf is None:
            continue
        known, area = cf
        a, b, iou, overlap, clear = family(name)
        sa, sb = (a[:, 3].astype(np.float64) * a[:, 4])[:, None], (b[:, 3].astype(np.float64) * b[:, 4])[None]
        want = area / (sa + sb - area)
        err = np.abs(iou - want)[known].max()
        print("closed form vs reference on the fp32 boxes, %-22s max |IoU diff| %.3e (stated %.1e)"
              % (name, err, R.CLOSED_FORM_INPUT_ERR[R.family_key(name)]))
        assert err <= R.CLOSED_FORM_INPUT_ERR[R.family_key(name)] + 1e-12, name


def test_reference_agrees_with_exact_clipping_away_from_the_margin_band():
    """Clearance above 2e-2: no corner lies within 1e-2 of the other box's outline on either side, so the margin takes in
    no corner that is not inside and both algorithms build the same polygon."""
    for name in ("clustered", "thin", "grid_axis_rotated_1.0"):
        a, b, _, overlap, clear = family(name)
        far_from_band = clear > 2e-2
        if name == "clustered":
            assert far_from_band.mean() >= 0.5
            assert (far_from_band & (overlap > 0)).sum() > 1000
        truth = R.clip_area(a, b)
        err = np.abs(overlap - truth)[far_from_band].max()
        print("reference vs exact clipping, %-22s %5.1f %% of pairs qualify, max |diff| %.3e"
              % (name, 100 * far_from_band.mean(), err))
        assert err < 1e-9, name


def test_reference_is_invariant_under_rigid_motion_and_heading_wraps():
    a, b = R._grid_axis64()
    base, clear = R.iou_ref(a, b)
    assert R.stable(clear).all()
    for angle in R.GRID_ANGLES.values():
        got, _ = R.iou_ref(R.rotate_about_origin(a, angle), R.rotate_about_origin(b, angle))
        assert np.abs(got - base).max() < 1e-9, angle
    moved, _ = R.iou_ref(R.rotate_about_origin(a, np.pi / 4, (75.0, -75.0)), R.rotate_about_origin(b, np.pi / 4, (75.0, -75.0)))
    assert np.abs(moved - base).max() < 1e-9
    a, b = (x.astype(np.float64) for x in R.clustered())
    base, clear = R.iou_ref(a, b)
    ok = R.stable(clear)
    for k in range(-3, 4):
        wa, wb = a.copy(), b.copy()
        wa[:, 6] += 2 * np.pi * k
        wb[:, 6] += 2 * np.pi * k
        assert np.abs(R.iou_ref(wa, wb)[0] - base)[ok].max() < 1e-9, k
        wb[:, 6] -= 4 * np.pi                                                   # the operands need not wrap alike
        assert np.abs(R.iou_ref(wa, wb)[0] - base)[ok].max() < 1e-9, k


@pytest.mark.parametrize("name", list(R.FAMILIES))
def test_family_meets_its_unstable_share_cap(name):
    a, b, iou, overlap, clear = family(name)
    share = float((~R.stable(clear)).mean())
    print("%-22s %6d pairs, %5d overlap, unstable share %.4f %% (cap %.0f %%)"
          % (name, clear.size, int((overlap > 0).sum()), 100 * share, 100 * R.UNSTABLE_CAP[R.family_key(name)]))
    assert share <= R.UNSTABLE_CAP[R.family_key(name)]
    assert np.isfinite(iou).all() and iou.min() >= 0 and iou.max() <= 1 and np.isfinite(overlap).all()
    assert (overlap > 0).sum() >= 100                                           # the family is not vacuous


def test_families_reach_the_cases_they_are_for():
    a, b = R.near_identical()
    cnt = R.vertex_count_ref(a, b)
    assert cnt.max() == 16 and (cnt.diagonal() == 16).sum() >= 8                 # pts[16] filled exactly
    a, b, iou, overlap, _ = family("sub_margin")
    assert (a[:, 3:5] == 0).any() and (b[:, 3:5] == 0).any() and max(a[:, 3:5].max(), b[:, 3:5].max()) <= 0.02
    d = np.hypot(a[:, None, 0].astype(np.float64) - b[None, :, 0], a[:, None, 1].astype(np.float64) - b[None, :, 1])
    assert d.max() <= 0.03
    sa, sb = (a[:, 3].astype(np.float64) * a[:, 4])[:, None], (b[:, 3].astype(np.float64) * b[:, 4])[None]
    assert ((sa + sb - overlap < R.K_EPS) & (overlap > 0)).sum() > 10            # the kEps clamp decides some
    assert (overlap / np.maximum(sa + sb - overlap, R.K_EPS) > 1).sum() > 10     # ... and the cap at 1 others
    a, b = R.wrapped_heading()
    assert np.abs(a[:, 6]).max() > 6 * np.pi - 3.2 and np.abs(b[:, 6]).max() > 6 * np.pi - 3.2
    a, b = R.far()
    assert np.abs(a[:, :2]).max() > 150 and (np.abs(a[:, :2]).min(1) > 40).all()
    a, b, _, overlap, _ = family("thin")
    assert (overlap[np.arange(96, 128), np.arange(96, 128)] > 0.05).sum() >= 4   # near-parallel partners overlap at length


def test_oracle_fp32_error_fits_tol(orc):
    """E_f = max |fp32 C oracle - float64 reference| over the margin-stable pairs of each family; 4 E_f must fit TOL."""
    worst = {}
    for name in R.FAMILIES:
        a, b, iou, overlap, clear = family(name)
        ok = R.stable(clear)
        e_iou = float(np.abs(orc.boxes_iou_bev(a, b).astype(np.float64) - iou)[ok].max())
        e_ov = float(np.abs(orc.boxes_iou_bev(a, b, overlap_only=True).astype(np.float64) - overlap)[ok].max())
        key = R.family_key(name)
        print("oracle fp32 vs float64 reference, %-22s E(iou) %.3e  E(overlap) %.3e  ->  TOL iou %.1e overlap %.1e"
              % (name, e_iou, e_ov, R.TOL[key]["iou"], R.TOL[key]["overlap"]))
        worst[key] = (max(worst.get(key, (0, 0))[0], e_iou), max(worst.get(key, (0, 0))[1], e_ov))
        on_unstable = orc.boxes_iou_bev(a, b)[~ok]
        assert np.isfinite(on_unstable).all() and (on_unstable >= 0).all() and (on_unstable <= 1).all()
    for key, (e_iou, e_ov) in worst.items():
        assert 4 * e_iou <= R.TOL[key]["iou"] and 4 * e_ov <= R.TOL[key]["overlap"], key
        # ... and TOL is not padded: at most twice what the rule max(4 E, 1e-6) gives for today's E
        assert R.TOL[key]["iou"] <= 2 * max(4 * e_iou, 1e-6) and R.TOL[key]["overlap"] <= 2 * max(4 * e_ov, 1e-6), key


@pytest.mark.parametrize("n", R.NMS_SIZES)
def test_nms_draws_are_stable_and_thresholds_sit_in_wide_gaps(n, orc):
    x, iou, clear, thresh, half = nms_case(n)
    upper = np.triu_indices(n, 1)
    assert R.stable(clear)[upper].all()                                          # NMS_SEEDS: no pair left out
    tol = R.TOL["clustered"]["iou"]
    keep = R.greedy_ref(iou, thresh)
    print("n %4d rotated: threshold %.6f, half gap %.2e (>= 10 TOL = %.1e), keeps %d" % (n, thresh, half, 10 * tol, len(keep)))
    assert NMS_LO < thresh < NMS_HI and half >= 10 * tol
    assert np.abs(iou[upper] - thresh).min() >= half * (1 - 1e-9)
    assert n // 8 < len(keep) < n                                                # it suppresses, and not everything
    assert np.array_equal(orc.nms_bev(x, thresh), keep)
    g = R.nms_boxes(n, grid=True)
    ion = R.iou_normal_ref(g, g)
    thresh_n, half_n = R.gap_threshold(ion, NMS_LO, NMS_HI)
    keep_n = R.greedy_ref(ion, thresh_n)
    print("n %4d axis-aligned: threshold %.6f, half gap %.2e, keeps %d" % (n, thresh_n, half_n, len(keep_n)))
    assert half_n >= 1e-4 and n // 8 < len(keep_n) < n      # exact-grid boxes: only the division rounds (6e-8 relative)
    assert np.array_equal(orc.nms_bev(g, thresh_n, True), keep_n)


def test_greedy_ref_and_gap_threshold_on_known_answers():
    iou = np.array([[1, .6, .1, .0], [.6, 1, .7, .0], [.1, .7, 1, .3], [.0, .0, .3, 1.]])
    assert R.greedy_ref(iou, 0.5).tolist() == [0, 2, 3]          # 1 is suppressed and therefore spares 2
    assert R.greedy_ref(iou, 0.6).tolist() == [0, 1, 3]          # strict: 0.6 is not above 0.6
    assert R.greedy_ref(iou, 0.05).tolist() == [0, 3]
    assert R.greedy_ref(np.zeros((0, 0)), 0.5).tolist() == []
    thresh, half = R.gap_threshold(iou, 0.05, 0.65)
    assert abs(thresh - 0.45) < 1e-12 and abs(half - 0.15) < 1e-12
    for n in (1, 2, 63, 64, 65, 128, 129, 193):
        for axis_aligned in (False, True):
            f = R.iou_normal_ref if axis_aligned else (lambda a, b: R.iou_ref(a, b)[0])
            assert R.greedy_ref(f(R.chain(n), R.chain(n)), 0.2).tolist() == list(range(0, n, 2))
            s = R.star(n)
            low = 1.0 / (s[0, 3] * s[0, 4])
            assert R.greedy_ref(f(s, s), low / 2).tolist() == [0]
            assert R.greedy_ref(f(s, s), min(2 * low, 0.9)).tolist() == ([0] if n == 1 else list(range(n)))
            assert R.greedy_ref(f(R.all_identical(n), R.all_identical(n)), 0.9).tolist() == [0]
            assert R.greedy_ref(f(R.all_disjoint(n), R.all_disjoint(n)), 0.0).tolist() == list(range(n))
            if n > 1:
                assert R.greedy_ref(f(R.late_hit(n), R.late_hit(n)), 0.2).tolist() == list(range(n - 1))
    flush = R.nested_flush()
    assert float(R.iou_normal_ref(flush, flush)[0, 1]) == 0.5
    chain = R.chain(5)
    assert np.abs(R.iou_ref(chain, chain)[0][0, :3] - [1, 1 / 3, 0]).max() < 1e-12
