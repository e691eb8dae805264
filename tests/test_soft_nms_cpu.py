"""Soft-NMS without a GPU: the C ABI's new symbols and refusals' wording, the properties of the specification's exp, and the properties
of the restatement tests/soft_nms_oracle.py that the GPU tests (tests/test_gpu_soft_nms.py) rely on - so that none of them can pass
vacuously."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nms_stage_oracle as ns  # noqa: E402
import soft_nms_cases as sc  # noqa: E402
import soft_nms_oracle as so  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["yn_soft_nms_merge", "yn_soft_nms", "yn_soft_lds_rows", "yn_op_soft_exp", "yn_merge_soft_tta", "yn_merge_soft_slice", "yn_merge_soft_fuse"]


def test_symbols_in_the_library_and_the_ctypes_table():
    from yolo_nano_amd import build, capi
    build.build()
    exported = set(re.findall(r" T (yn_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()))
    for name in NEW:
        assert name in exported and name in capi.SIGNATURES, name
    lib = capi.load_library()
    L = lib.yn_soft_lds_rows()
    assert L >= 256 and L % 256 == 0
    assert lib.yn_abi_version() == 2
    assert (capi.SOFT_OFF, capi.SOFT_HARD, capi.SOFT_LINEAR, capi.SOFT_GAUSSIAN) == (0, 1, 2, 3) == (so.OFF, so.HARD, so.LINEAR, so.GAUSSIAN)
    assert [capi.soft_method_id(m) for m in (None, "hard", "linear", "gaussian")] == [0, 1, 2, 3]
    for bad in ("soft", "nms", 2, ""):
        with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
            capi.soft_method_id(bad)
    # Soft-NMS is not a third merge rule
    with pytest.raises(ValueError, match="'nms' or 'wbf'"):
        capi.merge_rule_id("soft")
    with pytest.raises(ValueError, match="soft='linear' cannot be combined with merge='wbf'"):
        capi.check_soft_with_merge("x", "wbf", "linear")
    assert capi.check_soft_with_merge("x", "nms", "linear") == 2 and capi.check_soft_with_merge("x", "wbf", None) == 0


def test_refusals_are_worded_in_the_source():
    """No GPU here, so the refusals cannot be provoked: their reasons stand in the entry points (tests/test_gpu_soft_nms.py provokes them)."""
    src = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "yn_api.hip")).read()
    for text in ("%s: method %d is not %sYN_SOFT_HARD (1), YN_SOFT_LINEAR (2) or YN_SOFT_GAUSSIAN (3)", "%s: sigma is %g (it must be positive and finite)",
                 "%s: score_floor is %g (it must be 0 or more and finite)", "yn_soft_nms_merge: n is %d", "yn_soft_nms_merge: num_classes is %d, the handle has %d",
                 "yn_infer: Soft-NMS (yn_soft_nms method %d) has no DIoU form", "yn_postprocess: Soft-NMS (yn_soft_nms method %d) has no DIoU form",
                 "is neither YN_MERGE_NMS (0) nor YN_MERGE_WBF (1)"):
        assert text in src, text
    hdr = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    assert "YN_MERGE_NMS = 0, YN_MERGE_WBF = 1" in hdr
    assert "YN_SOFT_OFF = 0, YN_SOFT_HARD = 1, YN_SOFT_LINEAR = 2, YN_SOFT_GAUSSIAN = 3" in hdr and hdr.count("UNPINNED") >= 2
    from yolo_nano_amd import build
    assert ("kernels_soft.hip", ["-ffp-contract=off"]) in build.SOURCES


# ---- E: a property of the specification, not of the kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lo", [-2.0, -10.0, -87.0])
def test_exp_is_within_one_ulp_of_float64_exp_and_monotone(lo):
    rng = np.random.default_rng(int(-lo))
    x = np.concatenate([rng.uniform(lo, 0.0, 1_500_000), np.linspace(lo, 0.0, 1_000_001)]).astype(F)
    y = so.E(x)
    assert y.dtype == F and y.shape == x.shape
    ref = np.exp(x.astype(np.float64))
    ulp = np.spacing(ref.astype(F)).astype(np.float64)
    err = float((np.abs(y.astype(np.float64) - ref) / ulp).max())
    print("E on [%g, 0]: largest error %.3f ulp" % (lo, err))
    assert err <= 1.0, err
    assert not (y > F(1)).any() and (y > F(0)).all()
    ys = so.E(np.sort(x))
    assert not (np.diff(ys) < 0).any()


def test_exp_edge_values():
    assert so.E(F(0.0)) == F(1) and so.E(F(-0.0)) == F(1)
    assert so.same_bits(so.E(F(-87.0)), F(1.6458115e-38))
    assert so.E(F(-87.0001)) == F(0) and so.same_bits(so.E(F(-87.0001)), F(0.0))
    assert np.isnan(so.E(F(np.nan)))
    assert so.E(np.array([-np.inf, -1e30], F)).tolist() == [0.0, 0.0]
    # elementwise: an array gives what its elements give
    x = np.array([0.0, -0.5, -87.0, -88.0, np.nan, -3.25], F)
    assert so.same_bits(so.E(x), np.array([so.E(v) for v in x], F))


# ---- the hand-built cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.EXACT, ids=[c[0] for c in sc.EXACT])
def test_hand_built_cases_have_the_outcome_written_next_to_them(case):
    name, rows, method, thr, sigma, floor, kept, scores = case
    boxes, score, cls = sc._rows(rows)
    ob, osc, oc, oi = so.soft_nms(boxes, score, cls, 3, method, thr, sigma, floor)
    assert list(oi) == kept, (name, oi, osc)
    assert so.same_bits(ob, boxes[kept].reshape(-1, 4)) and list(oc) == [int(cls[r]) for r in kept]
    for got, want in zip(osc, scores):
        if want is not None:
            assert got == F(want), (name, got, want)
    assert ob.dtype == F and osc.dtype == F and oc.dtype == np.int32 and oi.dtype == np.int32


def test_exact_values_of_some_cases():
    boxes, *_ = sc.exact_case("ovr_equal_thr_not_hit")
    assert so.ovr(boxes[0], boxes[1:])[0] == F(0.5)
    boxes, *_ = sc.exact_case("inverted_box_nan_ovr_hard")
    assert np.isnan(so.ovr(boxes[0], boxes[1:])[0])
    boxes, *_ = sc.exact_case("ovr_above_one_linear_negative")
    o = so.ovr(boxes[0], boxes[1:])[0]
    assert o > F(1.5) and np.isfinite(o) and so.weight(o, so.LINEAR, 0.5, 0.5) < 0
    boxes, score, cls, method, thr, sigma, floor, kept, _ = sc.exact_case("chain_dynamic_argmax_gaussian")
    o = so.ovr(boxes[0], boxes[1:])
    assert o[0] == F(0.5) and o[1] == F(0.5) / F(5.5) and so.ovr(boxes[2], boxes[1:2])[0] == F(0.5) / F(3.5)
    # the dynamic arg-max drops B; decaying in the static order A, B, C would keep it
    b_dynamic = score[1] * so.E(-(o[0] * o[0] / F(sigma))) * so.E(-((F(0.5) / F(3.5)) ** 2 / F(sigma)))
    b_static = score[1] * so.E(-(o[0] * o[0] / F(sigma)))
    assert b_dynamic < F(floor) < b_static
    _, osc, _, oi = so.soft_nms(boxes, score, cls, 1, method, thr, sigma, floor)
    assert list(oi) == [0, 2] and osc[1] == score[2] * so.E(-(o[1] * o[1] / F(sigma)))
    # equal only after the decay: without the tie rule's "higher row" the scores of rows 1 and 2 would be swapped
    boxes, score, cls, method, thr, sigma, floor, kept, want = sc.exact_case("equal_after_decay_higher_row_first")
    _, osc, _, _ = so.soft_nms(boxes, score, cls, 1, method, thr, sigma, floor)
    assert osc[2] == F(0.25) and osc[1] == F(want[1]) < F(0.25)


def test_the_pick_is_sort_segments_first_row():
    """pick() is the arg-max the specification words; nms_stage_oracle.sort_segment's first row is the same row, ties included."""
    rng = np.random.default_rng(4)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        rows = rng.permutation(100)[:n].astype(np.int64)
        s = rng.integers(1, 6, n).astype(F) / F(8)             # many ties
        live = rng.random(n) < 0.7
        if not live.any():
            continue
        full = np.zeros(100, F); full[rows] = s
        assert rows[so.pick(rows, s, live)] == ns.sort_segment(rows[live], full)[0]


# ---- the two identities, on the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hard_at_floor_zero_is_the_nms_merge(seed):
    boxes, scores, cls = sc.clustered(seed)
    assert (scores > 0).all()
    for thr in (0.3, 0.5):
        a = so.soft_nms(boxes, scores, cls, 3, so.HARD, thr, 0.5, 0.0)
        b = so.nms_merge(boxes, scores, cls, 3, thr)
        assert len(a[3]) < len(boxes)
        assert all(so.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("C", [1, 3, 80])
def test_linear_without_a_hit_is_the_nms_merge(C):
    boxes, scores, cls = sc.grid(150, C=C, seed=C)
    a = so.soft_nms(boxes, scores, cls, C, so.LINEAR, 0.5, 0.5, 0.0)
    b = so.nms_merge(boxes, scores, cls, C, 0.5)
    assert len(a[3]) == 150 and all(so.same_bits(x, y) for x, y in zip(a, b))
    # and on a crowded list at a threshold nothing reaches
    boxes, scores, cls = sc.clustered(3)
    a = so.soft_nms(boxes, scores, cls, 3, so.LINEAR, 2.0, 0.5, 0.0)
    b = so.nms_merge(boxes, scores, cls, 3, 2.0)
    assert len(a[3]) == len(boxes) and all(so.same_bits(x, y) for x, y in zip(a, b))


# ---- the generator does what the GPU tests need ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [so.LINEAR, so.GAUSSIAN])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_random_generator_exercises_decay_drops_and_extra_rows(seed, method):
    boxes, scores, cls = sc.clustered(seed)
    assert len(np.unique(scores)) == len(scores)               # no natural ties: the tie cases are hand-built
    trace = []
    ob, osc, oc, oi = so.soft_nms(boxes, scores, cls, 3, method, 0.5, 0.5, 0.05, trace)
    decayed = int((osc != scores[oi]).sum())
    dropped = len(boxes) - len(oi)
    nms_rows = set(so.nms_merge(boxes, scores, cls, 3, 0.5)[3].tolist())
    extra = len(set(oi.tolist()) - nms_rows)
    print("seed %d method %d: %d rows, %d kept, %d decayed, %d dropped, %d not in the NMS result" % (seed, method, len(boxes), len(oi), decayed, dropped, extra))
    assert decayed >= 15 and dropped >= 100 and extra >= 1
    assert (osc <= scores[oi]).all() and (osc > F(0.05)).all()
    assert len(np.unique(osc)) == len(osc)                     # and none after the decays among the kept rows
    assert so.same_bits(ob, boxes[oi]) and np.array_equal(oc, cls[oi]) and (np.diff(oi) > 0).all()


def test_the_kept_set_does_not_depend_on_the_row_order_when_scores_differ():
    boxes, scores, cls = sc.clustered(5)
    assert len(np.unique(scores)) == len(scores)
    perm = np.random.default_rng(1).permutation(len(boxes))
    for method in sc.METHODS:
        ob, osc, oc, oi = so.soft_nms(boxes, scores, cls, 3, method, 0.5, 0.5, 0.05)
        pb, ps, pc, pi = so.soft_nms(boxes[perm], scores[perm], cls[perm], 3, method, 0.5, 0.5, 0.05)

        def as_set(b, s, c):
            return sorted((bytes(np.ascontiguousarray(b[i])), float(s[i]), int(c[i])) for i in range(len(b)))
        assert np.array_equal(np.sort(perm[pi]), oi)
        assert as_set(ob, osc, oc) == as_set(pb, ps, pc)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_straddle_builder(n):
    boxes, scores, cls = sc.straddle(n)
    assert (cls == 1).sum() == n and (cls == 0).sum() == 5 and len(np.unique(scores)) == len(scores)
    trace = []
    ob, osc, oc, oi = so.soft_nms(boxes, scores, cls, 2, so.LINEAR, 0.5, 0.5, 0.0, trace)
    hits = sum(int((~(o <= F(0.5))).sum()) for o in trace)
    assert n // 8 - 4 <= hits <= n // 8 + 1, hits              # about one row in eight overlaps a neighbour
    assert len(oi) == n + 5 and int((osc != scores[oi]).sum()) == hits
    assert len(so.soft_nms(boxes, scores, cls, 2, so.HARD, 0.5, 0.5, 0.0)[3]) == n + 5 - hits


def test_records_layout():
    boxes, scores, cls = sc.clustered(2)
    n = len(boxes)
    B = np.zeros((2, n + 3, 4), F); S = np.zeros((2, n + 3), F); Cl = np.full((2, n + 3), -1, np.int32)
    B[0, :n] = boxes; S[0, :n] = scores; Cl[0, :n] = cls
    B[1, :10] = boxes[:10]; S[1, :10] = scores[:10]; Cl[1, :10] = cls[:10]
    rec, off = so.soft_records(B, S, Cl, [n, 10], 3, so.GAUSSIAN, 0.5, 0.5, 0.05)
    ob, osc, oc, _ = so.soft_nms(boxes, scores, cls, 3, so.GAUSSIAN, 0.5, 0.5, 0.05)
    assert off[1] == len(ob) and off.dtype == np.int32 and rec.shape == (off[2], 6) and rec.dtype == F
    assert so.same_bits(rec[:off[1], :4], ob) and so.same_bits(rec[:off[1], 4], osc) and np.array_equal(rec[:off[1], 5], oc.astype(F))
