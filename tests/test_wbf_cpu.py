"""Weighted box fusion without a GPU: the C ABI's new symbols and refusals' wording, and the properties of the restatement
tests/wbf_oracle.py that the GPU tests (tests/test_gpu_wbf.py) rely on - so that none of them can pass vacuously."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nms_stage_oracle as ns  # noqa: E402
import wbf_cases as wc  # noqa: E402
import wbf_oracle as wo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["yn_wbf_merge", "yn_wbf_lds_clusters", "yn_wbf_cost", "yn_merge_rule_tta", "yn_merge_rule_slice", "yn_fuse_create", "yn_fuse_destroy",
       "yn_fuse_open", "yn_fuse_append", "yn_fuse_merge", "yn_fuse_result", "yn_fuse_lists"]


def nms_merge_oracle(boxes, scores, cls, C, thr):
    """yn_nms_merge restated: per class greedy NMS in pick order, kept rows in ascending row order -> row indices."""
    keep = []
    for c in range(C):
        ids = ns.sort_segment(np.flatnonzero(cls == c), scores)
        keep += list(ids[ns.greedy(boxes[ids], thr)])
    return np.sort(np.asarray(keep, np.int64))


def test_symbols_in_the_library_and_the_ctypes_table():
    from yolo_nano_amd import build, capi
    build.build()
    exported = set(re.findall(r" T (yn_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()))
    for name in NEW:
        assert name in exported and name in capi.SIGNATURES, name
    lib = capi.load_library()
    L = lib.yn_wbf_lds_clusters()
    assert L >= 64 and L % 64 == 0
    assert lib.yn_abi_version() == 2
    assert capi.MERGE_NMS == 0 and capi.MERGE_WBF == 1 and capi.merge_rule_id("wbf") == 1
    with pytest.raises(ValueError, match="'nms' or 'wbf'"):
        capi.merge_rule_id("soft")
    # the cost model: a row meets at most min(rows before it, clusters) clusters, 64 per step, and takes at least one step
    assert lib.yn_wbf_cost(0, 0) == 0 and lib.yn_wbf_cost(1, 1) == 1
    assert lib.yn_wbf_cost(64, 64) == 64 and lib.yn_wbf_cost(66, 66) == 67      # row 65 meets 65 clusters: two steps
    assert lib.yn_wbf_cost(1000, 10) == 1000
    n = 131072
    assert lib.yn_wbf_cost(n, n) == sum(max(1, -(-i // 64)) for i in range(n))


def test_refusals_are_worded_in_the_source():
    """No GPU here, so the refusals cannot be provoked: their reasons stand in the entry points (tests/test_gpu_wbf.py provokes them)."""
    src = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "yn_api.hip")).read()
    for text in ("yn_wbf_merge: expected is %d", "yn_wbf_merge: n is %d", "yn_wbf_merge: num_classes is %d, the handle has %d",
                 "is neither YN_MERGE_NMS (0) nor YN_MERGE_WBF (1)", "whose class is not an integer in 0..%d"):
        assert text in src, text
    hdr = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    assert "YN_MERGE_NMS = 0, YN_MERGE_WBF = 1" in hdr and "UNPINNED" in hdr
    assert '("kernels_wbf.hip", ["-ffp-contract=off"])' in open(os.path.join(ROOT, "yolo-nano_amd", "build.py")).read()


@pytest.mark.parametrize("case", wc.EXACT, ids=[c[0] for c in wc.EXACT])
def test_hand_built_cases_have_the_outcome_written_next_to_them(case):
    name, rows, thr, E, votes, founders = case
    boxes, scores, cls = wc._rows(rows)
    ob, osc, oc, of, ov, assign = wo.wbf(boxes, scores, cls, 3, thr, E)
    assert list(ov) == votes and list(of) == founders, (name, ov, of)
    assert list(oc) == [int(cls[f]) for f in founders]
    assert sorted(set(assign)) == sorted(founders) and all(assign[f] == f for f in founders)
    for i, f in enumerate(of):
        if ov[i] == 1:                                          # a single-vote cluster is its founder bit for bit; E = 1 keeps the score too
            assert wo.same_bits(ob[i], boxes[f])
            if E == 1:
                assert wo.same_bits(osc[i], scores[f])


def test_exact_values_of_some_cases():
    F = np.float32
    boxes, scores, cls, thr, E, _, _ = wc.exact_case("iou_equal_thr_no_join")
    assert wo.ovr(boxes[:1], boxes[1])[0] == F(0.5)
    boxes, scores, cls, thr, E, _, _ = wc.exact_case("equal_ovr_lowest_cluster")
    o = wo.ovr(boxes[:2], boxes[2])
    assert o[0] == o[1] > F(thr)
    boxes, scores, cls, thr, E, _, _ = wc.exact_case("votes_above_expected")
    ob, osc, _, _, ov, _ = wo.wbf(boxes, scores, cls, 1, thr, E)
    S = F(F(scores[0] + scores[1]) + scores[2])
    assert osc[0] == F(F(S / F(3)) * F(F(2) / F(2)))
    P = (scores[0] * boxes[0] + scores[1] * boxes[1]).astype(F) + scores[2] * boxes[2]
    assert wo.same_bits(ob[0], (P / S).astype(F))
    # fewer votes than expected mark the score down: 1 vote of 22
    boxes, scores, cls, thr, E, _, _ = wc.exact_case("single_row")
    _, osc, _, _, _, _ = wo.wbf(boxes, scores, cls, 3, thr, E)
    assert osc[0] == F(F(scores[0] / F(1)) * F(F(1) / F(22))) and osc[0] < scores[0]


@pytest.mark.parametrize("C", [1, 3, 80])
def test_without_overlap_and_one_expected_vote_wbf_is_the_nms_merge(C):
    boxes, scores, cls = wc.grid(150, C=C, seed=C)
    ob, osc, oc, of, ov, assign = wo.wbf(boxes, scores, cls, C, 0.55, 1)
    keep = nms_merge_oracle(boxes, scores, cls, C, 0.55)
    assert len(keep) == 150 and np.array_equal(of, keep) and (ov == 1).all() and np.array_equal(assign, np.arange(150))
    assert wo.same_bits(ob, boxes[keep]) and wo.same_bits(osc, scores[keep]) and np.array_equal(oc, cls[keep])
    # and on the clustered list with a threshold nothing reaches (IoU <= 1 < 2)
    boxes, scores, cls = wc.clustered(3, C=3)
    ob, osc, oc, of, ov, _ = wo.wbf(boxes, scores, cls, 3, 2.0, 1)
    keep = nms_merge_oracle(boxes, scores, cls, 3, 2.0)
    assert np.array_equal(of, keep) and wo.same_bits(ob, boxes[keep]) and wo.same_bits(osc, scores[keep])


def test_clusters_do_not_depend_on_the_row_order_when_scores_differ():
    boxes, scores, cls = wc.clustered(5)
    assert len(np.unique(scores)) == len(scores)
    ob, osc, oc, of, ov, assign = wo.wbf(boxes, scores, cls, 3, 0.55, 4)
    perm = np.random.default_rng(1).permutation(len(boxes))
    pb, ps, pc, pf, pv, pa = wo.wbf(boxes[perm], scores[perm], cls[perm], 3, 0.55, 4)

    def as_set(b, s, c, v):
        return sorted((bytes(np.ascontiguousarray(b[i])), float(s[i]), int(c[i]), int(v[i])) for i in range(len(b)))
    assert as_set(ob, osc, oc, ov) == as_set(pb, ps, pc, pv)
    assert np.array_equal(np.sort(perm[pf]), of)                # the same founders, named by their original rows


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_random_generator_exercises_joins_drift_and_capped_votes(seed):
    """What the GPU test on these lists needs the oracle to do, shown on the oracle alone."""
    boxes, scores, cls = wc.clustered(seed)
    assert 150 <= len(boxes) <= 320
    stats = {}
    ob, osc, oc, of, ov, assign = wo.wbf(boxes, scores, cls, 3, 0.55, 1, stats)
    K = len(ov)
    assert K < len(boxes) and (ov >= 2).sum() * 10 >= K, (K, ov)          # at least 10 % of the clusters have two or more votes
    assert stats.get("drift", 0) >= 1, stats                     # a join that matched the fused box but not the founder
    assert (ov > 4).any()                                        # more votes than a small E
    assert int(ov.sum()) == len(boxes) and (assign >= 0).all()
    # E only scales the scores
    ob4, osc4, _, of4, ov4, _ = wo.wbf(boxes, scores, cls, 3, 0.55, 4)
    assert wo.same_bits(ob, ob4) and np.array_equal(of, of4) and np.array_equal(ov, ov4) and not wo.same_bits(osc, osc4)


@pytest.mark.parametrize("K", [63, 64, 65])
def test_straddle_builder_ends_in_exactly_k_clusters(K):
    boxes, scores, cls = wc.straddle(K)
    ob, osc, oc, of, ov, assign = wo.wbf(boxes, scores, cls, 3, 0.55, 2)
    assert (oc == 1).sum() == K and (oc == 0).sum() == 5
    assert list(ov[oc == 1][-3:]) == [2, 2, 2] and (ov[oc == 1][:-3] == 1).all()
    # cluster k of the segment is grid box k: founders ascend with the creation order
    assert np.array_equal(of[oc == 1], 5 + np.arange(K))


def test_records_layout():
    boxes, scores, cls = wc.clustered(2)
    n = len(boxes)
    B = np.zeros((2, n + 3, 4), np.float32); S = np.zeros((2, n + 3), np.float32); Cl = np.full((2, n + 3), -1, np.int32)
    B[0, :n] = boxes; S[0, :n] = scores; Cl[0, :n] = cls
    B[1, :10] = boxes[:10]; S[1, :10] = scores[:10]; Cl[1, :10] = cls[:10]
    rec, off = wo.wbf_records(B, S, Cl, [n, 10], 3, 0.55, 2)
    ob, osc, oc, _, _, _ = wo.wbf(boxes, scores, cls, 3, 0.55, 2)
    assert off[1] == len(ob) and off.dtype == np.int32 and rec.shape == (off[2], 6) and rec.dtype == np.float32
    assert wo.same_bits(rec[:off[1], :4], ob) and wo.same_bits(rec[:off[1], 4], osc) and np.array_equal(rec[:off[1], 5], oc.astype(np.float32))
