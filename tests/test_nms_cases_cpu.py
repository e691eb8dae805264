"""The NMS-chain suite's own footing, proven without a GPU: (a) the composed stage restatements of tests/nms_stage_oracle.py give exactly the C
oracle's postprocess on every case of tests/nms_cases.py, (b) every case carries the plan the restated launch rules give, and the table reaches
every reachable value of every plan field, (c) every constructed sweep boundary has the property it claims, and the restated constants are
the source's."""
import os
import re

import numpy as np
import pytest

import nms_cases as nc
import nms_stage_oracle as so
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "kernels_post.hip")).read()


def _distinct_runs(case):
    seen = {}
    for run in case.runs:
        seen.setdefault((run[0], bool(case.plan_of(run)["prefilter"])), run)
    return list(seen.values())


@pytest.mark.parametrize("name", [c.name for c in nc.CASES])
def test_stage_chain_equals_the_oracle(name):
    case = nc.BY_NAME[name]
    for run in _distinct_runs(case):
        thresh = run[0]
        pl = dict(case.plan_of(run), B=case.B, N=case.N, C=case.C)
        for boxes, conf in case.images(thresh):
            cls, score = so.candidates(conf, nc.CONF)
            st = so.stages(boxes, cls, score, case.C, thresh, case.diou, pl)
            rb, rs, rc, ri = orc.postprocess(boxes, conf, nc.CONF, thresh, diou=case.diou, return_index=True)
            got = np.flatnonzero(st["keep"])
            assert np.array_equal(got, ri), (name, run[:2], len(got), len(ri))
            assert np.array_equal(boxes[got].view(np.uint32), rb.view(np.uint32)) and np.array_equal(score[got], rs) and np.array_equal(cls[got], rc)
            # the sorted list is a permutation of each class's candidates, ordered by (score descending, id descending)
            for c in range(case.C):
                ids = st["bucket"][st["seg_off"][c]:st["seg_off"][c] + st["seg_count"][c]]
                assert np.array_equal(np.sort(ids), np.flatnonzero(cls == c))
                s = score[ids]
                assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (ids[:-1] > ids[1:])))


def test_every_case_carries_the_plan_of_the_restated_rules():
    for case in nc.CASES:
        for thresh, mode, p in case.runs:
            want = so.plan(case.B, case.N, case.C, thresh, case.diou, mode, True)
            got = dict(case.plan_of((thresh, mode, p)), B=case.B, N=case.N, C=case.C)
            assert got == want, (case.name, thresh, mode, got, want)
            assert got["fused"] == got["few"] and got["chunks"] == 1 - got["few"]          # the unreachable branches (nms_cases' docstring)


def test_table_reaches_every_reachable_plan_value():
    seen = {k: set() for k in nc.PLAN}
    for case in nc.CASES:
        for run in case.runs:
            for k, v in case.plan_of(run).items():
                seen[k].add(v)
    want = dict(few={0, 1}, fused={0, 1}, chunks={0, 1}, merge={0, 1}, prefilter={0, 1}, pre_ranks={0, 1, 2, 3, 4}, sweep={0, 1},
                sweep_maxn={0, 3072, 6144}, sweep_slots={0, 1, 2, 3, 4}, sweep_split={0, 2, 3, 4, 5, 6, 7, 8}, resolve_one={0, 1},
                resolve_split={0, 1}, diou={0, 1})
    assert seen == want
    # combinations that are routes of their own: the prefilter on the few route (no sliced ranks), the one-launch resolve behind the chunked
    # sort (N > 16 384 at few classes), the chunked sort without a merge, the sweep refused by the threshold alone
    plans = [(c.B * c.C, c.N, c.plan_of(r), r[0]) for c in nc.CASES for r in c.runs]
    assert any(p["few"] and p["prefilter"] and p["pre_ranks"] == 0 for _, _, p, _ in plans)
    assert any(p["chunks"] and p["resolve_one"] and p["sweep"] for _, _, p, _ in plans)
    assert any(p["chunks"] and not p["merge"] for _, _, p, _ in plans)
    assert any(p["prefilter"] and not p["sweep"] and not p["few"] and n > 1024 and t < 1e-6 for _, n, p, t in plans)


def test_restated_constants_are_the_sources():
    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, SRC).group(1))
    assert define("YN_SORT_SMALL") == so.SORT_SMALL and define("YN_SORT_LARGE") == so.SORT_LARGE and define("YN_SWEEP_MAXN") == so.SWEEP_MAXN
    assert define("YN_SWEEP_IRR") == so.SWEEP_IRR and define("YN_SWEEP_WIDE") == so.SWEEP_WIDE
    assert (define("YN_PRE_W"), define("YN_PRE_Z"), define("YN_PRE_RANKS"), define("YN_PRE_TICKETS")) == (so.PRE_W, so.PRE_Z, so.PRE_RANKS, so.PRE_TICKETS)
    flat = re.sub(r"\s+", "", SRC)
    for rule in ("constexprintfew_n=16384;", "constboolfew=(long)B*C<=256&&N<=few_n;", "nms_thresh>=1e-6f", "sweep_maxn=N<=16384?YN_SWEEP_MAXN/2:YN_SWEEP_MAXN;",
                 "sweep_slots=large_cap<4?large_cap:4;", "intsweep_split=(sweep_maxn*20<=64*1024?256:128)/(B>0?B:1);",
                 "prefilter_env==2||(prefilter_env==1&&B>=4)", "constboolsplit=N>YN_SORT_SMALL&&wk.large_list&&large_cap>0;",
                 "returnL.keepm<=(unsignedlonglong)m*(unsignedlonglong)(m-1)/8ull;", "boolnms_colmajor(intn){returnn>1024;}"):
        assert rule in flat, rule
    api = re.sub(r"\s+", "", open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "yn_api.hip")).read())
    assert "w.large_cap=(N/1024+1)<C?(N/1024+1):C;" in api


@pytest.mark.parametrize("name", [c.name for c in nc.CASES if c.claims])
def test_sweep_boundaries_have_the_claimed_properties(name):
    case = nc.BY_NAME[name]
    for run in case.runs:
        thresh = run[0]
        pl = dict(case.plan_of(run), B=case.B, N=case.N, C=case.C)
        assert pl["sweep"]
        for img, claims in case.claims.items():
            boxes, conf = case.images(thresh)[img]
            cls, score = so.candidates(conf, nc.CONF)
            counts, off, large, order = so.bucket(cls, case.C)
            for c, claim in claims.items():
                ids = so.sort_segment(np.flatnonzero(cls == c), score)
                sb = boxes[ids]; n = len(sb)
                kept0, surv = so.prefilter(sb, thresh)
                assert kept0.all() and np.array_equal(surv, np.arange(64, n)) and n - 64 == claim["n2"], (c, n, len(surv))     # n2 = n - 64
                listed = c in large[:pl["sweep_slots"]] and order.index(c) < pl["pre_ranks"]
                assert listed == (not claim.get("fifth", False))
                visits, limit, nirr = so.sweep_visits(sb)
                want = so.sweep_expected(sb, len(surv), listed, pl["sweep_maxn"])
                assert want == claim["sparse"], (c, want, visits, limit, nirr)
                if claim["sparse"] is None:
                    assert limit < 2 * visits < 2 * limit                                    # between half the limit and the limit: the kernel's bins decide
                elif listed and nirr <= so.SWEEP_IRR and n - 64 <= so.SWEEP_MAXN:
                    assert 2 * visits <= limit                                               # (refused, where it is, by n2 or the irregular list - not by the estimate)
                if "irregular" in claim:
                    assert nirr == claim["irregular"]
                t = sb[64:]
                if "wide" in claim:                                                          # strips that each visit every box: more than YN_SWEEP_WIDE of them
                    full = (t[:, 0] <= t[:, 0].min()) & (t[:, 2] >= t[:, 2].max())
                    assert full.sum() == claim["wide"] > so.SWEEP_WIDE
                assert (t[:, 0] < 0).any() and (t[:, 2] > 1).any()
                touch = 0                                                                    # x2_i == x1_j with overlapping y
                for j in np.flatnonzero(np.isin(t[:, 0], t[:, 2])):
                    i = np.flatnonzero(t[:, 2] == t[j, 0])
                    touch += bool((np.minimum(t[i, 3], t[j, 3]) > np.maximum(t[i, 1], t[j, 1])).any())
                assert touch >= 20
                partners = len(t) - len(np.unique(t[:, [0, 1, 3]], axis=0))                  # same x1 and y extent, another x2: x-extents intersect
                assert partners >= 20
