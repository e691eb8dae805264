"""The per-class NMS chain of csrc/kernels_post.hip, stage by stage, against the exact restatements of tests/nms_stage_oracle.py - bit for
bit, nothing under a tolerance.  The existing NMS tests (test_gpu_parity.py) see the kept set only, in ascending candidate order: a wrong tie
rule among boxes that do not overlap, a key misplaced by the merge, a prefilter that removes too few boxes or a sweep decision that flips leave
it unchanged, and a changed launch condition moves them onto other kernels unnoticed.  Here every run of tests/nms_cases.py asserts, in chain
order (the first failing stage names the culprit):
  plan      the launch plan of the call (yn_nms_stages) == the plan the case carries
  bucket    seg_count, seg_off
  sort      the sorted candidate ids of every class (score descending, id descending) and the sorted boxes, as bit patterns
  prefilter seg_count2, the survivors' ids and boxes per class; seg_sparse wherever the restated estimate is unambiguous
  keep      the keep flags, and the compacted outputs == the C oracle's postprocess
then the same call with the sweep off (same bits, plan without a sweep), once more as it was (tickets and counters back at zero) and once
more after a call of another shape - each time the whole dumped state equals the first run's.  yn_pack_detections on 130 images of 64
candidates, some empty.

Wrong libraries, built once each on scratch copies (decisions changed only - no address, bound, loop limit or barrier) and run once on the
MI355X through this module (34 tests) and through the 28 NMS / postprocess / infer tests of test_gpu_parity.py:
  (1) sort_merge_kernel's placement with the tie rule reversed (equal scores: lower id first).  Here 23 of 34 fail, every one at
      "sort: ids" (each run of the chunked route with a class above 1 024 boxes).  There every test written for the NMS passes
      (test_postprocess_large_classes_many_segments, test_prefilter_slices_boundaries_bit_exact, test_nms_sweep_..., test_postprocess_very_
      large_classes, the guard-band test); only the whole-network test_infer_config2_bs32 (both thresholds) notices, by ONE box of one image.
  (2) nms_prefilter_kernel taking every band word of a segment's last chunk as zero.  Here 14 fail, every run with the prefilter, at
      "prefilter: seg_count2" (e.g. 15 300 survivors for 15 296).  There 15 of 28 fail as well: the dense stage does NOT repair a prefilter
      that removes too few - the survivors are only tested against one another, chunk 0's kept boxes are not among them - so the kept
      sets grow (499 for 481).  What this module adds for this stage is the place, not the detection.
  (3) nms_sweep_kernel visiting one bin fewer at the right end of a box's extent.  Here 5 fail at "keep" (both sweep cases at both
      thresholds, and plan-B65-N2100-C4: 1 105 kept for 1 099); there 4 (test_nms_sweep_spread_out_large_segments_bit_exact and
      test_infer_config2_bs32, both parameters each).

Measured on the MI355X: 34 tests (32 runs of 16 cases, the refused shape, the pack test), the module in 5.0 s of wall time; the slowest run
(sweep-6144, 17 000 candidates) 0.33 s, the C oracle's references included.
"""
import functools

import numpy as np
import pytest
import torch

import nms_cases as nc
import nms_stage_oracle as so
from oracle import oracle as orc
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def h():
    from yolo_nano_amd import capi
    capi.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    hd = capi.Handle(320, 20, arch.MULTI_ANCHOR_SIZE, "1.0x", nc.CONF, 0.5, max_batch=2)
    yield hd
    hd.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def reference(name, thresh):
    """Per distinct image of the case: (cls, score, the C oracle's postprocess with indices).  Computed once, shared by the runs."""
    case = nc.BY_NAME[name]
    out = []
    for boxes, conf in case.images(thresh):
        cls, score = so.candidates(conf, nc.CONF)
        out.append((cls, score, orc.postprocess(boxes, conf, nc.CONF, thresh, diou=case.diou, return_index=True)))
    return out


@functools.lru_cache(maxsize=None)
def expected(name, thresh, plan_items):
    case = nc.BY_NAME[name]
    pl = dict(plan_items)
    return [so.stages(boxes, cls, score, case.C, thresh, case.diou, pl, with_keep=False)
            for (boxes, _), (cls, score, _) in zip(case.images(thresh), reference(name, thresh))]


def call(h, case, thresh, inputs):
    """-> (per image outputs [(boxes, scores, cls, index)], dumped stages)"""
    if case.entry == "merge":
        ob, osc, oc, oi = h.nms_merge(*inputs, case.C, thresh, case.diou)
        outs = [(ob.cpu().numpy(), osc.cpu().numpy(), oc.cpu().numpy(), oi.cpu().numpy())]
    else:
        o = [t.cpu().numpy() for t in h.postprocess(*inputs)]
        outs = [tuple(o[q][b, :o[4][b]] for q in range(4)) for b in range(case.B)]
    return outs, h.nms_stages(case.B, case.N, case.C)


def same_state(a, b):
    (oa, sa), (ob, sb) = a, b
    for x, y in zip(oa, ob):
        for p, q in zip(x, y):
            assert np.array_equal(bits(p) if p.dtype == np.float32 else p, bits(q) if q.dtype == np.float32 else q)
    assert sa["plan"] == sb["plan"]
    for k in ("seg_count", "keep", "seg_count2", "seg_sparse") + (() if sa["plan"]["fused"] else ("seg_off",)):      # (fused: the classes lie in arrival order)
        assert (sa[k] is None) == (sb[k] is None) and (sa[k] is None or np.array_equal(sa[k], sb[k])), k
    B, C = sa["seg_count"].shape
    for b in range(B):                                       # the candidate arrays: each class's own stretch (what lies behind it is scratch)
        for c in np.flatnonzero(sa["seg_count"][b]):
            p, q, n = int(sa["seg_off"][b, c]), int(sb["seg_off"][b, c]), int(sa["seg_count"][b, c])
            assert np.array_equal(sa["bucket"][b, p:p + n], sb["bucket"][b, q:q + n]) and np.array_equal(bits(sa["sbox"][b, p:p + n]), bits(sb["sbox"][b, q:q + n]))
            if sa["seg_count2"] is not None:
                n2 = int(sa["seg_count2"][b, c])
                assert np.array_equal(sa["bucket2"][b, p:p + n2], sb["bucket2"][b, q:q + n2]) and np.array_equal(bits(sa["sbox2"][b, p:p + n2]), bits(sb["sbox2"][b, q:q + n2]))


@pytest.mark.parametrize("name,ri", nc.RUNS, ids=["%s-%d" % r for r in nc.RUNS])
def test_nms_chain_stage_by_stage(h, name, ri):
    case = nc.BY_NAME[name]
    thresh, mode, _ = run = case.runs[ri]
    pl = dict(case.plan_of(run), B=case.B, N=case.N, C=case.C)
    imgs = case.images(thresh)
    ref = reference(name, thresh)
    exp = expected(name, thresh, tuple(sorted(pl.items())))
    if case.entry == "merge":
        cls, score, _ = ref[0]
        inputs = (dev(imgs[0][0]), dev(score), dev(cls.astype(np.int32)))
    else:
        inputs = (dev(np.stack([imgs[i][0] for i in case.image_of])), dev(np.stack([imgs[i][1] for i in case.image_of])))
    h.set_thresholds(nc.CONF, thresh, case.diou)
    h.nms_prefilter(mode)
    h.nms_sweep(True)
    try:
        first = outs, st = call(h, case, thresh, inputs)
        assert st["plan"] == pl, ("plan", st["plan"], pl)
        ambiguous = False
        for b, i in enumerate(case.image_of):
            e, (cls, score, (rb, rs, rc, ridx)) = exp[i], ref[i]
            boxes = imgs[i][0]
            assert np.array_equal(st["seg_count"][b], e["seg_count"]), ("bucket: seg_count", b)
            # (the fused few-segments kernel lays the classes out in the order their workgroups arrive: seg_off is any packing of the counts)
            off = st["seg_off"][b].astype(np.int64)
            if not pl["fused"]:
                assert np.array_equal(off, e["seg_off"]), ("bucket: seg_off", b)
            live = np.flatnonzero(e["seg_count"])
            o = np.argsort(off[live], kind="stable")
            assert off[live][o][0] == 0 if len(live) else True
            assert np.array_equal((off[live] + e["seg_count"][live])[o][:-1], off[live][o][1:]), ("bucket: seg_off is not a packing", b)
            for c in live:
                n, eo = int(e["seg_count"][c]), int(e["seg_off"][c])
                ids = e["bucket"][eo:eo + n]
                got = st["bucket"][b, off[c]:off[c] + n]
                assert np.array_equal(got, ids), ("sort: ids", b, c, n, int(np.flatnonzero(got != ids)[0]))
                assert np.array_equal(bits(st["sbox"][b, off[c]:off[c] + n]), bits(boxes[ids])), ("sort: boxes", b, c)
            if pl["prefilter"]:
                assert np.array_equal(st["seg_count2"][b], e["seg_count2"]), ("prefilter: seg_count2", b, st["seg_count2"][b][:12], e["seg_count2"][:12])
                for c in live:
                    ids2 = e["bucket2"][c]
                    assert np.array_equal(st["bucket2"][b, off[c]:off[c] + len(ids2)], ids2), ("prefilter: survivors", b, c)
                    assert np.array_equal(bits(st["sbox2"][b, off[c]:off[c] + len(ids2)]), bits(boxes[ids2])), ("prefilter: boxes", b, c)
                for c in range(case.C):
                    if e["seg_sparse"][c] is None:
                        ambiguous = True
                    else:
                        assert st["seg_sparse"][b, c] == e["seg_sparse"][c], ("sweep decision", b, c, int(e["seg_count"][c]))
            else:
                assert st["seg_count2"] is None
            keep = np.zeros(case.N, np.int32); keep[ridx] = 1
            assert np.array_equal(st["keep"][b], keep), ("keep", b, int(st["keep"][b].sum()), len(ridx))
            ob, osc, oc, oi = outs[b]
            assert len(osc) == len(rs), ("compact: count", b)
            assert np.array_equal(oi, ridx) and np.array_equal(bits(ob), bits(rb)) and np.array_equal(osc, rs) and np.array_equal(oc.astype(np.int64), rc), ("compact", b)
        if pl["sweep"]:
            assert st["seg_sparse"].sum() > 0 or not case.claims
            h.nms_sweep(False)
            o2, s2 = call(h, case, thresh, inputs)
            assert s2["plan"] == dict(pl, sweep=0, sweep_maxn=0, sweep_slots=0, sweep_split=0) and not s2["seg_sparse"].any()
            s2 = dict(s2, plan=st["plan"], seg_sparse=st["seg_sparse"])
            same_state(first, (o2, s2))                      # (also where the decision is ambiguous: either way the same bits)
            h.nms_sweep(True)
        if case.claims:                                      # (the constructed boundaries: undecided only where the table says so)
            assert ambiguous == any(v["sparse"] is None for cl in case.claims.values() for v in cl.values())
        same_state(first, call(h, case, thresh, inputs))     # tickets, ctr and the counters are back at zero
        r = np.random.RandomState(3)
        c = r.uniform(0.1, 0.9, (2, 100, 2)); wh = r.uniform(0.05, 0.2, (2, 100, 2))
        cf = np.zeros((2, 100, 5), np.float32); cf[:, np.arange(100), np.arange(100) % 5] = 0.5
        h.postprocess(dev(np.concatenate([c - wh / 2, c + wh / 2], 2).astype(np.float32)), dev(cf))
        same_state(first, call(h, case, thresh, inputs))     # ... and after a call of another (B, N, C)
    finally:
        h.set_thresholds(nc.CONF, 0.5, False)
        h.nms_prefilter(1)
        h.nms_sweep(True)


def test_nms_stages_refuses_another_shape(h):
    from yolo_nano_amd import capi
    cf = np.zeros((1, 70, 5), np.float32); cf[0, np.arange(70), np.arange(70) % 5] = 0.5
    b = np.random.RandomState(1).uniform(0.1, 0.9, (1, 70, 4)).astype(np.float32)
    h.postprocess(dev(b), dev(cf))
    assert h.nms_stages(1, 70, 5)["plan"]["few"] == 1
    with pytest.raises(capi.YnError):
        h.nms_stages(2, 70, 5)


def test_pack_detections_130_images(h):
    """pack_kernel's count loop strides by 64: B = 130 images of 64 candidates, some of them empty; offsets and records == the per-image outputs."""
    B, N, C = 130, 64, 4
    r = np.random.RandomState(7)
    ctr = r.uniform(0.1, 0.9, (B, N, 2)); wh = r.uniform(0.05, 0.3, (B, N, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).astype(np.float32)
    conf = np.zeros((B, N, C), np.float32)
    conf[np.arange(B)[:, None], np.arange(N)[None], r.randint(0, C, (B, N))] = nc.SCORES[r.randint(0, 5, (B, N))]
    for b in (0, 5, 63, 64, 129):
        conf[b] = 0.0
    h.set_thresholds(nc.CONF, 0.5, False)
    out = h.postprocess(dev(boxes), dev(conf))
    counts = out[4].cpu().numpy()
    rec, offsets = h.pack_detections(out)
    off = offsets.cpu().numpy(); rec = rec.cpu().numpy()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(counts)])) and counts[[0, 5, 63, 64, 129]].sum() == 0 and counts.sum() > B
    ob, osc, oc = (t.cpu().numpy() for t in out[:3])
    for b in range(B):
        rb, rs, rc = orc.postprocess(boxes[b], conf[b], nc.CONF, 0.5)
        k = counts[b]
        assert k == len(rs) and np.array_equal(ob[b, :k], rb) and np.array_equal(osc[b, :k], rs) and np.array_equal(oc[b, :k], rc)
        q = rec[off[b]:off[b + 1]]
        assert np.array_equal(q[:, :4], ob[b, :k]) and np.array_equal(q[:, 4], osc[b, :k]) and np.array_equal(q[:, 5].astype(np.int32), oc[b, :k])
