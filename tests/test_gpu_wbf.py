"""Weighted box fusion on the device (yn_wbf_merge, the WBF rule of yn_tta / yn_slice, yn_fuse; csrc/kernels_wbf.hip) against the
restatement tests/wbf_oracle.py, bit for bit: boxes, scores, classes, founder rows, votes and the row-to-cluster assignment.  Every call runs
twice on the same handle (scratch reuse).  tests/test_wbf_cpu.py shows on the oracle alone that the lists used here join, drift and cap."""
import os
import sys

import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wbf_cases as wc  # noqa: E402
import wbf_oracle as wo  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)
F32 = np.float32


def _bare(C):
    from yolo_nano_amd import capi
    return capi.Handle(32, C, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=1)


@pytest.fixture(scope="module")
def h3():
    h = _bare(3)
    yield h
    h.close()


@pytest.fixture(scope="module")
def h80():
    h = _bare(80)
    yield h
    h.close()


def _device(h, boxes, scores, cls, C, thr, E):
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (boxes, scores, cls.astype(np.int32))]
    return [a.cpu().numpy() for a in h.wbf_merge(t[0], t[1], t[2], C, thr, E, assign=True)]


def _check(h, boxes, scores, cls, C, thr, E, tag):
    want = wo.wbf(boxes, scores, cls, C, thr, E)
    for run in range(2):
        got = _device(h, boxes, scores, cls, C, thr, E)
        for name, g, w in zip(("boxes", "scores", "cls", "founder", "votes", "assign"), got, want):
            assert wo.same_bits(g, w), (tag, run, name, g[:8], w[:8])
    return want


@pytest.mark.parametrize("E", [1, 22])
@pytest.mark.parametrize("seed", [0, 1])
def test_random_clustered_lists_three_classes(h3, seed, E):
    boxes, scores, cls = wc.clustered(seed)
    want = _check(h3, boxes, scores, cls, 3, 0.55, E, ("clustered", seed, E))
    assert (want[4] >= 2).sum() * 10 >= len(want[4])


@pytest.mark.parametrize("E", [1, 22])
def test_random_clustered_lists_eighty_classes(h80, E):
    boxes, scores, cls = wc.clustered(7, C=80, objects=40, clutter=120)
    want = _check(h80, boxes, scores, cls, 80, 0.55, E, ("clustered80", E))
    assert (want[4] >= 2).sum() * 10 >= len(want[4]) and len(set(want[2])) > 20


@pytest.mark.parametrize("case", wc.EXACT, ids=[c[0] for c in wc.EXACT])
def test_hand_built_cases(h3, case):
    name, rows, thr, E, votes, founders = case
    boxes, scores, cls = wc._rows(rows)
    want = _check(h3, boxes, scores, cls, 3, thr, E, name)
    assert list(want[4]) == votes and list(want[3]) == founders


def test_empty_list_rows_that_are_none_and_a_single_class(h3):
    from yolo_nano_amd import capi
    z = torch.zeros((0, 4), device="cuda")
    out = h3.wbf_merge(z, z[:, 0], z[:, 0].int(), 3, 0.55, 1, assign=True)
    assert [len(o) for o in out] == [0] * 6
    boxes, scores, cls = wc.clustered(4)
    cls = cls.copy(); cls[::5] = -1                              # not rows: in no cluster, assign -1
    want = _check(h3, boxes, scores, cls, 3, 0.55, 3, "holes")
    assert (want[5][::5] == -1).all() and (want[5][cls >= 0] >= 0).all()
    h1 = _bare(1)
    boxes, scores, cls = wc.clustered(6, C=1)
    _check(h1, boxes, scores, cls, 1, 0.55, 2, "one class")
    h1.close()
    b = torch.from_numpy(boxes).cuda(); s = torch.from_numpy(scores).cuda(); c = torch.from_numpy(cls).cuda()
    with pytest.raises(capi.YnError, match="expected is 0"):
        h3.wbf_merge(b, s, c, 3, 0.55, 0)
    with pytest.raises(capi.YnError, match="num_classes is 4, the handle has 3"):
        h3.wbf_merge(b, s, c, 4, 0.55, 1)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert h3.lib.yn_wbf_merge(h3.h, b.data_ptr(), s.data_ptr(), c.data_ptr(), -1, 3, 0.55, 1, b.data_ptr(), s.data_ptr(), c.data_ptr(), None, None, None,
                               cnt.data_ptr()) == 1
    assert "n is -1" in h3.lib.yn_last_error(h3.h).decode()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_cluster_count_straddles_the_lds_limit(h3, delta):
    """K - 1, K and K + 1 clusters in one segment (K = yn_wbf_lds_clusters()), joiners aimed at the last three: with K + 1 one joiner
    updates a cluster that lives in device memory, and every later row is evaluated against it."""
    K = h3.lib.yn_wbf_lds_clusters() + delta
    boxes, scores, cls = wc.straddle(K)
    want = _check(h3, boxes, scores, cls, 3, 0.55, 2, ("straddle", K))
    seg = want[2] == 1
    assert seg.sum() == K and list(want[4][seg][-3:]) == [2, 2, 2]


@pytest.mark.parametrize("C", [3, 80])
def test_without_overlap_wbf_is_the_nms_merge(h3, h80, C):
    h = h3 if C == 3 else h80
    boxes, scores, cls = wc.grid(700, C=C, seed=C)
    t = [torch.from_numpy(a).cuda() for a in (boxes, scores, cls)]
    for run in range(2):
        nb, ns_, nc, ni = [a.cpu().numpy() for a in h.nms_merge(t[0], t[1], t[2], C, 0.55)]
        wb, ws, wcl, wi, wv = [a.cpu().numpy() for a in h.wbf_merge(t[0], t[1], t[2], C, 0.55, 1)]
        assert len(ni) == 700 and wo.same_bits(nb, wb) and wo.same_bits(ns_, ws) and wo.same_bits(nc, wcl) and wo.same_bits(ni, wi) and (wv == 1).all()


# ---- yn_tta / yn_slice / the shims: one small model --------------------------------------------------------------------------------
S, C = 96, 20
SCALES = [64, 96]
CAP_T = 2 * sum(3 * ((s // 8) ** 2 + (s // 16) ** 2 + (s // 32) ** 2) for s in SCALES)
THR = 0.55


def _model(conf, seed_shift=0):
    import yolo_nano_amd
    model = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, trainable=False, conf_thresh=conf, nms_thresh=0.5,
                                   anchor_size=arch.MULTI_ANCHOR_SIZE, backbone="1.0x")
    sd = {k: torch.as_tensor(v) for k, v in weights.make_state_dict("1.0x", C).items()}
    if seed_shift:                                             # a second, different model for the ensemble: the head biases move
        g = torch.Generator().manual_seed(seed_shift)
        sd = {k: (v + 0.05 * torch.randn(v.shape, generator=g) if v.dtype == torch.float32 and k.endswith("bias") else v) for k, v in sd.items()}
    model.load_state_dict(sd, strict=False)
    return model.to("cuda").eval()


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    c.model = _model(0.05)
    c.x = torch.from_numpy(weights.make_input(3, S, seed=4)).cuda()
    c.h = c.model.handle(8)
    yield c


def _records_equal(rec, off, want_rec, want_off, tag):
    off = off.cpu().numpy() if isinstance(off, torch.Tensor) else off
    assert np.array_equal(off, want_off), (tag, off, want_off)
    got = rec[:int(off[-1])].cpu().numpy()
    assert wo.same_bits(got, want_rec), tag


def test_tta_rule(ctx):
    from yolo_nano_amd import capi
    B = 3
    tta = capi.Tta(ctx.h, SCALES, True, max_batch=B, list_capacity=CAP_T)
    tta.infer(ctx.x, THR)
    nrec, noff, ntot = tta.result(total=True)
    nrec = nrec[:ntot].cpu().numpy().copy(); noff = noff.cpu().numpy().copy()
    tta.merge_rule(capi.MERGE_WBF)
    for run in range(2):
        tta.infer(ctx.x, THR)
        rec, off = tta.result()
        lb, ls, lc, cnt, _ = tta.forwards_to_host(B)
        assert (cnt > 0).all()
        wrec, woff = wo.wbf_records(lb, ls, lc, cnt, C, THR, 4)         # the default E: 2 scales x flip = 4 forwards
        _records_equal(rec, off, wrec, woff, ("tta", run))
    assert woff[-1] < ntot or not wo.same_bits(wrec, nrec)       # the rule did something on these lists
    tta.merge_rule(capi.MERGE_WBF, 2)
    tta.infer(ctx.x, THR)
    wrec2, woff2 = wo.wbf_records(lb, ls, lc, cnt, C, THR, 2)
    _records_equal(*tta.result(), wrec2, woff2, "tta E = 2")
    tta.merge_rule(capi.MERGE_NMS)
    tta.infer(ctx.x, THR)
    _records_equal(*tta.result(), nrec, noff, "tta back to NMS")
    with pytest.raises(capi.YnError, match="neither YN_MERGE_NMS"):
        tta.merge_rule(2)
    with pytest.raises(capi.YnError, match="expected is -1"):
        tta.merge_rule(capi.MERGE_WBF, -1)
    tta.close()


def test_slice_rule(ctx):
    from yolo_nano_amd import capi
    from yolo_nano_amd.slicing import tile_table
    shapes = [(150, 200), (120, 96)]
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, shp + (3,), dtype=np.uint8)).cuda() for shp in shapes]
    tiles = tile_table(shapes, S, 0.25, True, S)
    cap = ctx.h.N * int(max((tiles[:, 0] == f).sum() for f in range(2)))
    sl = capi.Slice(ctx.h, 2, cap)
    sl.infer(frames, tiles, MEAN, STD, THR)
    nrec, noff, ntot = sl.result(total=True)
    nrec = nrec[:ntot].cpu().numpy().copy(); noff = noff.cpu().numpy().copy()
    sl.merge_rule(capi.MERGE_WBF)
    for run in range(2):
        sl.infer(frames, tiles, MEAN, STD, THR)
        lb, ls, lc, cnt, _ = sl.lists_to_host()
        wrec, woff = wo.wbf_records(lb, ls, lc, cnt, C, THR, 1)         # the default E of a slice: 1
        _records_equal(*sl.result(), wrec, woff, ("slice", run))
    sl.merge_rule(capi.MERGE_NMS)
    sl.merge(2, THR)
    _records_equal(*sl.result(), nrec, noff, "slice back to NMS")
    sl.close()


def _rec_lists(seed, B, C_, n_lo=20, n_hi=60):
    """B units of random records in yn_pack_detections' layout -> (rec [total, 6] f32, offsets [B + 1] i32)"""
    recs, off = [], [0]
    for b in range(B):
        boxes, scores, cls = wc.clustered(seed + b, C=C_, objects=4, views=8, clutter=10)
        recs.append(np.concatenate([boxes, scores[:, None], cls.astype(F32)[:, None]], 1).astype(F32))
        off.append(off[-1] + len(boxes))
    return np.concatenate(recs), np.asarray(off, np.int32)


def test_fuse_object(h3):
    from yolo_nano_amd import capi
    B, cap = 2, 256
    ra, oa = _rec_lists(10, B, 3)
    rb, ob = _rec_lists(20, B, 3)
    fu = capi.Fuse(h3, max_units=B, list_capacity=cap)
    da, db = [(torch.from_numpy(r).cuda(), torch.from_numpy(o).cuda()) for r, o in ((ra, oa), (rb, ob))]
    w = F32(0.7)
    for run in range(2):
        fu.open(B)
        fu.append(da[0], da[1], 1.0)
        fu.append(db[0], db[1], float(w))
        lb, ls, lc, cnt = fu.lists_to_host()
        for b in range(B):
            ua, ub = ra[oa[b]:oa[b + 1]], rb[ob[b]:ob[b + 1]]
            m = len(ua) + len(ub)
            assert cnt[b] == m
            assert wo.same_bits(lb[b, :m], np.concatenate([ua[:, :4], ub[:, :4]]))
            assert wo.same_bits(ls[b, :m], np.concatenate([ua[:, 4], (ub[:, 4] * w).astype(F32)]))      # 1.0f copies the bits, w is one multiply
            assert np.array_equal(lc[b, :m], np.concatenate([ua[:, 5], ub[:, 5]]).astype(np.int32)) and (lc[b, m:] == -1).all()
        fu.merge(B, capi.MERGE_WBF, THR)                          # expected 0: the two appends
        wrec, woff = wo.wbf_records(lb, ls, lc, cnt, 3, THR, 2)
        _records_equal(*fu.result(), wrec, woff, ("fuse", run))
        assert woff[-1] < cnt.sum()
    # the NMS rule gives yn_nms_merge's bits
    fu.merge(B, capi.MERGE_NMS, THR)
    rec, off = fu.result()
    off = off.cpu().numpy()
    for b in range(B):
        m = int(cnt[b])
        nb, ns_, nc, _ = [a.cpu().numpy() for a in h3.nms_merge(torch.from_numpy(lb[b, :m]).cuda(), torch.from_numpy(ls[b, :m]).cuda(),
                                                                torch.from_numpy(lc[b, :m]).cuda(), 3, THR)]
        got = rec[off[b]:off[b + 1]].cpu().numpy()
        assert wo.same_bits(got[:, :4], nb) and wo.same_bits(got[:, 4], ns_) and np.array_equal(got[:, 5], nc.astype(F32))
    # refusals: capacity, a bad class, the range mark
    small = capi.Fuse(h3, max_units=B, list_capacity=int(cnt.max()) - 1)
    small.open(B)
    small.append(da[0], da[1]); small.append(db[0], db[1])
    with pytest.raises(capi.YnError, match=r"the merge list of unit %d needs %d rows" % (int(np.argmax(cnt >= cnt.max())), int(cnt.max()))):
        small.merge(B)
    small.close()
    bad = ra.copy(); bad[oa[1] + 2, 5] = 3.0; bad[oa[1] + 3, 5] = 0.5          # unit 1: a class past C - 1 and one that is no integer
    fu.open(B)
    fu.append(torch.from_numpy(bad).cuda(), da[1])
    with pytest.raises(capi.YnError, match=r"unit 1 was appended 2 rows whose class is not an integer in 0..2"):
        fu.merge(B)
    marked = oa.copy(); marked[B] = -1 - marked[B]
    fu.open(B)
    fu.append(da[0], torch.from_numpy(marked).cuda())
    with pytest.raises(capi.YnRangeError):
        fu.merge(B)
    fu.open(B)                                                  # and the object still works
    fu.append(da[0], da[1])
    fu.merge(B, capi.MERGE_WBF, THR, 1)
    lb, ls, lc, cnt = fu.lists_to_host()
    _records_equal(*fu.result(), *wo.wbf_records(lb, ls, lc, cnt, 3, THR, 1), "fuse again")
    fu.close()


def test_shims_agree_with_the_oracle_on_their_lists(ctx):
    import yolo_nano_amd
    from yolo_nano_amd import evaluate
    from yolo_nano_amd.fusion import Ensemble, weighted_boxes_fusion
    model = ctx.model

    def triples_equal(trip, rec, off, tag):
        for b in range(len(off) - 1):
            q = rec[off[b]:off[b + 1]]
            assert wo.same_bits(trip[b][0], q[:, :4]) and wo.same_bits(trip[b][1], q[:, 4]) and np.array_equal(trip[b][2], q[:, 5].astype(np.int64)), tag

    tta = yolo_nano_amd.TestTimeAugmentation(num_classes=C, nms_thresh=THR, scale_range=[64, 96, 32], merge="wbf")
    tta.list_capacity = CAP_T
    trip = tta.batch(ctx.x, model)
    lb, ls, lc, cnt, _ = tta._tta.forwards_to_host(3)
    triples_equal(trip, *wo.wbf_records(lb, ls, lc, cnt, C, THR, 4), "tta shim")
    with pytest.raises(ValueError, match="'nms' or 'wbf'"):
        yolo_nano_amd.TestTimeAugmentation(num_classes=C, merge="soft")
    # evaluate(..., test_aug=tta) runs with the WBF rule: the same APs as the evaluator fed with batch()'s triples
    from yolo_nano_amd import VOCEval
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, (S, S, 3), dtype=np.uint8) for _ in range(3)]
    annots = [np.array([[5, 5, 60, 70, 1, 0], [30, 20, 90, 80, 7, 0]], np.int32) for _ in images]
    aps, mAP = evaluate(model, images, annots, batch=3, test_aug=tta)
    assert len(aps) == C and tta._tta.n == 3
    model.set_grid(S)

    sl = yolo_nano_amd.SlicedInference(tile=S, overlap=0.25, nms_thresh=THR, list_capacity=8 * model.handle(8).N, merge="wbf", expected=2)
    sl.chunk = 8
    frames = [rng.integers(0, 256, shp + (3,), dtype=np.uint8) for shp in ((150, 200), (120, 96))]
    trip = sl.batch(frames, model)
    lb, ls, lc, cnt, _ = sl._obj.lists_to_host()
    triples_equal(trip, *wo.wbf_records(lb, ls, lc, cnt, C, THR, 2), "slice shim")

    m2 = _model(0.05, seed_shift=11)
    ens = Ensemble([model, m2], iou_thr=THR, weights=[1.0, 0.5])
    ens.list_capacity = 2 * model.handle(8).N
    trip = ens.batch(ctx.x)
    lb, ls, lc, cnt = ens._obj.lists_to_host()
    assert (cnt > 0).all()
    wrec, woff = wo.wbf_records(lb, ls, lc, cnt, C, THR, 2)
    triples_equal(trip, wrec, woff, "ensemble")
    # the lists are the two models' own detections, the second model's scores halved
    for mi, (m, w) in enumerate(((model, 1.0), (m2, 0.5))):
        own = m.handle(8).detections_to_host(m.handle(8).infer(ctx.x))
        for b in range(3):
            k = len(own[b][1])
            lo = 0 if mi == 0 else int(cnt[b]) - k
            assert wo.same_bits(lb[b, lo:lo + k], own[b][0]) and wo.same_bits(ls[b, lo:lo + k], (own[b][1] * F32(w)).astype(F32))

    # the numpy-in, numpy-out call on one image: model lists as ensemble_boxes callers pass them
    b0 = int(cnt[0])
    k0 = len(model.handle(8).detections_to_host(model.handle(8).infer(ctx.x))[0][1])
    bl = [lb[0, :k0], lb[0, k0:b0]]; sc = [ls[0, :k0], ls[0, k0:b0]]; la = [lc[0, :k0], lc[0, k0:b0]]
    fb, fs, fl = weighted_boxes_fusion(bl, sc, la, iou_thr=THR, num_classes=C)
    q = wrec[woff[0]:woff[1]]
    assert wo.same_bits(fb, q[:, :4]) and wo.same_bits(fs, q[:, 4]) and np.array_equal(fl, q[:, 5].astype(np.int64))
    fb2, fs2, _ = weighted_boxes_fusion(bl, sc, la, iou_thr=THR, weights=[1.0, 0.5], expected=1)
    want = wo.wbf(lb[0, :b0], np.concatenate([sc[0], (sc[1] * F32(0.5)).astype(F32)]), lc[0, :b0], int(lc[0, :b0].max()) + 1, THR, 1)
    assert wo.same_bits(fb2, want[0]) and wo.same_bits(fs2, want[1])
