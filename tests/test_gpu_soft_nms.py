"""Soft-NMS on the device (yn_soft_nms_merge, yn_soft_nms inside yn_infer / yn_postprocess, the soft suppression of yn_tta / yn_slice /
yn_fuse; csrc/kernels_soft.hip) against the restatement tests/soft_nms_oracle.py, bit for bit: boxes, scores, classes, rows and counts.
Every merge call runs twice on the same handle (scratch reuse).  tests/test_soft_nms_cpu.py shows on the oracle alone that the lists used
here decay, drop and keep rows the NMS would not."""
import os
import sys

import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nms_stage_oracle as ns  # noqa: E402
import soft_nms_cases as sc  # noqa: E402
import soft_nms_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)
F32 = np.float32
NAMES = ("boxes", "scores", "cls", "index")


def _bare(C, **kw):
    from yolo_nano_amd import capi
    return capi.Handle(32, C, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=1, **kw)


@pytest.fixture(scope="module")
def h3():
    h = _bare(3)
    yield h
    h.close()


def _cuda(boxes, scores, cls):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (boxes.reshape(-1, 4), scores, cls.astype(np.int32))]


def _device(h, boxes, scores, cls, C, method, thr, sigma, floor):
    t = _cuda(boxes, scores, cls)
    return [a.cpu().numpy() for a in h.soft_nms_merge(t[0], t[1], t[2], C, method, thr, sigma, floor)]


def _check(h, boxes, scores, cls, C, method, thr, sigma, floor, tag, trace=None):
    want = so.soft_nms(boxes, scores, cls, C, method, thr, sigma, floor, trace)
    for run in range(2):
        got = _device(h, boxes, scores, cls, C, method, thr, sigma, floor)
        assert len(got[3]) == len(want[3]), (tag, run, len(got[3]), len(want[3]))
        for name, g, w in zip(NAMES, got, want):
            assert so.same_bits(g, w), (tag, run, name, g[:8], w[:8])
    return want


# ---- the exp on its own ----------------------------------------------------------------------------------------------------------------
def test_exp_equals_the_restatement_bit_for_bit(h3):
    rng = np.random.default_rng(0)
    trace = []
    for seed in (0, 1, 2):
        so.soft_nms(*sc.clustered(seed), 3, so.GAUSSIAN, 0.5, 0.5, 0.05, trace)
    for case in sc.EXACT:
        boxes, scores, cls = sc._rows(case[1])
        so.soft_nms(boxes, scores, cls, 3, so.GAUSSIAN, 0.5, case[4], 0.0, trace)
    o = np.concatenate(trace).astype(F32)
    with np.errstate(all="ignore"):
        args = np.concatenate([-((o * o).astype(F32) / F32(s)).astype(F32) for s in (0.5, 0.1)])      # every argument the other cases produce
    edge = np.array([0.0, -0.0, -87.0, -87.0001, np.nan, -np.inf, -88.0, -86.99999, -1e-30, -1e-45, -0.34657359, -0.6931472], F32)
    x = np.concatenate([rng.uniform(-88.0, 0.0, 700_000), np.linspace(-88.0, 0.0, 300_001), -np.exp(rng.uniform(-60.0, 0.0, 50_000)), args, edge]).astype(F32)
    assert len(args) > 1000 and np.isnan(args).any()
    got = h3.soft_exp(torch.from_numpy(x).cuda()).cpu().numpy()
    want = so.E(x)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    bad = bad[~(np.isnan(got[bad]) & np.isnan(want[bad]))]       # (a NaN is a NaN: its payload is not part of the claim)
    assert len(bad) == 0, (len(bad), x[bad[:8]], got[bad[:8]], want[bad[:8]])
    e = h3.soft_exp(torch.from_numpy(edge).cuda()).cpu().numpy()
    assert e[0] == 1 and e[1] == 1 and so.same_bits(e[2], F32(1.6458115e-38)) and so.same_bits(e[3], F32(0.0)) and np.isnan(e[4]) and e[5] == 0 and e[6] == 0
    assert len(h3.soft_exp(torch.zeros(0, device="cuda"))) == 0


# ---- yn_soft_nms_merge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.EXACT, ids=[c[0] for c in sc.EXACT])
def test_hand_built_cases(h3, case):
    name, rows, method, thr, sigma, floor, kept, scores = case
    boxes, score, cls = sc._rows(rows)
    want = _check(h3, boxes, score, cls, 3, method, thr, sigma, floor, name)
    assert list(want[3]) == kept
    for m in sc.METHODS:                                       # and under the other methods and another floor, whatever they give
        for fl in (0.0, 0.3):
            _check(h3, boxes, score, cls, 3, m, thr, sigma, fl, (name, m, fl))


@pytest.mark.parametrize("floor", [0.05, 0.3])
@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_clustered_lists(h3, seed, method, floor):
    boxes, scores, cls = sc.clustered(seed)
    want = _check(h3, boxes, scores, cls, 3, method, 0.5, 0.5, floor, ("clustered", seed, method, floor))
    assert 0 < len(want[3]) < len(boxes)
    if method != so.HARD and floor == 0.05:
        assert int((want[1] != scores[want[3]]).sum()) >= 15


def test_eighty_classes_rows_that_are_none_and_a_single_class():
    h80 = _bare(80)
    boxes, scores, cls = sc.clustered(7, C=80, objects=40, clutter=120)
    cls = cls.copy(); cls[::7] = -1                              # not rows
    for method in sc.METHODS:
        want = _check(h80, boxes, scores, cls, 80, method, 0.5, 0.5, 0.05, ("clustered80", method))
        assert len(set(want[2])) > 20 and not (set(want[3]) & set(range(0, len(cls), 7)))
    h80.close()
    h1 = _bare(1)
    boxes, scores, cls = sc.clustered(6, C=1)
    for method in sc.METHODS:
        _check(h1, boxes, scores, cls, 1, method, 0.4, 0.3, 0.1, ("one class", method))
    h1.close()


def test_the_two_identities_on_the_device(h3):
    for seed in (0, 1):
        boxes, scores, cls = sc.clustered(seed)
        t = _cuda(boxes, scores, cls)
        for run in range(2):
            nms = [a.cpu().numpy() for a in h3.nms_merge(t[0], t[1], t[2], 3, 0.5)]
            hard = [a.cpu().numpy() for a in h3.soft_nms_merge(t[0], t[1], t[2], 3, "hard", 0.5, 0.5, 0.0)]
            assert len(nms[3]) < len(boxes) and all(so.same_bits(a, b) for a, b in zip(nms, hard)), (seed, run)
    h80 = _bare(80)
    for h, C in ((h3, 3), (h80, 80)):
        boxes, scores, cls = sc.grid(700, C=C, seed=C)
        t = _cuda(boxes, scores, cls)
        for run in range(2):
            nms = [a.cpu().numpy() for a in h.nms_merge(t[0], t[1], t[2], C, 0.5)]
            lin = [a.cpu().numpy() for a in h.soft_nms_merge(t[0], t[1], t[2], C, "linear", 0.5, 0.5, 0.0)]
            assert len(nms[3]) == 700 and all(so.same_bits(a, b) for a, b in zip(nms, lin)), (C, run)
    h80.close()


@pytest.mark.parametrize("which", ["L-1", "L", "L+1", "2L+1"])
def test_segment_length_straddles_the_lds_limit(h3, which):
    """Segments of L - 1, L, L + 1 and 2 L + 1 rows (L = yn_soft_lds_rows()): past L a row's score lives in device memory, its box stays
    in the sorted boxes; with 2 L + 1 rows a lane owns several such rows."""
    L = h3.lib.yn_soft_lds_rows()
    n = {"L-1": L - 1, "L": L, "L+1": L + 1, "2L+1": 2 * L + 1}[which]
    boxes, scores, cls = sc.straddle(n)
    for method in (so.LINEAR, so.GAUSSIAN) if which != "L-1" else sc.METHODS:
        want = _check(h3, boxes, scores, cls, 3, method, 0.5, 0.5, 0.1, ("straddle", n, method))
        seg = want[2] == 1
        decayed = int((want[1][seg] != scores[want[3][seg]]).sum())
        assert (want[2] == 0).sum() == 5 and n // 2 < seg.sum() <= n, seg.sum()
        assert decayed >= n // 16 if method != so.HARD else seg.sum() < n - n // 16, (seg.sum(), decayed)


def test_refusals(h3):
    from yolo_nano_amd import capi
    boxes, scores, cls = sc.clustered(0)
    b, s, c = _cuda(boxes, scores, cls)
    z = torch.zeros((0, 4), device="cuda")
    assert [len(o) for o in h3.soft_nms_merge(z, z[:, 0], z[:, 0].int(), 3, "gaussian")] == [0] * 4
    for bad in (0, 4, -1):
        with pytest.raises(capi.YnError, match=r"yn_soft_nms_merge: method %d is not YN_SOFT_HARD" % bad):
            h3.soft_nms_merge(b, s, c, 3, bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(capi.YnError, match="yn_soft_nms_merge: sigma is .* positive and finite"):
            h3.soft_nms_merge(b, s, c, 3, "gaussian", 0.5, bad)
    for bad in (-0.001, float("inf"), float("nan")):
        with pytest.raises(capi.YnError, match="yn_soft_nms_merge: score_floor is .* 0 or more and finite"):
            h3.soft_nms_merge(b, s, c, 3, "gaussian", 0.5, 0.5, bad)
    with pytest.raises(capi.YnError, match="num_classes is 4, the handle has 3"):
        h3.soft_nms_merge(b, s, c, 4, "linear")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert h3.lib.yn_soft_nms_merge(h3.h, b.data_ptr(), s.data_ptr(), c.data_ptr(), -1, 3, 2, 0.5, 0.5, 0.0, b.data_ptr(), s.data_ptr(), c.data_ptr(), None,
                                    cnt.data_ptr()) == 1
    assert "n is -1" in h3.lib.yn_last_error(h3.h).decode()
    with pytest.raises(capi.YnError, match="yn_soft_nms: method 7 is not YN_SOFT_OFF"):
        h3.soft_nms(7)
    with pytest.raises(capi.YnError, match="yn_soft_nms: sigma is"):
        h3.soft_nms("linear", sigma=0.0)
    with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
        h3.soft_nms("soft")
    # out_index may be NULL: the other outputs are the same
    want = so.soft_nms(boxes, scores, cls, 3, so.LINEAR, 0.5, 0.5, 0.05)
    ob = torch.empty_like(b); osc = torch.empty_like(s); oc = torch.empty_like(c)
    assert h3.lib.yn_soft_nms_merge(h3.h, b.data_ptr(), s.data_ptr(), c.data_ptr(), len(boxes), 3, 2, 0.5, 0.5, 0.05, ob.data_ptr(), osc.data_ptr(), oc.data_ptr(),
                                    None, cnt.data_ptr()) == 0
    k = int(cnt.item())
    assert k == len(want[3]) and so.same_bits(ob[:k].cpu().numpy(), want[0]) and so.same_bits(osc[:k].cpu().numpy(), want[1])


# ---- yn_postprocess ------------------------------------------------------------------------------------------------------------------------
def _kept(out):
    boxes, scores, cls, index, count = [t.cpu().numpy() for t in out]
    return [(boxes[b, :count[b]].copy(), scores[b, :count[b]].copy(), cls[b, :count[b]].copy(), index[b, :count[b]].copy()) for b in range(len(count))]


def test_postprocess_with_the_soft_suppression():
    from yolo_nano_amd import capi
    B, N, C, conf, thr = 2, 300, 3, 0.2, 0.45
    h = _bare(C, conf_thresh=conf, nms_thresh=thr)
    rng = np.random.default_rng(11)
    local = np.zeros((B, N, 4), F32); confs = np.zeros((B, N, C), F32)
    for b in range(B):
        bx, s, c = sc.clustered(20 + b, C=C, objects=14, views=22, clutter=40)
        n = min(len(bx), N)
        local[b, :n] = bx[:n]
        confs[b, :n] = (rng.random((n, C)) * 0.15).astype(F32)
        confs[b, np.arange(n), c[:n]] = s[:n]
        local[b, n:] = bx[0]; confs[b, n:] = F32(0.01)          # below conf_thresh: no candidates
    tl, tc = torch.from_numpy(local).cuda(), torch.from_numpy(confs).cuda()
    before = _kept(h.postprocess(tl, tc))
    for b in range(B):                                          # OFF is the NMS chain
        cls, score = ns.candidates(confs[b], conf)
        assert all(so.same_bits(g, w) for g, w in zip(before[b], so.nms_merge(local[b], score, cls, C, thr)))
    for method, sigma, floor in (("linear", 0.5, conf), ("gaussian", 0.5, conf), ("gaussian", 0.2, 0.3), ("hard", 0.5, 0.0)):
        h.soft_nms(method, sigma, floor)
        for run in range(2):
            got = _kept(h.postprocess(tl, tc))
            for b in range(B):
                cls, score = ns.candidates(confs[b], conf)
                want = so.soft_nms(local[b], score, cls, C, so.METHODS[method], thr, sigma, floor)
                assert len(want[3]) > 20 and all(so.same_bits(g, w) for g, w in zip(got[b], want)), (method, run, b)
                if method == "hard":
                    assert all(so.same_bits(g, w) for g, w in zip(got[b], before[b]))
                else:
                    assert len(got[b][3]) != len(before[b][3]) or not so.same_bits(got[b][1], before[b][1])
    h.set_thresholds(conf, thr, True)
    with pytest.raises(capi.YnError, match="yn_postprocess: Soft-NMS .* has no DIoU form"):
        h.postprocess(tl, tc)
    h.set_thresholds(conf, thr, False)
    h.soft_nms(None)
    after = _kept(h.postprocess(tl, tc))
    assert all(so.same_bits(g, w) for b in range(B) for g, w in zip(after[b], before[b]))
    h.close()


# ---- yn_infer / yn_tta / yn_slice / yn_fuse / the shims: one small model --------------------------------------------------------------------------
S, C = 96, 20
SCALES = [64, 96]
CAP_T = 2 * sum(3 * ((s // 8) ** 2 + (s // 16) ** 2 + (s // 32) ** 2) for s in SCALES)
THR = 0.5
SOFT = ("gaussian", 0.5, 0.08)


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
    assert so.same_bits(got, want_rec), tag


def _soft_records(lb, ls, lc, cnt, soft=SOFT, thr=THR):
    return so.soft_records(lb, ls, lc, cnt, C, so.METHODS[soft[0]], thr, soft[1], soft[2])


def test_infer_eager_and_graph(ctx):
    from yolo_nano_amd import capi
    torch.cuda.synchronize()
    st = torch.cuda.Stream()                                    # the handle is made on a stream of the test's own: the default stream cannot be captured
    with torch.cuda.stream(st):
        h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, "1.0x", conf_thresh=0.05, nms_thresh=0.5, max_batch=2)
        h.load_state_dict(weights.make_state_dict("1.0x", C))
        h.fold_bn()
        _infer_eager_and_graph(capi, h, ctx.x[:2].contiguous())
        h.close()
    torch.cuda.synchronize()


def _infer_eager_and_graph(capi, h, x):
    before = _kept(h.infer(x))
    assert all(len(k[3]) > 0 for k in before)
    try:
        h.soft_nms("linear", 0.5, 0.05)
        eager = _kept(h.infer(x))
        assert any(len(e[3]) != len(b[3]) or not so.same_bits(e[1], b[1]) for e, b in zip(eager, before))
        out = h.alloc_outputs(2)
        h.use_graph(True)
        try:
            for run in range(3):                                # captured, then replayed
                for t in out[:4]:
                    t.zero_()
                got = _kept(h.infer(x, out=out))
                assert all(so.same_bits(g, w) for b in range(2) for g, w in zip(got[b], eager[b])), run
            h.soft_nms("gaussian", 0.5, 0.05)                   # a change drops the captured graphs
            gauss = _kept(h.infer(x, out=out))
            h.use_graph(False)
            assert all(so.same_bits(g, w) for b in range(2) for g, w in zip(gauss[b], _kept(h.infer(x))[b]))
            assert any(not so.same_bits(g[1], e[1]) for g, e in zip(gauss, eager))
            h.use_graph(True)
            h.soft_nms(None)
            off = _kept(h.infer(x, out=out))
            assert all(so.same_bits(g, w) for b in range(2) for g, w in zip(off[b], before[b]))
        finally:
            h.use_graph(False)
        h.soft_nms("linear", 0.5, 0.05)
        h.set_thresholds(0.05, 0.5, True)
        with pytest.raises(capi.YnError, match="yn_infer: Soft-NMS .* has no DIoU form"):
            h.infer(x)
    finally:
        h.set_thresholds(0.05, 0.5, False)
        h.soft_nms(None)
    after = _kept(h.infer(x))
    assert all(so.same_bits(g, w) for b in range(2) for g, w in zip(after[b], before[b]))


def test_tta_soft(ctx):
    from yolo_nano_amd import capi
    B = 3
    tta = capi.Tta(ctx.h, SCALES, True, max_batch=B, list_capacity=CAP_T)
    tta.infer(ctx.x, THR)
    nrec, noff, ntot = tta.result(total=True)
    nrec = nrec[:ntot].cpu().numpy().copy(); noff = noff.cpu().numpy().copy()
    tta.merge_soft(*SOFT)
    for run in range(2):
        tta.infer(ctx.x, THR)
        rec, off = tta.result()
        lb, ls, lc, cnt, _ = tta.forwards_to_host(B)
        assert (cnt > 0).all()
        wrec, woff = _soft_records(lb, ls, lc, cnt)
        _records_equal(rec, off, wrec, woff, ("tta", run))
    assert woff[-1] != ntot or not so.same_bits(wrec, nrec)      # the suppression did something on these lists
    # a soft setting under the WBF rule is kept but unused: the WBF records
    import wbf_oracle as wo
    tta.merge_rule(capi.MERGE_WBF)
    tta.infer(ctx.x, THR)
    _records_equal(*tta.result(), *wo.wbf_records(lb, ls, lc, cnt, C, THR, 4), "tta WBF with a soft setting")
    tta.merge_rule(capi.MERGE_NMS)
    tta.infer(ctx.x, THR)
    _records_equal(*tta.result(), wrec, woff, "tta soft again")
    tta.merge_soft(None)
    tta.infer(ctx.x, THR)
    _records_equal(*tta.result(), nrec, noff, "tta back to NMS")
    with pytest.raises(capi.YnError, match="yn_merge_soft_tta: method 4 is not YN_SOFT_OFF"):
        tta.merge_soft(4)
    with pytest.raises(capi.YnError, match="yn_merge_soft_tta: score_floor is -1"):
        tta.merge_soft("linear", 0.5, -1.0)
    with pytest.raises(capi.YnError, match="neither YN_MERGE_NMS"):
        tta.merge_rule(2)
    tta.close()


def test_slice_soft(ctx):
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
    soft = ("linear", 0.5, 0.06)
    sl.merge_soft(*soft)
    for run in range(2):
        sl.infer(frames, tiles, MEAN, STD, THR)
        lb, ls, lc, cnt, _ = sl.lists_to_host()
        wrec, woff = _soft_records(lb, ls, lc, cnt, soft)
        _records_equal(*sl.result(), wrec, woff, ("slice", run))
    assert woff[-1] != ntot or not so.same_bits(wrec, nrec)
    import wbf_oracle as wo
    sl.merge_rule(capi.MERGE_WBF)
    sl.merge(2, THR)
    _records_equal(*sl.result(), *wo.wbf_records(lb, ls, lc, cnt, C, THR, 1), "slice WBF with a soft setting")
    sl.merge_rule(capi.MERGE_NMS)
    sl.merge_soft(None)
    sl.merge(2, THR)
    _records_equal(*sl.result(), nrec, noff, "slice back to NMS")
    sl.close()


def test_fuse_soft(h3):
    from yolo_nano_amd import capi
    import wbf_oracle as wo
    B, cap = 2, 256
    recs, offs = [], []
    for seed in (10, 20):
        r, o = [], [0]
        for b in range(B):
            boxes, scores, cls = sc.clustered(seed + b, C=3, objects=4, views=8, clutter=10)
            r.append(np.concatenate([boxes, scores[:, None], cls.astype(F32)[:, None]], 1).astype(F32))
            o.append(o[-1] + len(boxes))
        recs.append(torch.from_numpy(np.concatenate(r)).cuda()); offs.append(torch.from_numpy(np.asarray(o, np.int32)).cuda())
    fu = capi.Fuse(h3, max_units=B, list_capacity=cap)

    def fill():
        fu.open(B)
        fu.append(recs[0], offs[0], 1.0)
        fu.append(recs[1], offs[1], 0.7)
    fill()
    fu.merge(B, capi.MERGE_NMS, THR)
    nrec, noff, ntot = fu.result(total=True)
    nrec = nrec[:ntot].cpu().numpy().copy(); noff = noff.cpu().numpy().copy()
    lb, ls, lc, cnt = fu.lists_to_host()
    for soft in (("gaussian", 0.3, 0.1), ("linear", 0.5, 0.1), ("hard", 0.5, 0.0)):
        fu.merge_soft(*soft)
        for run in range(2):
            fill()
            fu.merge(B, capi.MERGE_NMS, THR)
            wrec, woff = so.soft_records(lb, ls, lc, cnt, 3, so.METHODS[soft[0]], THR, soft[1], soft[2])
            _records_equal(*fu.result(), wrec, woff, ("fuse", soft, run))
        assert (soft[0] == "hard") == (np.array_equal(woff, noff) and so.same_bits(wrec, nrec))
        fu.merge(B, capi.MERGE_WBF, THR)
        _records_equal(*fu.result(), *wo.wbf_records(lb, ls, lc, cnt, 3, THR, 2), "fuse WBF with a soft setting")
    with pytest.raises(capi.YnError, match="neither YN_MERGE_NMS"):
        fu.merge(B, 2, THR)
    fu.merge_soft(None)
    fu.merge(B, capi.MERGE_NMS, THR)
    _records_equal(*fu.result(), nrec, noff, "fuse back to NMS")
    fu.close()


def test_shims_agree_with_the_oracle_on_their_lists(ctx):
    import yolo_nano_amd
    from yolo_nano_amd import evaluate
    from yolo_nano_amd.fusion import Ensemble, soft_nms
    model = ctx.model

    def triples_equal(trip, rec, off, tag):
        for b in range(len(off) - 1):
            q = rec[off[b]:off[b + 1]]
            assert so.same_bits(trip[b][0], q[:, :4]) and so.same_bits(trip[b][1], q[:, 4]) and np.array_equal(trip[b][2], q[:, 5].astype(np.int64)), tag

    # score_floor None = the model's conf_thresh (0.05)
    tta = yolo_nano_amd.TestTimeAugmentation(num_classes=C, nms_thresh=THR, scale_range=[64, 96, 32], soft="gaussian", sigma=0.4)
    tta.list_capacity = CAP_T
    trip = tta.batch(ctx.x, model)
    lb, ls, lc, cnt, _ = tta._tta.forwards_to_host(3)
    wrec, woff = _soft_records(lb, ls, lc, cnt, ("gaussian", 0.4, 0.05))
    triples_equal(trip, wrec, woff, "tta shim")
    rec, off = tta.records(ctx.x, model)
    _records_equal(rec, off, wrec, woff, "tta records")
    for cls_, kw in ((yolo_nano_amd.TestTimeAugmentation, dict(num_classes=C)), (yolo_nano_amd.SlicedInference, dict(tile=S)), (Ensemble, dict(models=[model]))):
        with pytest.raises(ValueError, match="soft='linear' cannot be combined with merge='wbf'"):
            cls_(merge="wbf", soft="linear", **kw)
        with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
            cls_(merge="nms", soft="soft", **kw)
    # evaluate(..., test_aug=tta) runs with the soft suppression, unchanged
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, (S, S, 3), dtype=np.uint8) for _ in range(3)]
    annots = [np.array([[5, 5, 60, 70, 1, 0], [30, 20, 90, 80, 7, 0]], np.int32) for _ in images]
    aps, mAP = evaluate(model, images, annots, batch=3, test_aug=tta)
    assert len(aps) == C and tta._tta.n == 3
    model.set_grid(S)
    # __call__ (the reference's loop over image 0) ends in yn_soft_nms_merge
    tta1 = yolo_nano_amd.TestTimeAugmentation(num_classes=C, nms_thresh=THR, scale_range=[64, 96, 32], soft="linear", score_floor=0.07)
    tta0 = yolo_nano_amd.TestTimeAugmentation(num_classes=C, nms_thresh=2.0, scale_range=[64, 96, 32])      # thr 2: the concatenated lists, all kept
    ab, as_, al = tta0(ctx.x[:1], model)
    sb, ss, sl_ = tta1(ctx.x[:1], model)
    model.set_grid(S)
    want = so.soft_nms(ab, as_, al, C, so.LINEAR, THR, 0.5, 0.07)
    assert len(ab) > len(sb) > 0 and so.same_bits(sb, want[0]) and so.same_bits(ss, want[1]) and np.array_equal(sl_, want[2].astype(np.int64))

    sl = yolo_nano_amd.SlicedInference(tile=S, overlap=0.25, nms_thresh=THR, list_capacity=8 * model.handle(8).N, soft="linear", score_floor=0.06)
    sl.chunk = 8
    frames = [rng.integers(0, 256, shp + (3,), dtype=np.uint8) for shp in ((150, 200), (120, 96))]
    trip = sl.batch(frames, model)
    lb, ls, lc, cnt, _ = sl._obj.lists_to_host()
    triples_equal(trip, *_soft_records(lb, ls, lc, cnt, ("linear", 0.5, 0.06)), "slice shim")

    m2 = _model(0.05, seed_shift=11)
    ens = Ensemble([model, m2], iou_thr=THR, merge="nms", weights=[1.0, 0.5], soft="gaussian", sigma=0.5, score_floor=0.04)
    ens.list_capacity = 2 * model.handle(8).N
    trip = ens.batch(ctx.x)
    lb, ls, lc, cnt = ens._obj.lists_to_host()
    assert (cnt > 0).all()
    wrec, woff = _soft_records(lb, ls, lc, cnt, ("gaussian", 0.5, 0.04))
    triples_equal(trip, wrec, woff, "ensemble")

    # the numpy-in, numpy-out call on one image
    b0 = int(cnt[0])
    fb, fs, fl = soft_nms(lb[0, :b0], ls[0, :b0], lc[0, :b0], method="gaussian", iou_thr=THR, sigma=0.5, score_floor=0.04, num_classes=C)
    q = wrec[woff[0]:woff[1]]
    assert so.same_bits(fb, q[:, :4]) and so.same_bits(fs, q[:, 4]) and np.array_equal(fl, q[:, 5].astype(np.int64))
    fb, fs, fl = soft_nms(lb[0, :b0], ls[0, :b0], lc[0, :b0], method="linear", iou_thr=THR)
    want = so.soft_nms(lb[0, :b0], ls[0, :b0], lc[0, :b0], int(lc[0, :b0].max()) + 1, so.LINEAR, THR, 0.5, 0.001)
    assert so.same_bits(fb, want[0]) and so.same_bits(fs, want[1]) and fl.dtype == np.int64
    with pytest.raises(ValueError, match="'hard', 'linear' or 'gaussian'"):
        soft_nms(lb[0, :b0], ls[0, :b0], lc[0, :b0], method="soft")
    e = soft_nms(np.zeros((0, 4)), np.zeros(0), np.zeros(0))
    assert [len(a) for a in e] == [0, 0, 0]
    # the model's own forward with set_soft_nms: the handle's yn_soft_nms at the model's conf_thresh, and off again
    base = model(ctx.x[:1])
    model.set_soft_nms("gaussian", sigma=0.5)
    soft_out = model(ctx.x[:1])
    h = model.handle(8)
    want = _kept(h.infer(ctx.x[:1]))[0]
    assert so.same_bits(soft_out[0], want[0]) and so.same_bits(soft_out[1], want[1]) and (soft_out[1] > F32(0.05)).all()
    assert len(soft_out[1]) != len(base[1]) or not so.same_bits(soft_out[1], base[1])
    model.set_soft_nms(None)
    again = model(ctx.x[:1])
    assert all(so.same_bits(a, b) for a, b in zip(again, base))
