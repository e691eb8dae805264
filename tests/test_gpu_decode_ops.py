"""The score / box decode front ends of csrc/kernels_post.hip on their own against float64: decode_kernel<FULL, KMAX> (yn_score_full, yn_op_decode_cand),
head_decode_kernel / head_decode_group_kernel / head_tail_group_kernel (yn_op_head_tail, the stretch of yn_infer's forward behind the heads' layer .1)
and argmax_cand_kernel (yn_postprocess).  tests/decode_cases.py holds the case tables, the float64 reference, the restated launch rules and the regimes;
tests/test_decode_cases_cpu.py proves without a GPU that the tables reach every instantiation and every regime.  Every case asserts the symbol of the
kernel that ran (the profile record of the call).

Two kinds of data per case: RANDOM normal logits, objectness on both sides of the threshold (conf 0.25), and STEERED exact binary fractions placed on
the fast / general / skip decisions of a wavefront, exact and near ties, -inf logits, a NaN objectness, saturated and overflowing box logits (conf 0.001).

Bars.  all_class, all_bbox, scores and boxes stay inside f64_bar.bar, 4 * e32 + 4 ulp, e32 = max |float32 numpy evaluation - float64| of the same
formulas.  No slack is added for exp_le0 (exp(x), x = logit - max <= 0, as v_exp_f32(x * log2 e)): the rounding of the product is a relative
|x| 2**-24 on e_c, which reaches a score p_k obj through e_k itself and through the sum, together at most sum_c |x_c| 2**-23 p_c obj - below
1e-6 for any class count the library accepts, and on these cases the kernels stay within a quarter of the plain bar (figures below).

What one decode must satisfy with itself, exactly, on the same raw heads: op_decode_cand's class is the first arg-max of score_full's all_class where
the maximum reaches conf, else -1; its score is that maximum bit for bit where the class is >= 0, that maximum or 0.0 where it is -1 (a candidate
whose objectness alone puts it below logit(conf) - 0.01 has score 0.0 in every front end); its boxes are all_bbox bit for bit.

Front ends: for every head-tail case the candidate arrays - all B * N boxes, scores, classes - of every setting of yn_tail_fuse x yn_fuse_decode x
yn_group_launch are bit-identical to each other and to op_decode_cand on raw heads computed from the same activations with op_dwconv3x3 / op_pwconv and
the handle's folded weights.

Measured on an MI355X: the worst (kernel error) / (4 * e32 + 4 ulp) over all cases of each check, with that case's kernel error and e32.
  score_full all_class      0.24  d-c33-s96 random    1.5e-07 / 1.0e-07        score_full all_bbox       0.13  d-c256-s96 random   1.3e-07 / 1.3e-07
  op_decode_cand score      0.24  d-c33-s96 random    1.5e-07 / 1.0e-07        op_decode_cand boxes      0.13  d-c256-s96 random   1.3e-07 / 1.3e-07
  head tail, decode of the device's raw heads: score 0.20 (t-c16-s64 random), boxes 0.16 (t-c20-s96 steered)
  head tail, raw heads against the float64 tail: 0.32 (t-c80-s96 random, stride 32: 1.5e-06 / 6.9e-07)
Every bit-identity and class assertion held.  Tried once with a deliberately wrong library (no address, bound or loop limit touched): (1) cand_class_stats
walking a lane's classes upwards, so that `first` ends at the lane's HIGHEST class with e == 1, failed all sixteen steered decode cases with C > 16 and the
threshold cases C = 32 and 256, and every steered head-tail case with C > 16; C <= 16 (one class per lane) rightly passed.  (2) head_tail_block writing the
wave-dependent score of a candidate that is out by its objectness alone failed both random C = 80 head-tail cases (the only ones that kernel takes).
"""
import numpy as np
import pytest
import torch

import decode_cases as dc
from f64_bar import bar
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle_for():
    """a handle per class count (no weights: the decode entries need none), moved to the case's grid"""
    from yolo_nano_amd import capi
    cache = {}

    def get(C, S):
        if C not in cache:
            cache[C] = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, max_batch=dc.B)
        h = cache[C]
        if h.S != S:
            h.set_grid(S)
        assert h.N == dc.num_pred(S)
        return h
    yield get
    for h in cache.values():
        h.close()


def _ran(h, fn):
    h.profile_enable(True)
    try:
        y = fn()
        torch.cuda.synchronize()
        names = [r[1] for r in h.profile_records()]
    finally:
        h.profile_enable(False)
    return [t.cpu().numpy() for t in y], names


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    ia, ib = a.view(np.int32), b.view(np.int32)
    if not np.array_equal(ia, ib):
        bad = np.argwhere(ia != ib)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r against %r" % (what, len(bad), a.size, i, a[i], b[i]))


def _box_checks(tag, got, r64, r32):
    ratio = bar("box", tag, _t(got), _t(r64["all_bbox"]), _t(r32["all_bbox"]))
    e32 = float(np.abs(r32["all_bbox"].astype(np.float64) - r64["all_bbox"]).max())
    b = 4 * e32 + 4 * float(np.spacing(np.float32(1.0)))
    pre = r64["pre_clamp"]
    assert (got[pre < -b] == 0.0).all() and (got[pre > 1 + b] == 1.0).all(), tag      # a clamped coordinate is exactly the bound
    assert (got >= 0).all() and (got <= 1).all(), tag
    return ratio


def _data(kind, C, S):
    heads = dc.random_heads(C, S) if kind == "random" else dc.steered_heads(C, S)
    return heads, dc.CONF_RANDOM if kind == "random" else dc.CONF_STEERED


def _score_checks(tag, C, conf, scores, cls, r64, r32):
    """op_decode_cand's (or a fused front end's) scores and classes against the float64 reference"""
    obj_raw, s64 = r64["obj_raw"], r64["score"]
    nan = np.isnan(obj_raw)
    L = dc.skip_logit(conf)
    must_zero, live = obj_raw < L - 1e-4, (obj_raw > L + 1e-4)
    assert (scores[must_zero] == 0.0).all() and (cls[must_zero] == -1).all(), tag
    assert np.isnan(scores[nan]).all() and (cls[nan] == -1).all(), tag              # a NaN objectness gives no detection
    z = lambda a: np.where(live, np.nan_to_num(a.astype(np.float64), nan=0.0), 0.0)
    ratio = bar("score", tag, _t(z(scores)), _t(z(s64)), _t(z(r32["score"])))
    sb = dc.score_bar(r64, r32)
    excused = dc.near_tie_mask(r64, r32)
    above, under = live & (s64 >= conf + sb) & ~excused, live & (s64 < conf - sb)
    bad = above & (cls != r64["best"])
    assert not bad.any(), (tag, "class", np.argwhere(bad)[:5], cls[bad][:5], r64["best"][bad][:5])
    assert (cls[under] == -1).all(), tag
    assert ((cls >= -1) & (cls < C)).all(), tag
    return ratio


@pytest.mark.parametrize("kind", ["random", "steered"])
@pytest.mark.parametrize("case", list(dc.DECODE_CASES))
def test_decode_vs_float64(handle_for, case, kind):
    C, S = dc.DECODE_CASES[case]
    h = handle_for(C, S)
    heads, conf = _data(kind, C, S)
    r64, r32 = dc.decode_ref(heads, S, C), dc.decode_ref(heads, S, C, np.float32)
    hd = [torch.from_numpy(t).cuda() for t in heads]
    tag = "%s %s" % (case, kind)
    # ---- score_full: decode_kernel<true, KMAX>
    (bbox, allc), names = _ran(h, lambda: h.score_full(hd))
    assert names == [dc.decode_kernel(C, True)], names
    nan = np.isnan(r64["obj_raw"])
    assert np.isnan(allc[nan]).all() and not np.isnan(allc[~nan]).any(), tag
    z = lambda a: np.where(nan[..., None], 0.0, a.astype(np.float64))
    bar("allcls", tag, _t(z(allc)), _t(z(r64["all_class"])), _t(z(r32["all_class"])))
    _box_checks(tag + " full", bbox, r64, r32)
    # ---- op_decode_cand: decode_kernel<false, KMAX>
    (boxes, scores, cls), names = _ran(h, lambda: h.op_decode_cand(hd, conf))
    assert names == [dc.decode_kernel(C, False)], names
    _box_checks(tag + " cand", boxes, r64, r32)
    _score_checks(tag, C, conf, scores, cls, r64, r32)
    # ---- steered: the engineered ties give the lowest tied index, and the regimes are those of the data
    if kind == "steered":
        m = dc.regimes(r64, S, C, conf, dc.wave_groups("decode", S))
        for name in dc.REGIMES:
            assert name not in m or m[name].any(), (tag, name)
        tied = ((r64["x"] == 0).sum(-1) >= 2) & (cls >= 0)
        assert tied.any() or C < 2
        assert (cls[tied] == (r64["x"] == 0).argmax(-1)[tied]).all(), tag
    # ---- one decode with itself, exactly
    _bits_equal(boxes, bbox, tag + " boxes against all_bbox")
    with np.errstate(invalid="ignore"):
        mx = np.where(nan, np.float32(np.nan), allc.max(-1))
        first = np.where(nan, 0, (allc == mx[..., None]).argmax(-1))
        want = np.where(mx >= np.float32(conf), first, -1)                         # (NaN >= conf is false)
    assert np.array_equal(cls, want), (tag, np.argwhere(cls != want)[:5])
    kept = cls >= 0
    _bits_equal(scores[kept], mx[kept], tag + " kept scores against the all_class maximum")
    rest = ~kept & ~nan
    assert ((scores[rest].view(np.int32) == mx[rest].view(np.int32)) | (scores[rest] == 0.0)).all(), tag


@pytest.mark.parametrize("C", [16, 32, 256])
def test_score_equal_to_threshold_is_kept(handle_for, C):
    """uniform logits over C = 2**k classes under objectness +40: the score is exactly 1 / C (sum = C, sigmoid = 1.0f); kept at conf = 1 / C,
    dropped at the next float above"""
    S = 64
    h = handle_for(C, S)
    N = dc.num_pred(S)
    heads = dc.pack_heads(np.full((dc.B, N), 40.0, np.float32), np.full((dc.B, N, C), 0.5, np.float32), np.zeros((dc.B, N, 4), np.float32), S)
    r64 = dc.decode_ref(heads, S, C, np.float32)
    assert (r64["score"] == np.float32(1.0 / C)).all()
    hd = [torch.from_numpy(t).cuda() for t in heads]
    conf = np.float32(1.0 / C)
    (_, scores, cls), names = _ran(h, lambda: h.op_decode_cand(hd, float(conf)))
    assert names == [dc.decode_kernel(C, False)]
    assert (scores == conf).all() and (cls == 0).all()
    (_, scores, cls), _ = _ran(h, lambda: h.op_decode_cand(hd, float(np.nextafter(conf, np.float32(1)))))
    assert (scores == conf).all() and (cls == -1).all()                              # the score is one ulp below this threshold


# =====================================================================================================================================
# the fused front ends
# =====================================================================================================================================
@pytest.fixture(scope="module")
def tail_handle():
    from yolo_nano_amd import capi
    cache = {}

    def get(C, S, kind):
        if (C, kind) not in cache:
            sd = dc.random_state_dict(C)
            conf = dc.CONF_RANDOM
            if kind == "steered":
                sd, conf = dc.steered_state_dict(sd, C), dc.CONF_STEERED
            h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, conf_thresh=conf, max_batch=dc.B)
            h.load_state_dict(sd)
            h.fold_bn()
            cache[(C, kind)] = (h, sd, conf)
        h, sd, conf = cache[(C, kind)]
        if h.S != S:
            h.set_grid(S)
        return h, sd, conf
    yield get
    for h, _, _ in cache.values():
        h.close()


@pytest.mark.parametrize("kind", ["random", "steered"])
@pytest.mark.parametrize("case", list(dc.HEAD_TAIL_CASES))
def test_head_tail_front_ends(tail_handle, case, kind):
    C, S = dc.HEAD_TAIL_CASES[case]
    h, sd, conf = tail_handle(C, S, kind)
    acts = dc.random_acts(S) if kind == "random" else dc.steered_acts(C, S)
    xs = [torch.from_numpy(x).cuda() for x in acts]
    tag = "%s %s" % (case, kind)
    # ---- the raw heads of the same activations, layer by layer with the handle's folded weights, and their plain decode
    shapes = ((dc.NECK, 1, 3, 3), (dc.NECK, dc.NECK, 1, 1), (dc.A * (5 + C), dc.NECK, 1, 1))
    raws, lays = [], []
    for hd, x in enumerate(xs):
        lay = [h.get_folded(conv, shp) for (conv, _), shp in zip(dc.head_keys(hd + 1), shapes)]
        (wd, bd), (wp, bp), (wf, bf) = [(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()) for w, b in lay]
        y = h.op_pwconv(h.op_dwconv3x3(x, wd, bd, 1, 2), wp, bp, 2)
        raws.append(h.op_pwconv(y, wf, bf, 0))
        lays.append([a for wb in lay for a in wb])
    raw_np = [r.cpu().numpy() for r in raws]
    if kind == "steered":                                   # the selection is exact: raw[n] = activation[n mod 96] + bias[n], in the folded weights too
        want = dc.selection_layers(C)
        for lay, x, r in zip(lays, acts, raw_np):
            for a, b in zip(lay, want):
                _bits_equal(a, b, tag + " folded selection weights")
            _bits_equal(r, dc.tail_ref(x, *want, dtype=np.float32), tag + " raw heads of the selection")
    (rb, rs, rc), names = _ran(h, lambda: h.op_decode_cand(raws, conf))
    assert names == [dc.decode_kernel(C, False)], names
    # ---- every switch setting: the kernel the rules name, the same B * N candidates bit for bit
    try:
        for tail, fuse, group in dc.SWITCHES:
            h.tail_fuse(tail); h.fuse_decode(fuse); h.group_launch(group)
            (boxes, scores, cls), names = _ran(h, lambda: h.op_head_tail(xs))
            ran = [n for n in names if dc.is_decode_kernel(n)]
            assert ran == dc.front_end(C, S, tail, fuse, group), (tag, (tail, fuse, group), names)
            what = "%s tail %d fuse %d group %d (%s)" % (tag, tail, fuse, group, ran[0])
            _bits_equal(boxes, rb, what + " boxes")
            _bits_equal(scores, rs, what + " scores")
            assert np.array_equal(cls, rc), what
    finally:
        h.tail_fuse(True); h.fuse_decode(True); h.group_launch(True)
    # ---- and against float64: the decode of the device's raw heads, and (random) the whole tail from the activations
    r64, r32 = dc.decode_ref(raw_np, S, C), dc.decode_ref(raw_np, S, C, np.float32)
    _box_checks(tag + " raw", rb, r64, r32)
    _score_checks(tag + " raw", C, conf, rs, rc, r64, r32)
    if kind == "steered":
        for front in ("decode", "head_decode", "head_tail"):
            m = dc.regimes(r64, S, C, conf, dc.wave_groups(front, S))
            for name in dc.HEAD_TAIL_REGIMES:
                if name == "tie_same_lane" and C <= 16:
                    continue
                assert m[name].any(), (tag, front, name)
    else:
        t64 = [dc.tail_ref(x, *lay, dtype=np.float64) for x, lay in zip(acts, lays)]
        t32 = [dc.tail_ref(x, *lay, dtype=np.float32) for x, lay in zip(acts, lays)]
        for s, (r, a, b) in enumerate(zip(raw_np, t64, t32)):
            bar("tailraw", "%s s%d" % (tag, s), _t(r), _t(a), _t(b))


# =====================================================================================================================================
# argmax_cand_kernel through yn_postprocess, nothing suppressed (nms_thresh 1.0)
# =====================================================================================================================================
@pytest.mark.parametrize("C", [1, 17, 80])
def test_argmax_cand(handle_for, C):
    h = handle_for(C, 64)
    rs = np.random.RandomState(31 + C)
    N, conf = 70, np.float32(0.5)
    allc = rs.uniform(0.0, 0.49, size=(dc.B, N, C)).astype(np.float32)
    want_cls = np.full((dc.B, N), -1)
    for b in range(dc.B):
        for n in range(0, N, 2):                             # every second candidate passes, with a class of its own
            c = (n * 7 + b) % C
            allc[b, n, c] = np.float32(0.5 + 0.4 * rs.uniform())
            want_cls[b, n] = c
        if C > 1:
            allc[b, 4, :] = 0.25; allc[b, 4, [C - 1, 0]] = 0.75; want_cls[b, 4] = 0                        # exact tie, first and last class
            allc[b, 6, :] = 0.25; allc[b, 6, [C - 1, C - 1 - 16 % C]] = 0.875; want_cls[b, 6] = min(C - 1, C - 1 - 16 % C)   # c and c + 16
            allc[b, 8, :] = 0.75; want_cls[b, 8] = 0                                                       # all equal
        allc[b, 10, :] = 0.25; allc[b, 10, C // 2] = conf; want_cls[b, 10] = C // 2                        # score == thresh is kept
        allc[b, 12, :] = 0.25; allc[b, 12, C // 2] = np.nextafter(conf, np.float32(0)); want_cls[b, 12] = -1   # one ulp below is not
        allc[b, 14, :] = np.nan; want_cls[b, 14] = -1                                                      # a NaN row gives no detection
    n = np.arange(N, dtype=np.float32)
    x0 = (n % 10) * 0.1
    y0 = (n // 10) * 0.1
    box = np.tile(np.stack([x0, y0, x0 + 0.05, y0 + 0.05], -1)[None], (dc.B, 1, 1)).astype(np.float32)     # disjoint boxes
    h.set_thresholds(float(conf), 1.0)
    boxes, scores, cls, index, count = [t.cpu().numpy() for t in h.postprocess(torch.from_numpy(box).cuda(), torch.from_numpy(allc).cuda())]
    for b in range(dc.B):
        keep = np.nonzero(want_cls[b] >= 0)[0]
        k = int(count[b])
        assert k == len(keep), (C, b, k, len(keep))
        assert np.array_equal(index[b, :k], keep), (C, b)
        assert np.array_equal(cls[b, :k], want_cls[b, keep]), (C, b, cls[b, :k], want_cls[b, keep])
        _bits_equal(scores[b, :k], allc[b, keep, want_cls[b, keep]], "argmax scores C %d image %d" % (C, b))
        _bits_equal(boxes[b, :k], box[b, keep], "argmax boxes C %d image %d" % (C, b))
