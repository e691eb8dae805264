"""Exact restatement of the package's Soft-NMS (csrc/kernels_soft.hip) in float32 numpy.  No GPU, no native code.

The rule is the package's own (after Bodla et al., 2017; parity with any third-party implementation is unpinned).  Per (list, class)
segment the live rows are those with score > score_floor (strict: a NaN score is never live).  While a row is live, the live row with the
largest CURRENT score is picked (equal scores: the higher row, nms_stage_oracle.sort_segment's tie rule), kept with that score, and every
remaining live row's score is multiplied by a weight of its overlap with the picked box - ovr in nms_stage_oracle.suppresses' arithmetic,
the picked box in the place of bi:

    hard      w = hit ? 0 : 1            hit = !(ovr <= thr): a NaN hits
    linear    w = hit ? 1 - ovr : 1
    gaussian  w = E(-((ovr * ovr) / sigma))   for every row; thr is not used

A row leaves the live set unless its new score is > score_floor.  Every multiply, add, subtract and divide is one float32 operation and
E is the package's own exp, so tests compare with `==` on the bits.
"""
import numpy as np

from nms_stage_oracle import F, area, sort_segment

OFF, HARD, LINEAR, GAUSSIAN = 0, 1, 2, 3
METHODS = {"hard": HARD, "linear": LINEAR, "gaussian": GAUSSIAN}
EXP_COEF = (1.9875691500e-4, 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1)


def E(x):
    """The package's exp for x <= 0, float32 in and out: NaN -> NaN, x < -87 -> 0, else 2^k * (1 + r + r^2 p(r)) with k = rint(x log2 e),
    r = x - k ln 2 in two pieces, p by Horner's rule - one multiply and one add per step."""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        dead = np.isnan(x) | (x < F(-87.0))
        xs = np.where(dead, F(0), x).astype(F)
        k = np.rint(xs * F(1.44269504)).astype(F)
        r = ((xs - k * F(0.693359375)).astype(F) - k * F(-2.12194440e-4)).astype(F)
        p = np.full(x.shape, F(EXP_COEF[0]), F)
        for c in EXP_COEF[1:]:
            p = ((p * r).astype(F) + F(c)).astype(F)
        y = (((p * (r * r).astype(F)).astype(F) + r).astype(F) + F(1.0)).astype(F)
        out = np.ldexp(y, k.astype(np.int32)).astype(F)
    out = np.where(x < F(-87.0), F(0), out)
    return np.where(np.isnan(x), F(np.nan), out).astype(F)


def ovr(p, b):
    """nms_stage_oracle.suppresses' ovr with the picked box p [4] in the place of bi, against the rows b [m, 4] -> float32 [m]."""
    p = np.asarray(p, F); b = np.asarray(b, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        xx1 = np.maximum(p[0], b[:, 0]); yy1 = np.maximum(p[1], b[:, 1])
        xx2 = np.minimum(p[2], b[:, 2]); yy2 = np.minimum(p[3], b[:, 3])
        w = np.maximum(F(1e-28), xx2 - xx1); h = np.maximum(F(1e-28), yy2 - yy1)
        inter = (w * h).astype(F)
        return (inter / ((area(p) + area(b)).astype(F) - inter)).astype(F)


def weight(o, method, thr, sigma):
    """The factor of a row whose overlap with the picked box is o -> float32, o's shape."""
    o = np.asarray(o, F)
    with np.errstate(all="ignore"):
        if method == GAUSSIAN:
            return E(-((o * o).astype(F) / F(sigma)).astype(F))
        hit = ~(o <= F(thr))
        if method == HARD:
            return np.where(hit, F(0), F(1)).astype(F)
        if method == LINEAR:
            return np.where(hit, (F(1.0) - o).astype(F), F(1)).astype(F)
    raise ValueError("method %r is not HARD, LINEAR or GAUSSIAN" % (method,))


def pick(rows, s, live):
    """The position (into rows) of the live row with the largest score, the higher row among equals."""
    idx = np.flatnonzero(live)
    cand = idx[s[idx] == s[idx].max()]
    return int(cand[np.argmax(rows[cand])])


def soft_segment(boxes, score, rows, method, thr, sigma, score_floor, trace=None):
    """One segment: rows = its list rows (any order) -> [(row, kept score)] in pick order.  trace (a list, optional) receives every
    overlap array the walk computed."""
    boxes = np.asarray(boxes, F); rows = np.asarray(rows, np.int64)
    b = boxes[rows]; s = np.asarray(score, F)[rows].copy()
    floor = F(score_floor)
    with np.errstate(all="ignore"):
        live = s > floor
    kept = []
    while live.any():
        p = pick(rows, s, live)
        kept.append((int(rows[p]), F(s[p])))
        live[p] = False
        idx = np.flatnonzero(live)
        if not len(idx):
            break
        o = ovr(b[p], b[idx])
        if trace is not None:
            trace.append(o)
        with np.errstate(all="ignore"):
            s[idx] = (s[idx] * weight(o, method, thr, sigma)).astype(F)
            live[idx] = s[idx] > floor
    return kept


def soft_nms(boxes, score, cls, C, method, thr, sigma, score_floor, trace=None):
    """One list: boxes [n, 4], score [n], cls [n] (-1: not a row) -> (boxes [K, 4] f32, scores [K] f32, cls [K] i32, index [K] i32): the
    kept rows in ascending row order, the box bit for bit, the score decayed."""
    boxes = np.asarray(boxes, F).reshape(-1, 4); score = np.asarray(score, F).reshape(-1); cls = np.asarray(cls).astype(np.int64).reshape(-1)
    out = []
    for c in range(C):
        for r, sc in soft_segment(boxes, score, np.flatnonzero(cls == c), method, thr, sigma, score_floor, trace):
            out.append((r, sc, c))
    out.sort(key=lambda t: t[0])
    oi = np.asarray([t[0] for t in out], np.int32)
    return (boxes[oi].reshape(-1, 4).astype(F), np.asarray([t[1] for t in out], F), np.asarray([t[2] for t in out], np.int32), oi)


def soft_records(boxes, score, cls, count, C, method, thr, sigma, score_floor):
    """B lists [B, cap, ...] with count [B] rows each -> (rec [total, 6] f32, offsets [B + 1] i32) in yn_pack_detections' layout."""
    recs, off = [], [0]
    for b in range(len(count)):
        m = int(count[b])
        ob, os_, oc, _ = soft_nms(boxes[b][:m], score[b][:m], cls[b][:m], C, method, thr, sigma, score_floor)
        recs.append(np.concatenate([ob, os_[:, None], oc.astype(F)[:, None]], axis=1).astype(F))
        off.append(off[-1] + len(ob))
    return (np.concatenate(recs) if recs else np.zeros((0, 6), F)), np.asarray(off, np.int32)


def nms_merge(boxes, score, cls, C, thr):
    """yn_nms_merge restated from nms_stage_oracle (sort_segment + greedy): the kept rows in ascending row order, the same four arrays."""
    from nms_stage_oracle import greedy
    boxes = np.asarray(boxes, F).reshape(-1, 4); score = np.asarray(score, F).reshape(-1); cls = np.asarray(cls).astype(np.int64).reshape(-1)
    keep = []
    for c in range(C):
        ids = sort_segment(np.flatnonzero(cls == c), score)
        keep += list(ids[greedy(boxes[ids], thr)])
    oi = np.sort(np.asarray(keep, np.int64)).astype(np.int32)
    return boxes[oi].reshape(-1, 4), score[oi], cls[oi].astype(np.int32), oi


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
