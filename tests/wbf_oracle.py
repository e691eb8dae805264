"""Exact restatement of the package's weighted box fusion (csrc/kernels_wbf.hip) in float32 numpy.  No GPU, no native code.

The rule is the package's own (parity with the ensemble_boxes family is unpinned).  Per (list, class) segment the rows are visited in the
pick order of the NMS chain's sort (nms_stage_oracle.sort_segment: score descending, higher row first among equals).  A row joins the
cluster whose FUSED box has the largest ovr with it among those with ovr > thr (strict; NaN never matches; equal ovr: the lowest cluster),
else it founds a cluster.  Every multiply, add and divide is one float32 operation, so tests compare with `==` on the bits.
"""
import numpy as np

from nms_stage_oracle import F, area, sort_segment


def ovr(fb, b):
    """The IoU arithmetic of nms_stage_oracle.suppresses with the cluster's fused box fb [k, 4] in the place of bi, against one row b [4]
    -> float32 [k]."""
    fb = np.asarray(fb, F).reshape(-1, 4); b = np.asarray(b, F)
    with np.errstate(all="ignore"):
        xx1 = np.maximum(fb[:, 0], b[0]); yy1 = np.maximum(fb[:, 1], b[1])
        xx2 = np.minimum(fb[:, 2], b[2]); yy2 = np.minimum(fb[:, 3], b[3])
        w = np.maximum(F(1e-28), xx2 - xx1); h = np.maximum(F(1e-28), yy2 - yy1)
        inter = (w * h).astype(F)
        return (inter / ((area(fb) + area(b)).astype(F) - inter)).astype(F)


def fuse_segment(boxes, score, ids, thr, stats=None):
    """One segment: ids = its list rows in pick order -> list of clusters dict(founder, n, S, P, Fb, rows) in creation order.
    stats (a dict, optional) counts "drift" joins: the row matched the fused box, but ovr against the founder's box is not above thr."""
    boxes = np.asarray(boxes, F); score = np.asarray(score, F); thr = F(thr)
    cl = []
    room = np.zeros((len(ids), 4), F)                          # the fused boxes of the clusters so far: room[:len(cl)]
    for i in ids:
        b = boxes[i]; s = score[i]
        best = -1
        if len(cl):
            o = ovr(room[:len(cl)], b)
            with np.errstate(all="ignore"):
                ok = o > thr                                   # NaN: False
            if ok.any():
                cand = np.flatnonzero(ok)
                best = int(cand[np.argmax(o[cand])])           # first maximum: the lowest cluster among equals
        with np.errstate(all="ignore"):
            if best < 0:
                cl.append(dict(founder=int(i), n=1, S=F(s), P=(s * b).astype(F), Fb=b.copy(), rows=[int(i)]))
                room[len(cl) - 1] = b
            else:
                c = cl[best]
                if stats is not None:
                    of = ovr(boxes[c["founder"]][None], b)[0]
                    if not of > thr:
                        stats["drift"] = stats.get("drift", 0) + 1
                c["n"] += 1
                c["S"] = F(c["S"] + s)
                c["P"] = (c["P"] + (s * b).astype(F)).astype(F)
                c["Fb"] = (c["P"] / c["S"]).astype(F)
                c["rows"].append(int(i))
                room[best] = c["Fb"]
    return cl


def wbf(boxes, score, cls, C, thr, E, stats=None):
    """One list: boxes [n, 4], score [n], cls [n] (-1: not a row) -> (boxes [K, 4] f32, scores [K] f32, cls [K] i32, founder [K] i32,
    votes [K] i32, assign [n] i32), the clusters in ascending order of the founder's row."""
    boxes = np.asarray(boxes, F).reshape(-1, 4); score = np.asarray(score, F); cls = np.asarray(cls).astype(np.int64)
    n = len(boxes)
    assert int(E) >= 1
    out = []
    assign = np.full(n, -1, np.int32)
    for c in range(C):
        ids = sort_segment(np.flatnonzero(cls == c), score)
        for k in fuse_segment(boxes, score, ids, thr, stats):
            with np.errstate(all="ignore"):
                sc = F(F(k["S"] / F(k["n"])) * F(F(min(k["n"], int(E))) / F(int(E))))
            out.append((k["founder"], k["Fb"], sc, c, k["n"]))
            assign[k["rows"]] = k["founder"]
    out.sort(key=lambda r: r[0])
    K = len(out)
    ob = np.zeros((K, 4), F); os_ = np.zeros(K, F); oc = np.zeros(K, np.int32); of = np.zeros(K, np.int32); ov = np.zeros(K, np.int32)
    for i, (f, fb, sc, c, v) in enumerate(out):
        ob[i] = fb; os_[i] = sc; oc[i] = c; of[i] = f; ov[i] = v
    return ob, os_, oc, of, ov, assign


def wbf_records(boxes, score, cls, count, C, thr, E):
    """B lists [B, cap, ...] with count [B] rows each -> (rec [total, 6] f32, offsets [B + 1] i32) in yn_pack_detections' layout."""
    recs, off = [], [0]
    for b in range(len(count)):
        m = int(count[b])
        ob, os_, oc, _, _, _ = wbf(boxes[b][:m], score[b][:m], cls[b][:m], C, thr, E)
        recs.append(np.concatenate([ob, os_[:, None], oc.astype(F)[:, None]], axis=1).astype(F))
        off.append(off[-1] + len(ob))
    return (np.concatenate(recs) if recs else np.zeros((0, 6), F)), np.asarray(off, np.int32)


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
