"""Exact restatements of the stages of the per-class NMS chain (csrc/kernels_post.hip: bucket -> sort -> prefilter -> matrix / sweep ->
resolve -> compact) and of launch_nms_pipeline's launch rules, in numpy.  No GPU, no native code.

Every arithmetic step is an elementwise IEEE float32 operation in the reference's order (models/yolo_nano.py:159-188, 191-242), so the
restatements are bit-exact, not approximate: tests compare them with `==`.  tests/test_nms_cases_cpu.py shows that the composed stages give
exactly the C oracle's postprocess on every case of tests/nms_cases.py; tests/test_gpu_nms_stages.py compares the device's state after each
stage (yn_nms_stages) with them.
"""
import numpy as np

F = np.float32
SORT_SMALL = 1024            # YN_SORT_SMALL: a class above this many boxes is LARGE (listed, chunk-sorted, column-major tiles)
SORT_LARGE = 16384           # YN_SORT_LARGE: the whole-LDS bitonic sort; also few_n of launch_nms_pipeline
SWEEP_MAXN = 6144            # YN_SWEEP_MAXN
SWEEP_IRR = 64               # YN_SWEEP_IRR
SWEEP_WIDE = 256             # YN_SWEEP_WIDE
PRE_W, PRE_Z, PRE_RANKS, PRE_TICKETS = 8, 8, 4, 4096

PLAN_FIELDS = ("B", "N", "C", "few", "fused", "chunks", "merge", "prefilter", "pre_ranks", "sweep", "sweep_maxn", "sweep_slots",
               "sweep_split", "resolve_one", "resolve_split", "diou")


# ---- launch rules (launch_nms_pipeline on a handle that ensure_post prepared) -----------------------------------------------------------
def large_cap(N, C):
    return min(N // 1024 + 1, C)                             # ensure_post


def plan(B, N, C, thresh, diou=False, prefilter_mode=1, sweep_on=True):
    """The launch plan of one call.  ensure_post always provides ctr, large_list, sbox2, seg_sparse, work_off and pre_sync, and
    N <= matrix_stride (64 * T (T + 1) / 2 words with T = ceil(N / 64) + C >= N): those conditions are constants here."""
    few = B * C <= 256 and N <= 16384
    fused = few
    chunks = not few
    merge = chunks and N > SORT_SMALL
    pre = (not diou) and (prefilter_mode == 2 or (prefilter_mode == 1 and B >= 4))
    cap = large_cap(N, C)
    pre_ranks = (min(C, PRE_RANKS) if (not fused and B * PRE_RANKS <= PRE_TICKETS) else 0) if pre else 0
    sweep = bool(pre and sweep_on and not few and cap > 0 and N > SORT_SMALL and F(thresh) >= F(1e-6))
    maxn = SWEEP_MAXN // 2 if N <= 16384 else SWEEP_MAXN
    split = max(2, min(8, (256 if maxn * 20 <= 64 * 1024 else 128) // B))
    one = B * C <= 256
    v = dict(B=B, N=N, C=C, few=few, fused=fused, chunks=chunks, merge=merge, prefilter=pre, pre_ranks=pre_ranks, sweep=sweep,
             sweep_maxn=maxn if sweep else 0, sweep_slots=min(cap, 4) if sweep else 0, sweep_split=split if sweep else 0,
             resolve_one=one, resolve_split=(not one) and N > SORT_SMALL and cap > 0, diou=bool(diou))
    return {k: int(v[k]) for k in PLAN_FIELDS}


# ---- candidates (argmax_cand_kernel; models/yolo_nano.py:253-261) ---------------------------------------------------------------------------
def candidates(conf, conf_thresh):
    """conf [N, C] -> (cls [N] int, -1 = no candidate; score [N] float32): first maximum, kept when score >= conf_thresh."""
    conf = np.asarray(conf, F)
    cls = conf.argmax(1)
    score = conf[np.arange(len(conf)), cls]
    return np.where(score >= F(conf_thresh), cls, -1).astype(np.int64), score


# ---- bucket ------------------------------------------------------------------------------------------------------------------------
def bucket(cls, C):
    """-> counts [C], offsets [C] (exclusive prefix), large list (classes above 1 024 boxes, ascending id, at most large_cap),
    seg_order [C] (count descending, class ascending)."""
    cls = np.asarray(cls)
    counts = np.bincount(cls[cls >= 0], minlength=C).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    large = [c for c in range(C) if counts[c] > SORT_SMALL][:large_cap(len(cls), C)]
    order = sorted(range(C), key=lambda c: (-counts[c], c))
    return counts, off, large, order


# ---- sort --------------------------------------------------------------------------------------------------------------------------
def sort_segment(ids, score):
    """Candidate ids of one class -> by (score descending, candidate id descending): `scores.argsort()[::-1]` with the oracle's pinned tie rule."""
    ids = np.asarray(ids, np.int64)
    return ids[np.lexsort((-ids, -np.asarray(score, np.float64)[ids]))]


# ---- predicate ---------------------------------------------------------------------------------------------------------------------
def area(b):
    b = np.asarray(b, F)
    with np.errstate(all="ignore"):
        return ((b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])).astype(F)


def suppresses(bi, bj, thresh, diou=False):
    """Does kept box bi [4] REMOVE each box of bj [m, 4]?  The reference keeps `ovr <= thresh`; NaN is removed."""
    bi = np.asarray(bi, F); bj = np.asarray(bj, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        xx1 = np.maximum(bi[0], bj[:, 0]); yy1 = np.maximum(bi[1], bj[:, 1])
        xx2 = np.minimum(bi[2], bj[:, 2]); yy2 = np.minimum(bi[3], bj[:, 3])
        w = np.maximum(F(1e-28), xx2 - xx1); h = np.maximum(F(1e-28), yy2 - yy1)
        inter = (w * h).astype(F)
        ovr = inter / ((area(bi) + area(bj)).astype(F) - inter)
        if diou:                                             # models/yolo_nano.py:216-236, as suppressed() writes it
            x = np.stack([np.full(len(bj), bi[0], F), np.full(len(bj), bi[2], F), bj[:, 0], bj[:, 2]])
            y = np.stack([np.full(len(bj), bi[1], F), np.full(len(bj), bi[3], F), bj[:, 1], bj[:, 3]])
            dx = np.fmax.reduce(x) - np.fmin.reduce(x); dy = np.fmax.reduce(y) - np.fmin.reduce(y)
            Cd = np.sqrt(dx * dx + dy * dy, dtype=F)
            ex = (bj[:, 0] + bj[:, 2]) / F(2) - (bi[0] + bi[2]) / F(2); ey = (bj[:, 1] + bj[:, 3]) / F(2) - (bi[1] + bi[3]) / F(2)
            D = np.sqrt(ex * ex + ey * ey, dtype=F)
            ovr = ovr - (D * D) / (Cd * Cd + F(1e-20))
        return ~(ovr <= F(thresh))


def greedy(boxes, thresh, diou=False):
    """Greedy NMS over boxes already in pick order -> bool [n], True = kept."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    kept = np.zeros(len(boxes), bool)
    alive = np.arange(len(boxes))
    while len(alive):
        i = alive[0]
        kept[i] = True
        rest = alive[1:]
        alive = rest[~suppresses(boxes[i], boxes[rest], thresh, diou)]
    return kept


# ---- prefilter ---------------------------------------------------------------------------------------------------------------------
def prefilter(sboxes, thresh):
    """Sorted boxes of one class -> (kept0: bool [min(n, 64)], the greedy result among the first 64; surv: sorted positions >= 64 that no
    chunk-0-KEPT box removes, ascending).  A one-chunk class has no survivors (seg_count2 = 0)."""
    sboxes = np.asarray(sboxes, F).reshape(-1, 4)
    kept0 = greedy(sboxes[:64], thresh)
    rest = sboxes[64:]
    dead = np.zeros(len(rest), bool)
    for i in np.flatnonzero(kept0):
        dead |= suppresses(sboxes[i], rest, thresh)
    return kept0, 64 + np.flatnonzero(~dead)


def final_keep(sboxes, thresh, diou=False, use_prefilter=True):
    """bool [n] over sorted positions: chunk-0 kept | greedy over the survivors (prefilter), or plain greedy."""
    sboxes = np.asarray(sboxes, F).reshape(-1, 4)
    if not use_prefilter or diou:
        return greedy(sboxes, thresh, diou)
    kept0, surv = prefilter(sboxes, thresh)
    keep = np.zeros(len(sboxes), bool)
    keep[:len(kept0)] = kept0
    keep[surv[greedy(sboxes[surv], thresh)]] = True
    return keep


# ---- sweep decision (sweep_spread_out, on the class's sorted boxes at positions >= 64, before the prefilter) ----------------------------------
def sweep_regular(b):
    b = np.asarray(b, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        w = b[:, 2] - b[:, 0]; a = (w * (b[:, 3] - b[:, 1])).astype(F)
        fin = np.isfinite(b).all(1)
        return fin & (w > F(1e-20)) & (a >= F(1e-20)) & (a < F(3.0e38))


def sweep_visits(sboxes):
    """-> (visits, limit, irregular): the restated visit count of the boxes at sorted positions >= 64 - every irregular box against all n,
    every regular box against the regular boxes whose LEFT EDGE lies inside its x-extent (itself included) - and the kernel's limit
    m (m - 1) / 8.  The kernel counts by 1 024 bins of the left edges, so its count is this one plus the strangers in a box's first and last
    bin: a decision is only called unambiguous when visits <= limit / 2 or visits >= 2 * limit (sweep_expected)."""
    sboxes = np.asarray(sboxes, F).reshape(-1, 4)
    n = len(sboxes); t = sboxes[64:]; m = len(t)
    reg = sweep_regular(t)
    x1 = np.sort(t[reg, 0].astype(np.float64))
    lo = np.searchsorted(x1, t[reg, 0].astype(np.float64), "left"); hi = np.searchsorted(x1, t[reg, 2].astype(np.float64), "right")
    return int((hi - lo).sum()) + int((~reg).sum()) * n, m * (m - 1) // 8, int((~reg).sum())


def sweep_expected(sboxes, n2, decided, sweep_maxn):
    """seg_sparse of one class: 1, 0, or None where the bin estimate could fall on either side.  decided: the class is sliced (rank <
    pre_ranks, more than 576 boxes), above 1 024 boxes and among the image's first sweep_slots listed classes."""
    n = len(sboxes)
    if not decided or n - 64 > SWEEP_MAXN or not (SORT_SMALL < n2 <= sweep_maxn):
        return 0
    visits, limit, nirr = sweep_visits(sboxes)
    if nirr > SWEEP_IRR or visits >= 2 * limit:
        return 0
    return 1 if 2 * visits <= limit else None


# ---- one image, all stages -------------------------------------------------------------------------------------------------------------
def stages(boxes, cls, score, C, thresh, diou, pl, with_keep=True):
    """boxes [N, 4], cls [N] (-1: none), score [N]; pl = plan(...) of the call -> dict of the state yn_nms_stages shows for this image:
    seg_count, seg_off [C]; bucket [sum], sbox [sum, 4] (valid prefix); with the prefilter seg_count2 [C], bucket2 {class: ids},
    seg_sparse [C] of 1 / 0 / None; keep [N] (with_keep=False leaves the greedy walks out: keep is None)."""
    boxes = np.asarray(boxes, F); N = len(boxes)
    counts, off, large, order = bucket(cls, C)
    out = dict(seg_count=counts, seg_off=off, large=large, order=order, bucket=np.zeros(int(counts.sum()), np.int64))
    keep = np.zeros(N, np.int32)
    n2s = np.zeros(C, np.int64); b2 = {}; sparse = [0] * C
    for c in range(C):
        n = int(counts[c])
        if not n:
            continue
        ids = sort_segment(np.flatnonzero(cls == c), score)
        out["bucket"][off[c]:off[c] + n] = ids
        sb = boxes[ids]
        if pl["prefilter"]:
            kept0, surv = prefilter(sb, thresh)
            n2s[c] = len(surv); b2[c] = ids[surv]
            k = np.zeros(n, bool); k[:len(kept0)] = kept0
            if with_keep:
                k[surv[greedy(sb[surv], thresh)]] = True
            rank = order.index(c)
            decided = bool(pl["sweep"]) and rank < pl["pre_ranks"] and n > 64 * (PRE_W + 1) and n > SORT_SMALL and c in large[:pl["sweep_slots"]]
            sparse[c] = sweep_expected(sb, len(surv), decided, pl["sweep_maxn"])
        else:
            k = greedy(sb, thresh, diou) if with_keep else np.zeros(n, bool)
        keep[ids[k]] = 1
    out["sbox"] = boxes[out["bucket"]]
    out["keep"] = keep if with_keep else None
    if pl["prefilter"]:
        out.update(seg_count2=n2s, bucket2=b2, seg_sparse=sparse)
    return out
