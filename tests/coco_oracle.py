"""Host restatement of pycocotools' COCOeval for iouType 'bbox' with its default parameters, as literal loops: computeIoU (the C
routine bbIou), evaluateImg, accumulate and summarize, plus the detection route of evaluator/cocoapi_evaluator.py:85-99 (un-letterbox
in float32 steps, then float64 [x, y, w, h]).  Used by the CPU tests (hand-worked cases, tests/golden/coco_eval.npz) and by the GPU
tests (against yn_coco_*).  pycocotools is not importable where this was written, so PARITY WITH PYCOCOTOOLS IS UNPINNED here;
tests/golden/gen_coco_eval.py asserts it wherever the library can be imported.

Data model.  One image is a dict:
    id        int image id
    gt        float64 [G][5] = x, y, w, h, area (area as the annotation file gives it, not w*h), in file order
    gt_cat    int [G] category index 0..C-1
    gt_crowd  int [G] iscrowd
    dt        float64 [K][4] = x, y, w, h in results-list order
    dt_score  float64 [K]
    dt_cat    int [K]
"""
import numpy as np


def default_params():
    return {"iouThrs": np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            "recThrs": np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            "maxDets": [1, 10, 100],
            "areaRng": [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]}


def geometry_arrays(geom):
    """(scale, offset, size) as ValTransforms / the evaluator build them from one (w0, h0, rw, rh, left, top, side) row."""
    w0, h0, rw, rh, left, top, side = [int(v) for v in geom]
    if h0 > w0:
        scale, offset = np.array([[rw / side, 1., rw / side, 1.]]), np.array([[left / side, 0., left / side, 0.]])
    elif h0 < w0:
        scale, offset = np.array([1., rh / side, 1., rh / side]), np.array([[0., top / side, 0., top / side]])
    else:
        scale, offset = 1., np.zeros([1, 4])
    return scale, offset, np.array([[w0, h0, w0, h0]])


def ingest(boxes, scores, geom):
    """Normalised float32 boxes [K,4] + float32 scores [K] of one image -> (bbox float64 [K][4] = x, y, w, h; score float64 [K]):
    bboxes -= offset; /= scale; *= size on the float32 array, then float() of each element and w = x2 - x1, h = y2 - y1 in float64."""
    scale, offset, size = geometry_arrays(geom)
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    b -= offset
    b /= scale
    b *= size
    out = np.zeros((len(b), 4), dtype=np.float64)
    for i in range(len(b)):
        x1, y1, x2, y2 = float(b[i, 0]), float(b[i, 1]), float(b[i, 2]), float(b[i, 3])
        out[i] = [x1, y1, x2 - x1, y2 - y1]
    sc = np.array([float(s) for s in np.asarray(scores, dtype=np.float32).reshape(-1)], dtype=np.float64)
    return out, sc


def bb_iou(d, g, crowd):
    """maskApi.c bbIou for one pair of [x, y, w, h] boxes"""
    da, ga = d[2] * d[3], g[2] * g[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def evaluate_img(dt, dt_score, gt, gt_crowd, area_rng, iou_thrs, max_det):
    """One (image, category, area range): dt float64 [K][4] / dt_score [K] in results-list order, gt float64 [G][5] (x, y, w, h, area)
    / gt_crowd [G] in file order.  -> None when both are empty, else a dict with
        order    indices into dt of the detections kept, by -score (stable), first max_det
        scores   their scores
        matched  bool [T][D]   (dtMatches != 0)
        match_gt int  [T][D]   index into the ORIGINAL gt list, -1 unmatched
        dt_ig    bool [T][D]
        gt_ig    bool [G] in the ORIGINAL gt order"""
    K, G = len(dt), len(gt)
    if K == 0 and G == 0:
        return None
    lo, hi = area_rng
    neg = [-float(s) for s in dt_score]
    order = [int(i) for i in np.argsort(neg, kind='mergesort')][:max_det]
    D = len(order)
    gt_ig_orig = [bool(gt_crowd[g]) or bool(gt[g][4] < lo or gt[g][4] > hi) for g in range(G)]
    gtind = [int(i) for i in np.argsort([int(v) for v in gt_ig_orig], kind='mergesort')]
    gt_ig = [gt_ig_orig[g] for g in gtind]
    crowd = [bool(gt_crowd[g]) for g in gtind]
    ious = [[bb_iou(dt[order[d]], gt[gtind[g]][:4], crowd[g]) for g in range(G)] for d in range(D)]
    T = len(iou_thrs)
    gtm = [[False] * G for _ in range(T)]
    matched = np.zeros((T, D), dtype=bool)
    match_gt = -np.ones((T, D), dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    if G > 0 and D > 0:
        for tind, t in enumerate(iou_thrs):
            for d in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for g in range(G):
                    if gtm[tind][g] and not crowd[g]:
                        continue
                    if m > -1 and not gt_ig[m] and gt_ig[g]:
                        break
                    if ious[d][g] < iou:
                        continue
                    iou = ious[d][g]
                    m = g
                if m == -1:
                    continue
                dt_ig[tind, d] = gt_ig[m]
                matched[tind, d] = True
                match_gt[tind, d] = gtind[m]
                gtm[tind][m] = True
    for d in range(D):
        b = dt[order[d]]
        area = b[2] * b[3]
        out = bool(area < lo or area > hi)
        for tind in range(T):
            if not matched[tind, d] and out:
                dt_ig[tind, d] = True
    return {"order": order, "scores": [float(dt_score[i]) for i in order], "matched": matched, "match_gt": match_gt, "dt_ig": dt_ig,
            "gt_ig": np.array(gt_ig_orig, dtype=bool)}


def evaluate(images, num_classes, params=None):
    """evaluate(): images in sorted(unique(id)) order, every category, every area range -> eval_imgs[k][a][i] (None where empty)"""
    p = params or default_params()
    ids = [int(im["id"]) for im in images]
    assert len(set(ids)) == len(ids), "duplicate image id"
    walk = [images[i] for i in np.argsort(ids, kind='mergesort')]
    max_det = p["maxDets"][-1]
    out = []
    for k in range(num_classes):
        per_area = [[] for _ in p["areaRng"]]
        for im in walk:
            gsel = [g for g in range(len(im["gt"])) if int(im["gt_cat"][g]) == k]
            dsel = [d for d in range(len(im["dt"])) if int(im["dt_cat"][d]) == k]
            gt = [im["gt"][g] for g in gsel]
            cr = [im["gt_crowd"][g] for g in gsel]
            dt = [im["dt"][d] for d in dsel]
            sc = [im["dt_score"][d] for d in dsel]
            for a, rng in enumerate(p["areaRng"]):
                per_area[a].append(evaluate_img(dt, sc, gt, cr, rng, p["iouThrs"], max_det))
        out.append(per_area)
    return out


def accumulate(eval_imgs, params=None):
    """-> precision [T][R][K][A][M], recall [T][K][A][M] float64, -1 where there is no non-ignored ground truth"""
    p = params or default_params()
    T, R, K, A, M = len(p["iouThrs"]), len(p["recThrs"]), len(eval_imgs), len(p["areaRng"]), len(p["maxDets"])
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(p["maxDets"]):
                E = [e for e in eval_imgs[k][a] if e is not None]
                if len(E) == 0:
                    continue
                scores, tpm, igm = [], [[] for _ in range(T)], [[] for _ in range(T)]
                for e in E:
                    n = min(max_det, len(e["scores"]))
                    scores.extend(e["scores"][:n])
                    for t in range(T):
                        tpm[t].extend(bool(v) for v in e["matched"][t][:n])
                        igm[t].extend(bool(v) for v in e["dt_ig"][t][:n])
                inds = np.argsort([-s for s in scores], kind='mergesort')
                npig = 0
                for e in E:
                    for v in e["gt_ig"]:
                        npig += 0 if v else 1
                if npig == 0:
                    continue
                nd = len(scores)
                for t in range(T):
                    tp, fp = np.zeros(nd), np.zeros(nd)
                    ctp = cfp = 0
                    for j, i in enumerate(inds):
                        if tpm[t][i] and not igm[t][i]:
                            ctp += 1
                        if not tpm[t][i] and not igm[t][i]:
                            cfp += 1
                        tp[j], fp[j] = float(ctp), float(cfp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros(R)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, thr in enumerate(p["recThrs"]):
                        pi = 0                                  # np.searchsorted(rc, thr, side='left')
                        while pi < nd and rc[pi] < thr:
                            pi += 1
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall, params=None):
    """The 12 stats of COCOeval.summarize for iouType 'bbox'"""
    p = params or default_params()

    def one(ap, iou_thr=None, area=0, max_det=100):
        a = area
        m = [i for i, v in enumerate(p["maxDets"]) if v == max_det]
        s = precision if ap else recall
        if iou_thr is not None:
            t = np.where(iou_thr == p["iouThrs"])[0]
            s = s[t]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        sel = s[s > -1]
        return -1.0 if len(sel) == 0 else float(np.mean(sel))

    last = p["maxDets"][2]
    return np.array([one(1, max_det=last), one(1, .5, max_det=last), one(1, .75, max_det=last),
                     one(1, area=1, max_det=last), one(1, area=2, max_det=last), one(1, area=3, max_det=last),
                     one(0, max_det=p["maxDets"][0]), one(0, max_det=p["maxDets"][1]), one(0, max_det=last),
                     one(0, area=1, max_det=last), one(0, area=2, max_det=last), one(0, area=3, max_det=last)], dtype=np.float64)


def coco_eval(images, num_classes, params=None):
    """-> (stats [12], precision, recall, eval_imgs)"""
    p = params or default_params()
    ev = evaluate(images, num_classes, p)
    precision, recall = accumulate(ev, p)
    return summarize(precision, recall, p), precision, recall, ev


def image_from_arrays(image_id, gt_rows, dets=None, geom=None):
    """gt_rows float64 [G][7] = x, y, w, h, area, category, iscrowd; dets = (boxes f32 [K,4] normalised, scores f32 [K], cls [K]) taken
    through ingest() with `geom`, or None."""
    g = np.asarray(gt_rows, dtype=np.float64).reshape(-1, 7)
    im = {"id": int(image_id), "gt": g[:, :5].copy(), "gt_cat": g[:, 5].astype(np.int64), "gt_crowd": g[:, 6].astype(np.int64)}
    if dets is None:
        im["dt"], im["dt_score"], im["dt_cat"] = np.zeros((0, 4)), np.zeros(0), np.zeros(0, dtype=np.int64)
    else:
        im["dt"], im["dt_score"] = ingest(dets[0], dets[1], geom)
        im["dt_cat"] = np.asarray(dets[2]).astype(np.int64).reshape(-1)
    return im
