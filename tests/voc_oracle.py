"""Host restatement of the VOC metric of evaluator/vocapi_evaluator.py, with the stable tie rule of yn_eval: among equal 3-decimal
scores of one class, detections keep file order (image in add order, then position in the image's list).  Used by the CPU test
(against the reference's own voc_eval, tests/golden/voc_eval.npz) and by the GPU tests (against yn_eval_*)."""
import numpy as np


def geometry_arrays(geom):
    """(scale, offset, size) exactly as ValTransforms.geometry / the evaluator build them from one (w0, h0, rw, rh, left, top, side)."""
    w0, h0, rw, rh, left, top, side = [int(v) for v in geom]
    if h0 > w0:
        scale, offset = np.array([[rw / side, 1., rw / side, 1.]]), np.array([[left / side, 0., left / side, 0.]])
    elif h0 < w0:
        scale, offset = np.array([1., rh / side, 1., rh / side]), np.array([[0., top / side, 0., top / side]])
    else:
        scale, offset = 1., np.zeros([1, 4])
    return scale, offset, np.array([[w0, h0, w0, h0]])


def text_route(boxes, scores, geom):
    """Normalised float32 boxes [K,4] + scores [K] of one image -> what the results file keeps: (score bin k [K], tenths [K,4]) with
    score = float('%.3f') = k / 1000 and coordinate = float('%.1f' of box + 1) = tenths / 10, through real format / parse."""
    scale, offset, size = geometry_arrays(geom)
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    b -= offset
    b /= scale
    b *= size
    dets = np.hstack((b, np.asarray(scores, dtype=np.float32).reshape(-1, 1))).astype(np.float32, copy=False)
    ks = np.zeros(len(dets), dtype=np.int64)
    tn = np.zeros((len(dets), 4), dtype=np.int64)
    for i in range(len(dets)):
        line = '{:.3f} {:.1f} {:.1f} {:.1f} {:.1f}'.format(dets[i, -1], dets[i, 0] + 1, dets[i, 1] + 1, dets[i, 2] + 1, dets[i, 3] + 1)
        f = [float(z) for z in line.split(' ')]
        ks[i] = int(round(f[0] * 1000))
        tn[i] = [int(round(v * 10)) for v in f[1:]]
    return ks, tn


def pairwise_sum(a):
    """numpy's pairwise summation of a contiguous float64 vector (the order yn_eval's area AP restates on the device)."""
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res += v
        return res
    if n <= 128:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] += a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += a[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def numpy_sum(a):
    """np.sum of a 1-d float64 array: 0.0 plus the pairwise sum of each 8192-element block"""
    a = [float(v) for v in a]
    res = 0.0
    for s in range(0, len(a), 8192):
        res += pairwise_sum(a[s:s + 8192])
    return res


def average_precision(rec, prec, use_07_metric):
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            sel = prec[rec >= t]
            ap = ap + (np.max(sel) if sel.size else 0) / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    idx = np.where(mrec[1:] != mrec[:-1])[0]
    return numpy_sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1])


def voc_metric(records, gt, gt_off, num_classes, ovthresh=0.5, use_07_metric=True):
    """records int [n][7] = image, class, k, x1..y2 tenths in file order; gt int [G][6] = x1, y1, x2, y2, class, difficult per image
    (gt_off [I+1]).  -> (aps [C], curves: list of (rec, prec) or (-1., -1.), npos [C])."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, 7)
    gt = np.asarray(gt, dtype=np.int64).reshape(-1, 6)
    n_img = len(gt_off) - 1
    aps, curves, nposs = [], [], []
    for c in range(num_classes):
        boxes, diff, npos = [], [], 0
        for i in range(n_img):
            g = gt[gt_off[i]:gt_off[i + 1]]
            g = g[g[:, 4] == c]
            boxes.append(g[:, :4].astype(float))
            diff.append(g[:, 5].astype(bool))
            npos += int((~diff[-1]).sum())
        nposs.append(npos)
        r = records[records[:, 1] == c]
        if len(r) == 0:
            aps.append(-1.)
            curves.append((-1., -1.))
            continue
        conf = r[:, 2] / 1000.0
        bb = r[:, 3:7] / 10.0
        order = np.argsort(-conf, kind='stable')
        claimed = [np.zeros(len(b), dtype=bool) for b in boxes]
        nd = len(order)
        tp, fp = np.zeros(nd), np.zeros(nd)
        for d, j in enumerate(order):
            im = int(r[j, 0])
            det = bb[j]
            G = boxes[im]
            best = -np.inf
            if G.size > 0:
                iw = np.maximum(np.minimum(G[:, 2], det[2]) - np.maximum(G[:, 0], det[0]), 0.)
                ih = np.maximum(np.minimum(G[:, 3], det[3]) - np.maximum(G[:, 1], det[1]), 0.)
                inters = iw * ih
                uni = (det[2] - det[0]) * (det[3] - det[1]) + (G[:, 2] - G[:, 0]) * (G[:, 3] - G[:, 1]) - inters
                with np.errstate(invalid='ignore', divide='ignore'):
                    ov = inters / uni
                best, arg = np.max(ov), np.argmax(ov)
            if best > ovthresh:
                if diff[im][arg]:
                    continue
                if claimed[im][arg]:
                    fp[d] = 1.
                else:
                    tp[d] = 1.
                    claimed[im][arg] = True
            else:
                fp[d] = 1.
        fp, tp = np.cumsum(fp), np.cumsum(tp)
        with np.errstate(invalid='ignore', divide='ignore'):
            rec = tp / float(npos)
        prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
        aps.append(average_precision(rec, prec, use_07_metric))
        curves.append((rec, prec))
    return np.array(aps, dtype=np.float64), curves, np.array(nposs, dtype=np.int64)


def ingest(boxes, scores, classes, offsets, geoms):
    """The text route for a whole record list (offsets [B+1] over images) -> int64 [n][7] as yn_eval_records returns it."""
    out = []
    for b in range(len(offsets) - 1):
        s, e = offsets[b], offsets[b + 1]
        ks, tn = text_route(boxes[s:e], scores[s:e], geoms[b])
        rows = np.zeros((e - s, 7), dtype=np.int64)
        rows[:, 0] = b
        rows[:, 1] = np.asarray(classes[s:e], dtype=np.int64)
        rows[:, 2] = ks
        rows[:, 3:] = tn
        out.append(rows)
    return np.concatenate(out) if out else np.zeros((0, 7), dtype=np.int64)
