"""yn_eval_* (kernels_eval.hip) against the reference's voc_eval (tests/golden/voc_eval.npz) and the host oracle with the stable tie
rule (tests/voc_oracle.py): every comparison is exact (NaN where the reference gives NaN)."""
import numpy as np
import pytest
import torch

import voc_oracle

pytestmark = pytest.mark.gpu

C = 20


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _split(boxes, scores, classes, offsets):
    return [(boxes[offsets[b]:offsets[b + 1]], scores[offsets[b]:offsets[b + 1]], classes[offsets[b]:offsets[b + 1]])
            for b in range(len(offsets) - 1)]


def _gts(gt, gt_off):
    return [gt[gt_off[b]:gt_off[b + 1]] for b in range(len(gt_off) - 1)]


def _check_against_oracle(ev, recs, gt, gt_off, num_classes=C):
    for use07 in (True, False):
        aps, m = ev.compute(use07)
        raps, rcurves, rnpos = voc_oracle.voc_metric(recs, gt, gt_off, num_classes, ev.ovthresh, use07)
        assert _same(aps, raps), (use07, aps, raps)
        assert _same(m, np.mean(raps))
        assert np.array_equal(ev.npos, rnpos)
        for c in range(num_classes):
            r, p = ev.curve(c)
            if np.ndim(rcurves[c][0]) == 0:
                assert (r, p) == (-1., -1.)
            else:
                assert _same(r, rcurves[c][0]) and _same(p, rcurves[c][1]), c
    return aps


def test_fixture_parity(golden):
    from yolo_nano_amd import VOCEval
    g = golden("voc_eval.npz")
    ev = VOCEval(C)
    ev.add_host(_split(g["boxes"], g["scores"], g["classes"], g["offsets"]), g["geoms"], _gts(g["gt"], g["gt_off"]))
    off = g["curve_off"]
    for tag, use07 in (("07", True), ("area", False)):
        aps, m = ev.compute(use07)
        assert _same(aps, g["ap_" + tag]) and _same(m, g["map_" + tag]), tag
        for c in range(C):
            r, p = ev.curve(c)
            if off[c + 1] == off[c]:
                assert (r, p) == (-1., -1.)
            else:
                assert _same(r, g["rec_" + tag][off[c]:off[c + 1]]) and _same(p, g["prec_" + tag][off[c]:off[c + 1]]), (tag, c)
    assert ev.ndet[18] == 0 and ev.npos[19] == 0


GEOMS = [(375, 500, 1024), (500, 333, 416), (640, 640, 320)]        # wide, tall, square: (h0, w0, side)


def test_ingest_matches_text_route():
    from yolo_nano_amd import VOCEval, voc_geometry
    rng = np.random.default_rng(3)
    dets, geoms = [], []
    for h0, w0, side in GEOMS:
        g = voc_geometry(h0, w0, side)
        scale, offset, size = voc_oracle.geometry_arrays(g)
        sc = np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1), (4,))
        # pixel values on the .x5 boundaries (box + 1 = m + 0.05), and their float32 neighbours after the round trip
        pix = (rng.integers(-30, max(h0, w0), 400) + 0.05 + rng.integers(0, 10, 400) / 10.0 - 1.0)
        norm = []
        for q in range(400):
            ax = q % 4
            v = np.float32(pix[q] / size.reshape(-1)[ax] * sc[ax] + offset.reshape(-1)[ax])
            norm.append([v, np.nextafter(v, np.float32(2)), np.nextafter(v, np.float32(-2))][q % 3])
        boxes = np.array(norm, dtype=np.float32).reshape(-1, 4)
        boxes = np.concatenate([boxes, rng.uniform(-0.2, 1.1, (200, 4)).astype(np.float32)])   # margins: negative pixels
        n = len(boxes)
        k = rng.integers(0, 1000, n)
        s = ((k + 0.5) / 1000.0).astype(np.float32)                  # the .0005 boundaries and their neighbours
        s = np.where(np.arange(n) % 3 == 1, np.nextafter(s, np.float32(2)), np.where(np.arange(n) % 3 == 2, np.nextafter(s, np.float32(-2)), s))
        s = np.clip(s, 0, 1).astype(np.float32)
        s[:3] = [0.0, 1.0, np.float32(0.0004999)]
        dets.append((boxes, s, rng.integers(0, C, n)))
        geoms.append(g)
    ev = VOCEval(C)
    ev.add_host(dets, geoms, [None] * len(dets))
    got = ev.records()
    off = np.cumsum([0] + [len(d[1]) for d in dets])
    want = voc_oracle.ingest(np.concatenate([d[0] for d in dets]), np.concatenate([d[1] for d in dets]),
                             np.concatenate([d[2] for d in dets]), off, geoms)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert (got[:, 3:] < 10).any()                                 # some coordinates land left of / above the image


def _workload(rng, n_img, per_img, tie_bins, gt_per_img=6, w=500, h=375):
    geoms, gts, dets = [], [], []
    for i in range(n_img):
        hh, ww = (h, w) if i % 3 == 0 else ((w, h) if i % 3 == 1 else (h, h))
        side = 416
        g = voc_geometry_np(hh, ww, side)
        geoms.append(g)
        m = int(rng.integers(0, gt_per_img + 1))
        x1 = rng.integers(0, ww - 60, m); y1 = rng.integers(0, hh - 60, m)
        gt = np.stack([x1, y1, x1 + rng.integers(10, 60, m), y1 + rng.integers(10, 60, m), rng.integers(0, C, m),
                       (rng.random(m) < 0.2).astype(int)], 1).astype(np.int32) if m else np.zeros((0, 6), np.int32)
        gts.append(gt)
        scale, offset, size = voc_oracle.geometry_arrays(g)
        sc = np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1), (4,))
        n = per_img
        src = gt[rng.integers(0, m, n)] if m else np.zeros((n, 6), np.int32)
        pix = src[:, :4] + rng.normal(0, 6, (n, 4))
        rnd = rng.random(n) < 0.3
        pix[rnd] = rng.uniform(0, min(ww, hh), (int(rnd.sum()), 4))
        cls = np.where(rng.random(n) < 0.8, src[:, 4], rng.integers(0, C, n)) if m else rng.integers(0, C, n)
        norm = (pix / size.reshape(-1)) * sc + offset.reshape(-1)
        s = (rng.integers(1000 - tie_bins, 1001, n) / 1000.0).astype(np.float32)
        dets.append((norm.astype(np.float32), s, cls))
    return dets, geoms, gts


def voc_geometry_np(h0, w0, side):
    from yolo_nano_amd import voc_geometry
    return voc_geometry(h0, w0, side)


def _records_of(dets, geoms):
    off = np.cumsum([0] + [len(d[1]) for d in dets])
    return voc_oracle.ingest(np.concatenate([d[0] for d in dets]), np.concatenate([d[1] for d in dets]),
                             np.concatenate([d[2] for d in dets]), off, geoms)


def _gt_concat(gts):
    gt_off = np.cumsum([0] + [len(g) for g in gts])
    return np.concatenate(gts), gt_off


def test_ties_and_scale_and_batching():
    from yolo_nano_amd import VOCEval
    rng = np.random.default_rng(11)
    dets, geoms, gts = _workload(rng, 200, 300, tie_bins=12)
    recs = _records_of(dets, geoms)
    gt, gt_off = _gt_concat(gts)
    results = []
    for bs in (1, 7, 32):
        ev = VOCEval(C)
        for s in range(0, len(dets), bs):
            ev.add_host(dets[s:s + bs], geoms[s:s + bs], gts[s:s + bs])
        assert ev.size() == (len(recs), len(dets))
        assert np.array_equal(ev.records(), recs)
        results.append([ev.compute(u)[0] for u in (True, False)])
        if bs == 7:
            _check_against_oracle(ev, recs, gt, gt_off)
    for r in results[1:]:
        assert all(_same(a, b) for a, b in zip(r, results[0]))


def _square(n_img=1, side=1024):
    return [(side, side, side, side, 0, 0, side)] * n_img


def _dets_from_eval_coords(boxes_eval, scores, cls, side=1024):
    """detections given in the evaluator's frame (pixel + 1), on a square side x side image: norm = (coord - 1) / side exactly"""
    b = (np.asarray(boxes_eval, dtype=np.float64) - 1.0) / side
    return (b.astype(np.float32), np.asarray(scores, dtype=np.float32), np.asarray(cls))


def test_edges():
    from yolo_nano_amd import VOCEval
    ims, gts = [], []
    # image 0, class 0: IoU exactly 0.5 is not a match; a duplicate of a claimed GT is FP; a difficult GT's match is neither
    gts.append(np.array([[0, 0, 10, 10, 0, 0], [100, 100, 120, 120, 0, 0], [200, 200, 220, 220, 0, 1]], np.int32))
    ims.append(_dets_from_eval_coords([[0, 0, 20, 10], [100, 100, 120, 120], [100, 100, 120, 120.5], [200, 200, 220, 220]],
                                      [0.9, 0.8, 0.7, 0.6], [0, 0, 0, 0]))
    # image 1, class 1: zero-area detection on a zero-area GT (0/0 = NaN -> FP), then a normal match
    gts.append(np.array([[5, 5, 5, 5, 1, 0], [20, 20, 40, 40, 1, 0]], np.int32))
    ims.append(_dets_from_eval_coords([[5, 5, 5, 5], [20, 20, 40, 40]], [0.95, 0.5], [1, 1]))
    # image 2, class 2: 150 GT in one (image, class); hits on GT 100 and 140, and a duplicate
    gx = np.arange(150) * 6
    gts.append(np.stack([gx, gx * 0, gx + 5, gx * 0 + 5, gx * 0 + 2, gx * 0], 1).astype(np.int32))
    ims.append(_dets_from_eval_coords([[600, 0, 605, 5], [840, 0, 845, 5], [600, 0, 605, 5]], [0.9, 0.8, 0.7], [2, 2, 2]))
    # image 3, class 3: one segment of 5000 detections; class 4: difficult GT only (npos = 0)
    rng = np.random.default_rng(5)
    g3 = np.array([[10 + 30 * j, 10, 35 + 30 * j, 40, 3, int(j % 4 == 0)] for j in range(20)] + [[500, 500, 540, 540, 4, 1]], np.int32)
    gts.append(g3)
    src = g3[rng.integers(0, 20, 5000), :4] + np.round(rng.normal(0, 3, (5000, 4)), 1)
    b = np.concatenate([src, [[500, 500, 540, 540], [501, 500, 540, 540]]])
    ims.append(_dets_from_eval_coords(b, np.concatenate([rng.integers(0, 1001, 5000) / 1000.0, [0.5, 0.4]]), [3] * 5000 + [4, 4]))
    geoms = _square(len(ims))
    ev = VOCEval(C)
    ev.add_host(ims, geoms, gts)
    recs = _records_of(ims, geoms)
    gt, gt_off = _gt_concat(gts)
    assert np.array_equal(ev.records(), recs)
    aps = _check_against_oracle(ev, recs, gt, gt_off)
    assert ev.ndet[3] == 5000 and ev.npos[4] == 0 and np.isnan(aps[4])       # area metric: rec is NaN throughout
    assert ev.compute(True)[0][4] == 0.0
    r, p = ev.curve(0)                                          # FP (IoU 0.5), TP, FP (duplicate), neither (difficult)
    assert np.array_equal(r, [0, 0.5, 0.5, 0.5]) and np.array_equal(p, [0, 0.5, 1 / 3, 1 / 3])
    r, p = ev.curve(1)
    assert np.isclose(r[-1], 0.5) and p[0] == 0.0
    r, p = ev.curve(2)
    assert np.array_equal(r, np.array([1., 2., 2.]) / 150.)
    # the split-f16 range mark: offsets[B] negative -> YnRangeError, nothing added
    from yolo_nano_amd import YnRangeError
    n0 = ev.size()
    rec = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    off = torch.tensor([0, 2, -1 - 4], dtype=torch.int32, device="cuda")
    with pytest.raises(YnRangeError):
        ev.add(rec, off, _square(2), [None, None])
    assert ev.size() == n0


def test_evaluate_end_to_end():
    import yolo_nano_amd
    from yolo_nano_amd import arch, weights, evaluate, ValTransforms, rescale_boxes, voc_geometry
    S = 320
    sd = weights.make_state_dict("1.0x", C)
    for hd in (1, 2, 3):                                       # YOLONano.init_bias (models/yolo_nano.py:77-83)
        sd["head_det_%d.4.bias" % hd][:3] = -4.595
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, conf_thresh=0.001, nms_thresh=0.5, anchor_size=arch.MULTI_ANCHOR_SIZE)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to("cuda").eval()
    rng = np.random.default_rng(9)
    shapes = [(240, 320), (320, 240), (256, 256), (300, 500), (500, 300)]
    images = [rng.integers(0, 256, shapes[i % 5] + (3,), dtype=np.uint8) for i in range(64)]
    annots = []
    for im in images:
        h0, w0 = im.shape[:2]
        k = int(rng.integers(0, 5))
        x1, y1 = rng.integers(0, w0 - 50, k), rng.integers(0, h0 - 50, k)
        annots.append(np.stack([x1, y1, x1 + rng.integers(5, 50, k), y1 + rng.integers(5, 50, k), rng.integers(0, C, k),
                                (rng.random(k) < 0.1).astype(int)], 1).astype(np.int32).reshape(-1, 6))
    got07 = evaluate(m, images, annots, batch=32, use_07_metric=True)
    got = evaluate(m, images, annots, batch=32, use_07_metric=False)
    # host route: forward per image, rescale_boxes, the results-file text, the stable oracle
    tf = ValTransforms(S)
    rows = []
    for i, im in enumerate(images):
        x, _, _, scale, offset = tf(im)
        bboxes, scores, cls_inds = m(x.unsqueeze(0))
        h0, w0 = im.shape[:2]
        b = rescale_boxes(bboxes.copy(), scale, offset, np.array([[w0, h0, w0, h0]]))
        dets = np.hstack((b, scores[:, None])).astype(np.float32, copy=False)
        for j in range(len(dets)):
            f = [float(z) for z in '{:.3f} {:.1f} {:.1f} {:.1f} {:.1f}'.format(
                dets[j, -1], dets[j, 0] + 1, dets[j, 1] + 1, dets[j, 2] + 1, dets[j, 3] + 1).split(' ')]
            rows.append([i, int(cls_inds[j]), int(round(f[0] * 1000))] + [int(round(v * 10)) for v in f[1:]])
        assert voc_geometry(h0, w0, S)[2:6] == tuple(int(v) for v in tf.geometry(h0, w0)[:4])
    assert len(rows) > 0
    gt, gt_off = _gt_concat(annots)
    for use07, (aps, mAP) in ((True, got07), (False, got)):
        raps = voc_oracle.voc_metric(np.array(rows), gt, gt_off, C, 0.5, use07)[0]
        assert _same(aps, raps) and _same(mAP, np.mean(raps)), use07
