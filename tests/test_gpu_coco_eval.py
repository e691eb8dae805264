"""yn_coco_* (kernels_coco.hip) against the host restatement of COCOeval (tests/coco_oracle.py) and the committed fixture
(tests/golden/coco_eval.npz).  Every comparison is == on float64 arrays; nothing is excluded (COCOeval's orders are fully determined,
so there is no tie carve-out)."""
import numpy as np
import pytest
import torch

import coco_oracle

pytestmark = pytest.mark.gpu

C = 80
AREAS = coco_oracle.default_params()["areaRng"]
THRS = coco_oracle.default_params()["iouThrs"]


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b)


def _images(ids, geoms, gts, dets):
    return [coco_oracle.image_from_arrays(ids[i], gts[i] if gts[i] is not None else np.zeros((0, 7)), dets[i], geoms[i])
            for i in range(len(ids))]


def _run(ids, geoms, gts, dets, num_classes=C, bs=None, order=None):
    from yolo_nano_amd import COCOEval
    ev = COCOEval(num_classes)
    order = list(range(len(ids))) if order is None else list(order)
    bs = bs or len(order)
    for s in range(0, len(order), bs):
        sel = order[s:s + bs]
        ev.add_host([dets[i] for i in sel], [geoms[i] for i in sel], [ids[i] for i in sel], [gts[i] for i in sel])
    stats = ev.compute()
    return ev, stats


def _check_bits(ev, images, add_order, num_classes):
    """the store and the per-detection match / ignore bits of every (image, category, area range) against oracle.evaluate_img"""
    det, seg, matched, ignored = ev.matches()
    assert seg[-1] == len(det) == ev.size()[0]
    seen = 0
    for pos, i in enumerate(add_order):
        im = images[i]
        for k in range(num_classes):
            s, e = seg[pos * num_classes + k], seg[pos * num_classes + k + 1]
            gsel, dsel = im["gt_cat"] == k, im["dt_cat"] == k
            kept = min(int(dsel.sum()), 100)
            assert e - s == kept, (i, k)
            if kept == 0:
                continue
            for a, rng in enumerate(AREAS):
                o = coco_oracle.evaluate_img(im["dt"][dsel], im["dt_score"][dsel], im["gt"][gsel], im["gt_crowd"][gsel], rng, THRS, 100)
                assert np.array_equal(matched[a][:, s:e], o["matched"]), (i, k, a)
                assert np.array_equal(ignored[a][:, s:e], o["dt_ig"]), (i, k, a)
            want = im["dt"][dsel][o["order"]]
            d = det[s:e].astype(np.float64)
            got = np.stack([d[:, 0], d[:, 1], d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]], 1)
            assert np.array_equal(got, want) and np.array_equal(d[:, 4], np.asarray(o["scores"])), (i, k)
            seen += kept
    assert seen == len(det)


def _check(ev, stats, images, num_classes=C, add_order=None, bits=True):
    ostats, oprec, orec, _ = coco_oracle.coco_eval(images, num_classes)
    assert _same(ev.precision, oprec)
    assert _same(ev.recall, orec)
    assert _same(stats, ostats)
    if bits:
        _check_bits(ev, images, list(range(len(images))) if add_order is None else add_order, num_classes)


def _fixture(g):
    n = len(g["image_ids"])
    gts = [g["gt"][g["gt_off"][i]:g["gt_off"][i + 1]] for i in range(n)]
    dets = [(g["boxes"][g["offsets"][i]:g["offsets"][i + 1]], g["scores"][g["offsets"][i]:g["offsets"][i + 1]],
             g["classes"][g["offsets"][i]:g["offsets"][i + 1]]) for i in range(n)]
    return g["image_ids"].tolist(), [tuple(int(v) for v in r) for r in g["geoms"]], gts, dets


def test_fixture_parity(golden):
    g = golden("coco_eval.npz")
    ids, geoms, gts, dets = _fixture(g)
    ev, stats = _run(ids, geoms, gts, dets)
    assert _same(ev.precision, g["precision"])
    assert _same(ev.recall, g["recall"])
    assert _same(stats, g["stats"])
    assert ev.size()[1] == len(ids)
    ev.reset()
    assert ev.size() == (0, 0)
    ev.close()


def test_fixture_match_bits(golden):
    ids, geoms, gts, dets = _fixture(golden("coco_eval.npz"))
    ev, stats = _run(ids, geoms, gts, dets, bs=9)
    _check_bits(ev, _images(ids, geoms, gts, dets), list(range(len(ids))), C)


def _square(side=512):
    return (side, side, side, side, 0, 0, side)


def _workload(rng, n_img, num_classes, per_img, gt_per_img=8, side=512):
    """square side x side images (normalised = pixel / side, exact), integer boxes on a grid of 4 (equal IoUs), scores on a grid of
    1/32 (ties inside and across images), crowd boxes, annotation areas off w * h"""
    ids = [int(v) for v in rng.permutation(100000)[:n_img]]
    geoms, gts, dets = [], [], []
    for i in range(n_img):
        geoms.append(_square(side))
        m = int(rng.integers(0, gt_per_img + 1))
        w, h = rng.integers(2, 40, m) * 4, rng.integers(2, 40, m) * 4
        x, y = rng.integers(0, (side - 160) // 4, m) * 4, rng.integers(0, (side - 160) // 4, m) * 4
        gt = np.stack([x, y, w, h, w * h * rng.uniform(0.3, 1.0, m), rng.integers(0, num_classes, m), rng.random(m) < 0.15], 1).astype(np.float64)
        gts.append(gt.reshape(-1, 7))
        n = per_img
        if m:
            src = gt[rng.integers(0, m, n)]
            pix = np.stack([src[:, 0], src[:, 1], src[:, 0] + src[:, 2], src[:, 1] + src[:, 3]], 1) + rng.integers(-3, 4, (n, 4)) * 4
            cls = np.where(rng.random(n) < 0.8, src[:, 5], rng.integers(0, num_classes, n))
        else:
            pix = np.zeros((n, 4))
            cls = rng.integers(0, num_classes, n)
        rnd = rng.random(n) < (0.3 if m else 1.0)
        p0 = rng.integers(0, side // 4, (int(rnd.sum()), 2)) * 4
        pix[rnd] = np.concatenate([p0, p0 + rng.integers(0, 50, (int(rnd.sum()), 2)) * 4], 1)      # zero-area boxes among them
        dets.append(((pix / side).astype(np.float32), (rng.integers(1, 33, n) / 32.0).astype(np.float32), cls.astype(np.int64)))
    return ids, geoms, gts, dets


def test_random_ties_batching_and_add_order():
    rng = np.random.default_rng(11)
    NC = 6                                                   # few categories: long (image, category) lists, some over 100
    ids, geoms, gts, dets = _workload(rng, 60, NC, 260)
    images = _images(ids, geoms, gts, dets)
    results = []
    for bs in (1, 7, 32):
        ev, stats = _run(ids, geoms, gts, dets, NC, bs=bs)
        results.append((ev.precision.copy(), ev.recall.copy(), stats.copy()))
        if bs == 7:
            _check(ev, stats, images, NC)
        ev.close()
    order = [int(v) for v in rng.permutation(len(ids))]
    ev, stats = _run(ids, geoms, gts, dets, NC, bs=13, order=order)
    results.append((ev.precision.copy(), ev.recall.copy(), stats.copy()))
    _check_bits(ev, images, order, NC)
    for r in results[1:]:
        assert all(_same(a, b) for a, b in zip(r, results[0]))
    assert max(np.bincount(d[2], minlength=NC).max() for d in dets) > 100
    assert -1 < results[0][2][0] < 1


def _pix(boxes_xyxy, scores, cls, side=512):
    return ((np.asarray(boxes_xyxy, dtype=np.float64).reshape(-1, 4) / side).astype(np.float32), np.asarray(scores, dtype=np.float32),
            np.asarray(cls, dtype=np.int64))


def test_edges():
    from yolo_nano_amd import COCOEval, YnError, YnRangeError
    NC = 5
    none = _pix(np.zeros((0, 4)), [], [])
    gt1 = np.array([[10, 10, 40, 40, 1600, 0, 0]], dtype=np.float64)
    # no detections at all: precision 0 and recall 0 where there is ground truth, -1 elsewhere
    ev, stats = _run([5, 2], [_square()] * 2, [gt1, None], [none, none], NC)
    _check(ev, stats, _images([5, 2], [_square()] * 2, [gt1, None], [none, none]), NC)
    assert (ev.precision[:, :, 0, 0, :] == 0).all() and (ev.recall[:, 0, 0, :] == 0).all() and (ev.precision[:, :, 1:] == -1).all()
    # no ground truth at all: everything -1
    d = _pix([[10, 10, 50, 50], [0, 0, 8, 8]], [.9, .8], [0, 3])
    ev, stats = _run([5], [_square()], [None], [d], NC)
    assert (ev.precision == -1).all() and (ev.recall == -1).all() and (stats == -1).all()
    _check(ev, stats, _images([5], [_square()], [None], [d]), NC)
    # one image: zero-area detection on a zero-area ground truth (IoU 0 by bbIou's early exit), a detection wholly inside a crowd box
    # (IoU = 1 against the crowd, ignored), equal IoU 0.6 against two boxes, 150 ground truths of one category (three lane chunks)
    gx = np.arange(150) * 3.0
    gt = np.concatenate([
        np.array([[5, 5, 0, 0, 0, 0, 0], [20, 20, 40, 40, 1600, 0, 0],
                  [100, 100, 200, 200, 30000, 1, 1], [400, 400, 20, 20, 400, 1, 0],
                  [100, 100, 40, 40, 1600, 2, 0], [120, 100, 40, 40, 1600, 2, 0]], dtype=np.float64),
        np.stack([gx, gx * 0 + 480, gx * 0 + 2, gx * 0 + 2, gx * 0 + 4, gx * 0 + 3, (np.arange(150) % 50 == 7) * 1.0], 1)])
    d = _pix([[5, 5, 5, 5], [20, 20, 60, 60], [150, 150, 170, 170], [120, 120, 140, 140], [400, 400, 420, 420],
              [110, 100, 150, 140], [110, 100, 150, 140], [110, 100, 150, 140],
              [300, 480, 302, 482], [420, 480, 422, 482], [300, 480, 302, 482], [21, 480, 23, 482]],
             [.95, .5, .9, .9, .3, .9, .8, .7, .9, .8, .7, .6], [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3])
    ev, stats = _run([77], [_square()], [gt], [d], NC)
    images = _images([77], [_square()], [gt], [d])
    _check(ev, stats, images, NC)
    det, seg, matched, ignored = ev.matches()
    assert matched[0][0][seg[0]:seg[1]].tolist() == [False, True]                    # category 0: the zero-area pair does not match
    assert matched[0][:, seg[1]:seg[2]].all() and ignored[0][0][seg[1]:seg[2]].tolist() == [True, True, False]
    assert matched[0][0][seg[2]:seg[3]].tolist() == [True, True, False]
    assert matched[0][0][seg[3]:seg[4]].tolist() == [True, True, False, True] and ignored[0][0][seg[3]:seg[4]].tolist() == [False] * 3 + [True]
    # the split-f16 range mark: offsets[B] negative -> YnRangeError, nothing added; a repeated image id is refused by name
    n0 = ev.size()
    rec = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    off = torch.tensor([0, 2, -1 - 4], dtype=torch.int32, device="cuda")
    with pytest.raises(YnRangeError):
        ev.add(rec, off, [_square()] * 2, [1, 2], [None, None])
    assert ev.size() == n0
    ev.add_host([none], [_square()], [77], [None])
    with pytest.raises(YnError, match="image id"):
        ev.compute()
    ev.close()
    # a category outside 0..C-1 and a non-finite box are reported by compute()
    for bad in (_pix([[0, 0, 8, 8]], [.5], [NC]), (np.array([[0, 0, np.inf, 1]], np.float32), np.array([.5], np.float32), np.array([0]))):
        ev = COCOEval(NC)
        ev.add_host([bad], [_square()], [1], [gt1])
        with pytest.raises(YnError):
            ev.compute()
        ev.close()
    ev = COCOEval(NC)
    with pytest.raises(YnError, match="4096"):
        ev.add_host([none], [_square()], [1], [np.tile(gt1, (4097, 1))])
    ev.close()


def test_evaluate_coco_end_to_end():
    import yolo_nano_amd
    from yolo_nano_amd import arch, weights, evaluate_coco, ValTransforms, voc_geometry, coco_gt_arrays
    S = 416
    sd = weights.make_state_dict("1.0x", C)
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, conf_thresh=0.001, nms_thresh=0.5, anchor_size=arch.MULTI_ANCHOR_SIZE_COCO)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to("cuda").eval()
    rng = np.random.default_rng(9)
    shapes = [(240, 320), (320, 240), (256, 256), (300, 500), (500, 300)]
    images = [rng.integers(0, 256, shapes[i % 5] + (3,), dtype=np.uint8) for i in range(8)]
    image_ids = [int(v) for v in rng.permutation(5000)[:8] + 1]
    # the host route: forward_batch's triples for the same frames, cocoapi_evaluator.py:85-99 restated by the oracle
    tf = ValTransforms(S)
    triples = []
    for s in range(0, len(images), 5):
        triples += m.forward_batch(tf.batch(images[s:s + 5])[0])
    geoms = [voc_geometry(im.shape[0], im.shape[1], S) for im in images]
    assert sum(len(t[1]) for t in triples) > 1000
    # ground truth as a COCO annotation dict: some of the detections' own boxes, jittered, plus a crowd box per image
    anns, cats = [], [{"id": 3 * k + 1} for k in range(C)]
    for i, t in enumerate(triples):
        box, _ = coco_oracle.ingest(t[0], t[1], geoms[i])
        for j in rng.permutation(len(box))[:6]:
            x, y, w, h = (box[j] + rng.normal(0, 1.5, 4)).tolist()
            anns.append({"id": len(anns) + 1, "image_id": image_ids[i], "category_id": 3 * int(t[2][j]) + 1,
                         "bbox": [x, y, max(w, 1.0), max(h, 1.0)], "area": max(w, 1.0) * max(h, 1.0) * 0.7, "iscrowd": 0})
        h0, w0 = images[i].shape[:2]
        anns.append({"id": len(anns) + 1, "image_id": image_ids[i], "category_id": 3 * int(t[2][0]) + 1,
                     "bbox": [0.0, 0.0, w0 / 2, h0 / 2], "area": w0 * h0 / 8.0, "iscrowd": 1})
    gts, gt_ids, cat_ids = coco_gt_arrays({"images": [{"id": v} for v in image_ids], "annotations": anns, "categories": cats})
    assert gt_ids == image_ids and cat_ids == [3 * k + 1 for k in range(C)]
    ap50, ap50_95 = evaluate_coco(m, images, image_ids, gts, batch=5)
    ostats = coco_oracle.coco_eval(_images(image_ids, geoms, gts, triples), C)[0]
    assert ap50 == ostats[1] and ap50_95 == ostats[0]
    assert ap50 > 0
