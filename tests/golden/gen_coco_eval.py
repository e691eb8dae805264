"""Generate tests/golden/coco_eval.npz: a synthetic COCO-style set and its COCOeval('bbox') result, for tests/test_coco_eval_cpu.py
and tests/test_gpu_coco_eval.py.

    python tests/golden/gen_coco_eval.py

When pycocotools can be imported, the result comes from pycocotools.COCOeval and the host restatement tests/coco_oracle.py is
asserted equal to it, bit for bit (precision, recall and the 12 stats): running this script where the library is installed is how
the parity gap is closed.  Otherwise the restatement produces the file.  `source` in the file says which of the two did.

40 images (wide, tall, square) with unsorted, non-contiguous ids, 80 categories.  Covered on purpose: crowd boxes with several
detections inside, ground truth in every area range with annotation areas that differ from w*h (some across a range boundary),
categories without ground truth (75..79; 75 and 76 have detections), categories without detections (70..74), images without ground
truth, without detections and without either, more than 100 detections in one (image, category), scores on a coarse grid (ties
inside an image and across images), and on the square images integer boxes with equal IoUs against two ground truths.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))

import coco_oracle                                           # noqa: E402

C = 80
N_IMG = 40


def geometry(h0, w0, side):
    """Resize's integer geometry (ValTransforms.geometry) for a side x side square"""
    if h0 > w0:
        rw, rh = int(w0 / h0 * side), side
        return (w0, h0, rw, rh, (rh - rw) // 2, 0, side)
    if h0 < w0:
        rw, rh = side, int(h0 / w0 * side)
        return (w0, h0, rw, rh, 0, (rw - rh) // 2, side)
    return (w0, h0, side, side, 0, 0, side)


def normalise(pix_xyxy, geom):
    scale, offset, size = coco_oracle.geometry_arrays(geom)
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1), (4,))
    return ((np.asarray(pix_xyxy, dtype=np.float64) / size.reshape(-1)) * sc + offset.reshape(-1)).astype(np.float32)


def make():
    rng = np.random.default_rng(20261016)
    shapes = [(480, 640), (640, 480), (512, 512), (375, 500), (500, 333), (427, 640)]
    ids = [int(v) for v in rng.permutation(np.arange(3, 900000, 7919))[:N_IMG]]
    geoms, gts, dets = [], [], []
    for i in range(N_IMG):
        h0, w0 = shapes[i % len(shapes)]
        square = h0 == w0
        geom = geometry(h0, w0, 512 if square else 416)
        geoms.append(geom)
        g = []
        if i % 9 not in (4, 7):                              # images 4, 7, 13, 16, ...: no ground truth
            for _ in range(int(rng.integers(1, 9))):
                c = int(rng.integers(0, 75))
                kind = int(rng.integers(0, 3))               # small, medium, large by w * h
                lo_, hi_ = [(6, 30), (34, 90), (100, 300)][kind]
                w, h = int(rng.integers(lo_, hi_)), int(rng.integers(lo_, hi_))
                w, h = min(w, w0 - 2), min(h, h0 - 2)
                x, y = int(rng.integers(0, w0 - w)), int(rng.integers(0, h0 - h))
                crowd = int(rng.random() < 0.12)
                area = float(w * h) * float(rng.uniform(0.35, 1.0))      # the segmentation area, not w * h
                g.append([x, y, w, h, area, c, crowd])
            if i % 4 == 1:                                   # w * h in one area range, the annotation area in the one below
                g.append([10, 10, 40, 40, 900.0, 5, 0])
                g.append([200, 120, 100, 100, 9000.0, 6, 0])
        if i == 2:                                           # equal IoUs against two ground truths (0.6 each), integer boxes
            g.append([100, 100, 40, 40, 1500.0, 8, 0])
            g.append([120, 100, 40, 40, 1500.0, 8, 0])
            g.append([300, 300, 200, 150, 20000.0, 9, 1])    # a crowd box with detections inside it
        g = np.array(g, dtype=np.float64).reshape(-1, 7)
        gts.append(g)
        d = []                                               # (x1, y1, x2, y2, category)
        if i % 9 not in (5, 7):                              # images 5, 7, 14, 16, ...: no detections
            for row in g:
                reps = int(rng.integers(0, 4)) + (4 if row[6] else 0)
                for _ in range(reps):
                    if row[5] >= 70:
                        continue
                    if row[6]:                               # inside the crowd box
                        w, h = row[2] * rng.uniform(0.2, 0.6), row[3] * rng.uniform(0.2, 0.6)
                        x, y = row[0] + rng.uniform(0, row[2] - w), row[1] + rng.uniform(0, row[3] - h)
                    else:
                        jit = rng.normal(0, 0.1, 4) * np.array([row[2], row[3]] * 2)
                        x, y, w, h = row[0] + jit[0], row[1] + jit[1], max(row[2] + jit[2], 1.0), max(row[3] + jit[3], 1.0)
                    box = np.array([x, y, x + w, y + h])
                    if square:
                        box = np.round(box)
                    d.append((box, int(row[5]) if rng.random() < 0.85 else int(rng.integers(0, 77))))
            for _ in range(int(rng.integers(0, 6))):         # false positives anywhere, categories 75 and 76 included
                x, y = rng.uniform(-10, w0 - 20), rng.uniform(-10, h0 - 20)
                box = np.array([x, y, x + rng.uniform(5, 200), y + rng.uniform(5, 200)])
                d.append((np.round(box) if square else box, int(rng.integers(0, 77))))
            if i == 2:
                d += [(np.array([110., 100., 150., 140.]), 8)] * 3
                d += [(np.array([320. + 10 * j, 310., 360. + 10 * j, 350.]), 9) for j in range(6)]
            if i == 3:                                       # 130 detections of one category in one image
                for j in range(130):
                    x, y = rng.uniform(0, w0 - 60), rng.uniform(0, h0 - 60)
                    d.append((np.array([x, y, x + rng.uniform(8, 120), y + rng.uniform(8, 120)]), 3))
        d = [(b, c) for b, c in d if c < 70 or c in (75, 76)]
        boxes = normalise(np.array([b for b, _ in d]).reshape(-1, 4), geom)
        scores = (rng.integers(1, 64, len(d)) / 64.0).astype(np.float32)     # a coarse grid: ties everywhere
        dets.append((boxes, scores, np.array([c for _, c in d], dtype=np.int32)))
    return ids, np.array(geoms, dtype=np.int32), gts, dets


def oracle_images(ids, geoms, gts, dets):
    return [coco_oracle.image_from_arrays(ids[i], gts[i], dets[i], geoms[i]) for i in range(len(ids))]


def run_pycocotools(images):
    """pycocotools.COCOeval on the same data (category id = index + 1, annotation ids from 1) -> (stats, precision, recall)"""
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    gt = COCO()
    anns = []
    for im in images:
        for g in range(len(im["gt"])):
            x, y, w, h, area = [float(v) for v in im["gt"][g]]
            anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": int(im["gt_cat"][g]) + 1, "bbox": [x, y, w, h],
                         "area": area, "iscrowd": int(im["gt_crowd"][g])})
    gt.dataset = {"images": [{"id": im["id"]} for im in images], "annotations": anns,
                  "categories": [{"id": k + 1, "name": "c%d" % k} for k in range(C)]}
    gt.createIndex()
    res = []
    for im in images:
        for d in range(len(im["dt"])):
            res.append({"image_id": im["id"], "category_id": int(im["dt_cat"][d]) + 1, "bbox": [float(v) for v in im["dt"][d]],
                        "score": float(im["dt_score"][d])})
    dt = gt.loadRes(res)
    ev = COCOeval(gt, dt, "bbox")
    ev.params.imgIds = [im["id"] for im in images]
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return np.asarray(ev.stats, dtype=np.float64), ev.eval["precision"], ev.eval["recall"]


def main():
    ids, geoms, gts, dets = make()
    images = oracle_images(ids, geoms, gts, dets)
    stats, precision, recall, _ = coco_oracle.coco_eval(images, C)
    source = "oracle"
    try:
        import pycocotools  # noqa: F401
        have = True
    except ImportError:
        have = False
    if have:
        pstats, pprecision, precall = run_pycocotools(images)
        assert np.array_equal(precision, pprecision) and np.array_equal(recall, precall) and np.array_equal(stats, pstats), \
            "tests/coco_oracle.py differs from pycocotools"
        stats, precision, recall, source = pstats, pprecision, precall, "pycocotools"
    gt_off = np.zeros(len(gts) + 1, dtype=np.int32)
    gt_off[1:] = np.cumsum([len(g) for g in gts])
    offsets = np.zeros(len(dets) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(d[1]) for d in dets])
    np.savez_compressed(os.path.join(HERE, "coco_eval.npz"), image_ids=np.array(ids, dtype=np.int64), geoms=geoms,
                        gt=np.concatenate(gts), gt_off=gt_off, boxes=np.concatenate([d[0] for d in dets]),
                        scores=np.concatenate([d[1] for d in dets]), classes=np.concatenate([d[2] for d in dets]), offsets=offsets,
                        precision=precision, recall=recall, stats=stats, source=np.array(source))
    print("coco_eval.npz (%s): %d images, %d detections, %d ground truth; stats %s"
          % (source, len(ids), int(offsets[-1]), int(gt_off[-1]), np.round(stats, 4)))


if __name__ == "__main__":
    main()
