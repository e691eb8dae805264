"""Generate tests/golden/voc_eval.npz: the reference's own voc_eval (evaluator/vocapi_evaluator.py, imported unmodified) on a
synthetic VOC tree, for tests/test_eval_cpu.py and tests/test_gpu_eval.py.

    python tests/golden/gen_voc_eval.py [path/to/reference]     (default: $YN_REFERENCE, else ../reference beside the repository)

48 images (tall, wide, square), 20 classes, detections jittered around the ground truth with distinct 3-decimal scores inside each
class (so the reference's unstable argsort has no ties to order); class 18 has no detections (AP -1), class 19 only difficult ground
truth (npos = 0), some images have no ground truth.  The per-class result files are written here in the reference's format
(:154): its own writer tests `dets == []`, which raises under numpy >= 2.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("YN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))      # data/voc.py imports cv2; never called
np.bool = bool                                              # voc_eval's np.bool (restored alias under numpy 2 anyway)
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from evaluator.vocapi_evaluator import VOCAPIEvaluator      # noqa: E402
from data.voc import VOC_CLASSES                            # noqa: E402
import voc_oracle                                            # noqa: E402

SIDE = 416
C = 20
N_IMG = 48


def make():
    rng = np.random.default_rng(20261016)
    shapes = [(375, 500), (500, 375), (400, 400), (333, 500), (500, 281), (288, 288)]
    geoms, gts, boxes, scores, classes, offsets = [], [], [], [], [], [0]
    used = [set() for _ in range(C)]

    def score_for(c):
        while True:
            k = int(rng.integers(1, 1000))
            if k not in used[c]:
                used[c].add(k)
                return np.float32((k + rng.uniform(-0.3, 0.3)) / 1000.0)

    for i in range(N_IMG):
        h0, w0 = shapes[i % len(shapes)]
        geom = voc_oracle_geometry(h0, w0)
        geoms.append(geom)
        scale, offset, size = voc_oracle.geometry_arrays(geom)
        g = []
        if i % 7 != 3:                                       # every 7th image from the 4th on: no ground truth
            for _ in range(int(rng.integers(1, 6))):
                c = int(rng.integers(0, 18))
                x1, y1 = int(rng.integers(1, w0 - 40)), int(rng.integers(1, h0 - 40))
                x2, y2 = int(rng.integers(x1 + 10, min(w0, x1 + 200))), int(rng.integers(y1 + 10, min(h0, y1 + 200)))
                g.append([x1, y1, x2, y2, c, int(rng.random() < 0.15)])
            if i % 5 == 0:
                x1, y1 = int(rng.integers(1, w0 // 2)), int(rng.integers(1, h0 // 2))
                g.append([x1, y1, x1 + 30, y1 + 30, 19, 1])         # class 19: difficult only
        g = np.array(g, dtype=np.int32).reshape(-1, 6)
        gts.append(g)
        det = []
        for row in g:
            for _ in range(int(rng.integers(0, 4))):
                if row[4] == 18:
                    continue
                jit = rng.normal(0, 0.12, 4) * np.array([row[2] - row[0], row[3] - row[1]] * 2)
                det.append((row[:4] - 1 + jit, int(row[4]) if rng.random() < 0.85 else int(rng.integers(0, 18))))
        for _ in range(int(rng.integers(0, 4))):             # false positives anywhere
            x1, y1 = rng.uniform(-10, w0 - 20), rng.uniform(-10, h0 - 20)
            det.append((np.array([x1, y1, x1 + rng.uniform(5, 150), y1 + rng.uniform(5, 150)]), int(rng.integers(0, 18))))
        for pix, c in det:
            if c == 18:
                continue
            norm = (np.asarray(pix, dtype=np.float64) / size.reshape(-1)) * np.asarray(scale).reshape(-1)[:4] + offset.reshape(-1)
            boxes.append(norm.astype(np.float32))
            scores.append(score_for(c))
            classes.append(c)
        offsets.append(len(scores))
    return (np.array(geoms, dtype=np.int32), gts, np.array(boxes, dtype=np.float32).reshape(-1, 4),
            np.array(scores, dtype=np.float32), np.array(classes, dtype=np.int32), np.array(offsets, dtype=np.int32))


def voc_oracle_geometry(h0, w0):
    """Resize's integer geometry (data/transforms.py:79-116, ValTransforms.geometry) for the SIDE square"""
    if h0 > w0:
        rw, rh = int(w0 / h0 * SIDE), SIDE
        return (w0, h0, rw, rh, (rh - rw) // 2, 0, SIDE)
    if h0 < w0:
        rw, rh = SIDE, int(h0 / w0 * SIDE)
        return (w0, h0, rw, rh, 0, (rw - rh) // 2, SIDE)
    return (w0, h0, SIDE, SIDE, 0, 0, SIDE)


def run_reference(geoms, gts, boxes, scores, classes, offsets):
    names = ["%06d" % i for i in range(len(geoms))]
    with tempfile.TemporaryDirectory() as tmp:
        voc = os.path.join(tmp, "VOC2007")
        for d in ("Annotations", "ImageSets/Main", "results"):
            os.makedirs(os.path.join(voc, d))
        with open(os.path.join(voc, "ImageSets", "Main", "test.txt"), "w") as f:
            f.write("".join(n + "\n" for n in names))
        for n, g in zip(names, gts):
            objs = "".join("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
                           "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
                           % (VOC_CLASSES[r[4]], r[5], r[0], r[1], r[2], r[3]) for r in g)
            with open(os.path.join(voc, "Annotations", n + ".xml"), "w") as f:
                f.write("<annotation><filename>%s.jpg</filename>%s</annotation>" % (n, objs))
        # results files in the reference's format (:147-159), the evaluator's own rescale (:72-74)
        lines = [[] for _ in range(C)]
        for i, n in enumerate(names):
            s, e = offsets[i], offsets[i + 1]
            scale, offset, size = voc_oracle.geometry_arrays(geoms[i])
            b = boxes[s:e].copy()
            b -= offset
            b /= scale
            b *= size
            for c in range(C):
                inds = np.where(classes[s:e] == c)[0]
                dets = np.hstack((b[inds], scores[s:e][inds][:, None])).astype(np.float32, copy=False)
                for k in range(dets.shape[0]):
                    lines[c].append('{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}\n'.format(
                        n, dets[k, -1], dets[k, 0] + 1, dets[k, 1] + 1, dets[k, 2] + 1, dets[k, 3] + 1))
        ev = object.__new__(VOCAPIEvaluator)
        ev.imgsetpath = os.path.join(voc, "ImageSets", "Main", "test.txt")
        ev.annopath = os.path.join(voc, "Annotations", "%s.xml")
        ev.display = False
        out = {}
        for use07 in (True, False):
            cache = os.path.join(tmp, "cache07" if use07 else "cache")
            aps, recs, precs, offs = [], [], [], [0]
            for c, cls in enumerate(VOC_CLASSES[:C]):
                path = os.path.join(voc, "results", "det_test_%s.txt" % cls)
                with open(path, "wt") as f:
                    f.write("".join(lines[c]))
                rec, prec, ap = ev.voc_eval(detpath=path, classname=cls, cachedir=cache, ovthresh=0.5, use_07_metric=use07)
                aps.append(ap)
                if np.ndim(rec):
                    recs.append(rec); precs.append(prec)
                offs.append(offs[-1] + (len(rec) if np.ndim(rec) else 0))
            tag = "07" if use07 else "area"
            out["ap_" + tag] = np.array(aps, dtype=np.float64)
            out["map_" + tag] = np.float64(np.mean(aps))
            out["rec_" + tag] = np.concatenate(recs)
            out["prec_" + tag] = np.concatenate(precs)
            out["curve_off"] = np.array(offs, dtype=np.int64)
    return out


def main():
    geoms, gts, boxes, scores, classes, offsets = make()
    gt_off = np.zeros(len(gts) + 1, dtype=np.int32)
    gt_off[1:] = np.cumsum([len(g) for g in gts])
    out = run_reference(geoms, gts, boxes, scores, classes, offsets)
    np.savez_compressed(os.path.join(HERE, "voc_eval.npz"), geoms=geoms, gt=np.concatenate(gts).astype(np.int32), gt_off=gt_off,
                        boxes=boxes, scores=scores, classes=classes, offsets=offsets, **out)
    print("voc_eval.npz: %d images, %d detections, %d ground truth; AP07 %s; mAP07 %.6f, mAP area %.6f"
          % (len(geoms), len(scores), int(gt_off[-1]), np.round(out["ap_07"], 3), out["map_07"], out["map_area"]))


if __name__ == "__main__":
    main()
