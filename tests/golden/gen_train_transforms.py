"""Generate tests/golden/train_transforms.npz: the reference's own augmentation classes (data/transforms.py, imported unmodified),
for tests/test_train_aug_cpu.py.

    python tests/golden/gen_train_transforms.py [path/to/reference]     (default: $YN_REFERENCE, else ../reference beside the repository)

cv2 is not needed: the cv2 module is an empty placeholder, PhotometricDistort's two ConvertColor entries are replaced by
pass-throughs (they draw nothing), and Resize is not run (its geometry is checked through oracle/preprocess.py's restatement).

Sampler cases: TrainTransforms' and ColorTransforms' sequence up to ToPercentCoords (ConvertFromInts, ToAbsoluteCoords,
PhotometricDistort, [RandomSampleCrop,] RandomMirror, ToPercentCoords) on tall, wide, square and thin frames down to 4 px, with
random box sets, the empty-image target zeros([1, 5]) and a tiny corner box most crops miss.  Each case records every np.random
draw (function, arguments, value; numpy.random.randint / uniform are wrapped during the run), the boxes and labels after
ToPercentCoords and the cropped image's shape.

Pointwise cases: RandomBrightness, RandomContrast, RandomSaturation and RandomHue on small float32 images whose values include
negatives, values above 255, and hues next to 0 and 360: input, output and the draws.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("YN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))      # data/transforms.py imports cv2; never called here
sys.path.insert(0, REF)

from data import transforms as T                            # noqa: E402

SHAPES = [(375, 500), (500, 375), (400, 400), (4, 4), (4, 9), (9, 4), (37, 53), (53, 37), (640, 427), (7, 300), (300, 7), (64, 64)]
FN = {"randint": 0, "uniform": 1}


class DrawLog(object):
    """Wraps numpy.random.randint / uniform (the reference's `random.` and `np.random.` both resolve through the module)."""

    def __init__(self):
        self.rows = []

    def __enter__(self):
        self._orig = {k: getattr(np.random, k) for k in FN}
        for k in FN:
            setattr(np.random, k, self._wrap(k, self._orig[k]))
        return self

    def __exit__(self, *exc):
        for k, f in self._orig.items():
            setattr(np.random, k, f)

    def _wrap(self, name, f):
        def g(*args):
            v = f(*args)
            a = list(args) + [np.nan] * (2 - len(args))
            self.rows.append((FN[name], float(a[0]), float(a[1]), float(v)))
            return v
        return g


def passthrough(image, boxes=None, labels=None, scale=None, offset=None):
    return image, boxes, labels, scale, offset


def pipeline(crop):
    pd = T.PhotometricDistort()
    pd.pd[1] = passthrough                                  # ConvertColor(BGR -> HSV): cv2, no draws
    pd.pd[4] = passthrough                                  # ConvertColor(HSV -> BGR)
    steps = [T.ConvertFromInts(), T.ToAbsoluteCoords(), pd] + ([T.RandomSampleCrop()] if crop else []) + [T.RandomMirror(), T.ToPercentCoords()]
    return T.Compose(steps)


def boxes_for(rs, kind, n):
    if kind == "empty":
        t = np.zeros([1, 5])                                # data/voc.py:227 for an image without objects
        return t
    if kind == "corner":                                    # one tiny box in the top-left corner: most crops miss its centre
        return np.array([[0.0, 0.0, 0.02, 0.03, 7.0]])
    xy = rs.rand(n, 2) * 0.7
    wh = 0.05 + rs.rand(n, 2) * 0.3
    return np.hstack([xy, np.minimum(xy + wh, 1.0), rs.randint(0, 20, (n, 1)).astype(np.float64)])


def make_sampler_cases():
    cases = {k: [] for k in ("crop", "seed", "shape", "target", "target_off", "draws", "draws_off", "boxes", "labels", "out_off", "crop_shape")}
    for k in ("target_off", "draws_off", "out_off"):
        cases[k].append(0)
    tgt, drw, bxs, lbs = [], [], [], []
    rs = np.random.RandomState(20261016)
    i = 0
    for crop in (1, 0):
        n_cases = 288 if crop else 72
        for c in range(n_cases):
            h0, w0 = SHAPES[c % len(SHAPES)]
            kind = "empty" if c % 24 == 4 else ("corner" if c % 24 == 13 else "boxes")
            target = boxes_for(rs, kind, int(rs.randint(1, 5)))
            seed = 1000 + i
            i += 1
            image = np.zeros((h0, w0, 3), np.uint8)
            np.random.seed(seed)
            with DrawLog() as log:
                t = target.copy()
                img, boxes, labels, _, _ = pipeline(crop)(image, t[:, :4], t[:, 4])
            cases["crop"].append(crop)
            cases["seed"].append(seed)
            cases["shape"].append((h0, w0))
            tgt.append(target)
            cases["target_off"].append(cases["target_off"][-1] + len(target))
            drw.extend(log.rows)
            cases["draws_off"].append(len(drw))
            bxs.append(np.asarray(boxes, np.float64))
            lbs.append(np.asarray(labels, np.float64))
            cases["out_off"].append(cases["out_off"][-1] + len(boxes))
            cases["crop_shape"].append(img.shape[:2])
    out = {"s_" + k: np.array(v) for k, v in cases.items()}
    out["s_crop"] = out["s_crop"].astype(np.int8)
    out["s_target"] = np.concatenate(tgt)
    out["s_draws"] = np.array(drw, np.float64)
    out["s_boxes"] = np.concatenate(bxs)
    out["s_labels"] = np.concatenate(lbs)
    return out


def pointwise_image(rs):
    img = rs.uniform(-60.0, 320.0, (6, 8, 3)).astype(np.float32)
    img[0, :, 0] = np.array([0.0, 1e-3, 0.5, 17.9, 359.5, 359.999, 360.0, 342.0], np.float32)     # hues next to the wraps
    img[1, :, :] = np.float32(255.0)
    return img


def make_pointwise_cases():
    classes = [("brightness", T.RandomBrightness()), ("contrast", T.RandomContrast()), ("saturation", T.RandomSaturation()),
               ("hue", T.RandomHue())]
    rs = np.random.RandomState(7)
    out = {}
    for name, op in classes:
        ins, outs, draws = [], [], []
        for k in range(24):
            img = pointwise_image(rs)
            np.random.seed(500 + k)
            with DrawLog() as log:
                res = op(img.copy())[0]
            ins.append(img)
            outs.append(res)
            rows = log.rows + [(-1, np.nan, np.nan, np.nan)] * (2 - len(log.rows))
            draws.append(rows)
        out["p_%s_in" % name] = np.stack(ins)
        out["p_%s_out" % name] = np.stack(outs)
        out["p_%s_draws" % name] = np.array(draws, np.float64)
    return out


def main():
    data = make_sampler_cases()
    data.update(make_pointwise_cases())
    path = os.path.join(HERE, "train_transforms.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes): %d sampler cases, %d draws" % (path, os.path.getsize(path), len(data["s_seed"]), len(data["s_draws"])))


if __name__ == "__main__":
    main()
