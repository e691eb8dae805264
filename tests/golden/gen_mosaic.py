"""Generate tests/golden/mosaic.npz: the reference's own VOCDetection.load_mosaic (data/voc.py, imported unmodified) called on a stub
dataset, then its ColorTransforms sequence up to ToPercentCoords, for tests/test_mosaic_cpu.py.

    python tests/golden/gen_mosaic.py [path/to/reference]     (default: $YN_REFERENCE, else ../reference beside the repository)

cv2 is not installed where this runs, so the cv2 module is a placeholder whose `resize` is oracle/preprocess.py's restatement of the
8-bit INTER_LINEAR path (the same function the pixel oracle tests/mosaic_oracle.py uses), and PhotometricDistort's two ConvertColor
entries are pass-throughs (they draw nothing), as in gen_train_transforms.py.

The stub serves seeded synthetic frames and targets through `load_img_targets`.  Every case runs with TAG frames (frame k of the
mosaic filled with k + 1), so that the canvas rectangle of each frame can be read off the returned canvas; the frames are an ndarray
subclass that logs the slices load_mosaic takes from them (the source rectangles), and the placeholder resize logs its dsize.  Cases
of the small sizes run a second time from the same seeds with noise frames (tests/mosaic_oracle.py: frame) and store that canvas.

Per case: both seeds, index, the picked ids, shapes, targets, the two `random.uniform` draws (arguments and value), every np.random
draw of the colour pass, resized extents, both rectangles per frame, the mosaic targets, the boxes and labels after ToPercentCoords,
and the next value of each generator after the call (so a test can tell that the same number of draws was consumed).
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("YN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))

sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle.preprocess import cv2_resize_linear_u8          # noqa: E402
import mosaic_oracle as mo                                  # noqa: E402

RESIZES = []


class Frame(np.ndarray):
    """uint8 frame that logs `img_i[y1b:y2b, x1b:x2b]`."""
    log = []

    def __getitem__(self, key):
        if isinstance(key, tuple) and len(key) == 2 and all(isinstance(k, slice) for k in key):
            Frame.log.append((key[1].start, key[0].start, key[1].stop, key[0].stop))
        return np.asarray(self).__getitem__(key)


def _resize(img, dsize):
    RESIZES.append((int(dsize[0]), int(dsize[1])))
    return cv2_resize_linear_u8(np.asarray(img), dsize).view(Frame)


cv2 = types.ModuleType("cv2")
cv2.resize = _resize
sys.modules.setdefault("cv2", cv2)
sys.path.insert(0, REF)

from data import transforms as T                            # noqa: E402
from data.voc import VOCDetection                           # noqa: E402

MEAN = (0.406, 0.456, 0.485)
N_IDS = 23
# frame shapes (h0, w0): VOC-like, square, odd, thin; per size S also S x S-ish (r == 1) and 2S-long even frames (exact 2:1)
BASE = [(375, 500), (500, 375), (333, 500), (480, 640), (400, 400), (37, 53), (53, 37), (129, 95), (61, 200), (300, 7), (7, 300), (9, 4)]


def shapes_for(s):
    """The shape list of size s: BASE plus the frames that hit the r == 1 and exact 2:1 branches, without any shape whose resized
    extent `int(min * (s / max))` would be 0 (load_mosaic dies in cv2.resize there; the sampler refuses them by design)."""
    extra = [(s, s), (s, s - s // 4), (s - s // 3, s), (2 * s, 2 * s), (2 * s, 2 * s - 2 * (s // 8)), (s + 1, 2 * s)]
    return [(h, w) for h, w in BASE + extra if int(min(h, w) * (s / max(h, w))) >= 1]


class DrawLog(object):
    """Wraps numpy.random.randint / uniform (as gen_train_transforms.py) and Python's random.uniform / random.sample."""
    FN = {"randint": 0, "uniform": 1}

    def __init__(self):
        self.rows, self.py_uniform, self.py_sample = [], [], []

    def __enter__(self):
        self._np = {k: getattr(np.random, k) for k in self.FN}
        self._py = {k: getattr(random, k) for k in ("uniform", "sample")}
        for k in self.FN:
            setattr(np.random, k, self._wrap(k, self._np[k]))
        random.uniform = self._uniform
        random.sample = self._sample
        return self

    def __exit__(self, *exc):
        for k, f in self._np.items():
            setattr(np.random, k, f)
        for k, f in self._py.items():
            setattr(random, k, f)

    def _wrap(self, name, f):
        def g(*args):
            v = f(*args)
            a = list(args) + [np.nan] * (2 - len(args))
            self.rows.append((self.FN[name], float(a[0]), float(a[1]), float(v)))
            return v
        return g

    def _uniform(self, a, b):
        v = self._py["uniform"](a, b)
        self.py_uniform.append((float(a), float(b), float(v)))
        return v

    def _sample(self, population, k):
        v = self._py["sample"](population, k)
        self.py_sample.append((len(population), k, list(v)))
        return v


def passthrough(image, boxes=None, labels=None, scale=None, offset=None):
    return image, boxes, labels, scale, offset


def color_pipeline():
    pd = T.PhotometricDistort()
    pd.pd[1] = passthrough                                  # ConvertColor(BGR -> HSV): cv2, no draws
    pd.pd[4] = passthrough                                  # ConvertColor(HSV -> BGR)
    return T.Compose([T.ConvertFromInts(), T.ToAbsoluteCoords(), pd, T.RandomMirror(), T.ToPercentCoords()])


class Stub(object):
    """What load_mosaic reads of a VOCDetection: ids, img_size, transform.mean, load_img_targets."""

    def __init__(self, s, shapes, targets, noise_seed=None):
        self.ids = list(range(N_IDS))
        self.img_size = s
        self.transform = types.SimpleNamespace(mean=MEAN)
        self._shapes, self._targets, self._noise, self._served = shapes, targets, noise_seed, 0

    def load_img_targets(self, img_id):
        h0, w0 = self._shapes[img_id]
        if self._noise is None:
            img = np.full((h0, w0, 3), self._served + 1, np.uint8)
        else:
            img = mo.frame(self._noise + img_id, h0, w0)
        self._served += 1
        return img.view(Frame), [list(r) for r in self._targets[img_id]], h0, w0


def targets_for(rs, empty):
    n = 0 if empty else int(rs.randint(0, 4))
    xy = rs.rand(n, 2) * 0.7
    return np.hstack([xy, np.minimum(xy + 0.05 + rs.rand(n, 2) * 0.3, 1.0), rs.randint(0, 20, (n, 1)).astype(np.float64)])


def run_case(s, shapes, targets, index, py_seed, np_seed, noise_seed):
    stub = Stub(s, shapes, targets, noise_seed)
    del RESIZES[:]
    del Frame.log[:]
    random.seed(py_seed)
    np.random.seed(np_seed)
    with DrawLog() as log:
        img, tg, _, _ = VOCDetection.load_mosaic(stub, index)
        py_probe = log._py["uniform"](0.0, 1.0)
        assert img.dtype == np.float64 and img.shape == (2 * s, 2 * s, 3)
        mosaic_tg = tg.copy()
        _, boxes, labels, _, _ = color_pipeline()(img.copy(), tg[:, :4], tg[:, 4])
        np_probe = log._np["uniform"](0.0, 1.0)
    return img, mosaic_tg, np.asarray(boxes, np.float64), np.asarray(labels, np.float64), log, py_probe, np_probe, list(RESIZES), list(Frame.log)


def main():
    plan = [(16, 10, 10), (32, 6, 6), (64, 40, 3), (416, 24, 0), (500, 12, 0), (608, 24, 0)]     # (S, cases, canvases kept)
    rs = np.random.RandomState(20261016)
    keys = ("size", "index", "py_seed", "np_seed", "ids", "shapes", "uniform", "ext", "rect_a", "rect_b", "py_probe", "np_probe", "canvas_id")
    c = {k: [] for k in keys}
    tgt, tgt_off, mtg, mtg_off, drw, drw_off, bxs, lbs, out_off = [], [0], [], [0], [], [0], [], [], [0]
    canvases = {}
    case = 0
    for s, n_cases, n_canvas in plan:
        sl = shapes_for(s)
        for k in range(n_cases):
            shapes = [sl[int(v)] for v in rs.randint(0, len(sl), N_IDS)]
            all_empty = k % 8 == 5
            targets = [targets_for(rs, all_empty or i % 5 == 3) for i in range(N_IDS)]
            index = [0, N_IDS - 1, int(rs.randint(1, N_IDS - 1))][k % 3]
            py_seed, np_seed = 5000 + case, 9000 + case
            img, mosaic_tg, boxes, labels, log, py_probe, np_probe, resizes, slices = run_case(s, shapes, targets, index, py_seed, np_seed, None)
            (pop, kk, picks), = log.py_sample
            assert pop == N_IDS - 1 and kk == 3 and len(log.py_uniform) == 2 and len(slices) == 4
            ids = [index] + picks
            ext, rect_a, it = [], [], iter(resizes)
            for i, j in enumerate(ids):
                h0, w0 = shapes[j]
                ext.append(next(it) if s / max(h0, w0) != 1 else (w0, h0))
                ys, xs = np.nonzero(img[:, :, 0] == i + 1)                     # the tag of frame i on the canvas
                rect_a.append((xs.min(), ys.min(), xs.max() + 1, ys.max() + 1))
                assert len(xs) == (rect_a[-1][2] - rect_a[-1][0]) * (rect_a[-1][3] - rect_a[-1][1])
            assert next(it, None) is None
            canvas_id = -1
            if k < n_canvas:                                                # the same draws with noise frames: the canvas itself
                noise = 700000 + 100 * case
                img2, mtg2, b2, l2, _, p2, q2, r2, s2 = run_case(s, shapes, targets, index, py_seed, np_seed, noise)
                assert np.array_equal(mtg2, mosaic_tg) and np.array_equal(b2, boxes) and (p2, q2, r2, s2) == (py_probe, np_probe, resizes, slices)
                canvas_id = noise
                canvases["canvas_%d" % case] = img2.astype(np.float32)
            for key, v in zip(keys, (s, index, py_seed, np_seed, ids, [shapes[j] for j in ids], log.py_uniform, ext, rect_a, slices,
                                     py_probe, np_probe, canvas_id)):
                c[key].append(v)
            for j in ids:
                tgt.append(targets[j])
                tgt_off.append(tgt_off[-1] + len(targets[j]))
            mtg.append(mosaic_tg)
            mtg_off.append(mtg_off[-1] + len(mosaic_tg))
            drw.extend(log.rows)
            drw_off.append(len(drw))
            bxs.append(boxes)
            lbs.append(labels)
            out_off.append(out_off[-1] + len(boxes))
            case += 1
    data = {"m_" + k: np.array(v) for k, v in c.items()}
    data.update(m_n_ids=np.array(N_IDS), m_mean=np.array(MEAN), m_target=np.concatenate(tgt), m_target_off=np.array(tgt_off),
                m_mosaic_tg=np.concatenate(mtg), m_mosaic_tg_off=np.array(mtg_off), m_draws=np.array(drw, np.float64),
                m_draws_off=np.array(drw_off), m_boxes=np.concatenate(bxs), m_labels=np.concatenate(lbs), m_out_off=np.array(out_off))
    data.update(canvases)
    path = os.path.join(HERE, "mosaic.npz")
    np.savez_compressed(path, **data)
    print("wrote %s (%d bytes): %d cases, %d canvases" % (path, os.path.getsize(path), case, len(canvases)))


if __name__ == "__main__":
    main()
