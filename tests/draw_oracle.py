"""Scalar restatement of the drawing specification, one pixel at a time: the oracle of tests/test_draw_cpu.py and
tests/test_gpu_draw.py.  It shares no code with the package; it takes the same atlas, colours, labels, geometry and records.

A frame is uint8 [h0][w0][3] BGR.  Records [n][6] = x1, y1, x2, y2, score, class are taken in order, a later one painted over an
earlier one.  LETTERBOX maps a normalised box of the letterboxed square like the evaluators (`bboxes -= offset; bboxes /= scale;
bboxes *= size` on a float32 array with float64 operands); PIXELS takes the box as it is.  Every coordinate then goes through int().
"""
import math

import numpy as np

LETTERBOX, PIXELS = 0, 1


def map_box(box, geom, space):
    """box: four float32 -> four float32 in pixels of the frame.  geom = w0, h0, rw, rh, left, top, side."""
    out = []
    for c in range(4):
        v = np.float32(box[c])
        if space == LETTERBOX:
            w0, h0, rw, rh, left, top, side = (int(g) for g in geom)
            off = (left / side, top / side)[c & 1]             # Python floats are float64
            sc = (rw / side, rh / side)[c & 1]
            size = float((w0, h0)[c & 1])
            with np.errstate(all="ignore"):
                v = np.float32(np.float64(v) - off)
                v = np.float32(np.float64(v) / sc)
                v = np.float32(np.float64(v) * size)
        out.append(v)
    return out


def score_digits(score):
    """k with '%.2f' % score == '%d.%02d' % (k // 100, k % 100) for 0 <= k <= 100, else None: float32 score -> double, times 100
    (exact), rounded half to even."""
    p = float(np.float32(score)) * 100.0
    if not math.isfinite(p):
        return None
    k = round(p)                                               # Python rounds an exact half to even
    return k if 0 <= k <= 100 else None


def select(recs, geom, space, vis_thresh, num_classes):
    """-> (prims, skipped): prims = [(class, x1, y1, x2, y2, k)] of the drawn records in order."""
    prims, skipped = [], 0
    thr = np.float32(vis_thresh)
    for r in np.asarray(recs, dtype=np.float32).reshape(-1, 6):
        if not (r[4] > thr):                                   # strict; False for NaN
            continue
        m = map_box(r[:4], geom, space)
        c = float(r[5])
        ok = math.isfinite(c) and c == math.floor(c) and 0 <= c < num_classes
        ok = ok and all(math.isfinite(float(v)) and abs(float(v)) < 2.0 ** 30 for v in m)
        k = score_digits(r[4])
        if not ok or k is None:
            skipped += 1
            continue
        prims.append((int(c),) + tuple(int(v) for v in m) + (k,))
    return prims, skipped


def label_text(name, k):
    return "%s: %d.%02d" % (name, k // 100, k % 100)


def paint(frame, prims, colors, labels, atlas, thickness):
    """Paints prims (select()'s) onto frame in place.  colors [C][3] BGR; labels: C strings or None; atlas uint8 [95][gh][gw]."""
    h0, w0 = frame.shape[:2]
    t = int(thickness)
    a, c = t // 2, (t - 1) // 2
    for cls, x1, y1, x2, y2, k in prims:
        color = [int(v) for v in colors[cls]]
        for y in range(max(y1 - a, 0), min(y2 + a, h0 - 1) + 1):
            for x in range(max(x1 - a, 0), min(x2 + a, w0 - 1) + 1):
                if x1 + c + 1 <= x <= x2 - c - 1 and y1 + c + 1 <= y <= y2 - c - 1:
                    continue                                   # the hole
                frame[y, x] = color
        if labels is None:
            continue
        gh, gw = int(atlas.shape[1]), int(atlas.shape[2])
        text = label_text(labels[cls], k)
        L = len(text)
        assert L == len(labels[cls]) + 6
        for y in range(max(y1 - gh - 1, 0), min(y1, h0 - 1) + 1):
            for x in range(max(x1, 0), min(x1 + L * gw + 1, w0 - 1) + 1):
                frame[y, x] = color
        for j, ch in enumerate(text):
            for r in range(gh):
                for col in range(gw):
                    x, y = x1 + 1 + j * gw + col, y1 - gh + r
                    if not (0 <= x < w0 and 0 <= y < h0):
                        continue
                    a8 = int(atlas[ord(ch) - 32, r, col])
                    if a8 == 0:
                        continue                               # (dst * 255 + 127) // 255 == dst
                    for ch3 in range(3):
                        frame[y, x, ch3] = (int(frame[y, x, ch3]) * (255 - a8) + 0 * a8 + 127) // 255
    return frame


def draw(frame, recs, geom, space, vis_thresh, colors, labels, atlas, thickness):
    """One frame: -> (painted copy, prims, skipped)."""
    prims, skipped = select(recs, geom, space, vis_thresh, len(colors))
    out = paint(np.array(frame, dtype=np.uint8, copy=True), prims, colors, labels, atlas, thickness)
    return out, prims, skipped
