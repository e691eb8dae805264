"""Restatement of the chip specification, one record at a time, in float32 / int64 numpy and Python integers: the oracle
of tests/test_chip_cpu.py and tests/test_gpu_chip.py.  It shares no code with the package.  The resize is
oracle.preprocess.cv2_resize_linear_u8 (not re-derived here); everything else is restated.

A frame is uint8 [h0][w0][3] BGR.  Records [n][6] = x1, y1, x2, y2, score, class are taken frame by frame in list order.  Every record
gets a reason: one of NOT_SELECTED (score, class_keep), the SKIP_* causes (counted as skipped), OVERFLOW, or CHIP.
"""
import math

import numpy as np

from oracle.preprocess import cv2_resize_linear_u8

LETTERBOX, PIXELS = 0, 1                                       # space
FIT_LETTERBOX, FIT_STRETCH = 0, 1
U8, F32 = 0, 1

CHIP = "chip"
LOW_SCORE, CLASS_OFF = "not selected: score", "not selected: class_keep"
SKIP_CLASS, SKIP_COORD, SKIP_INVERTED = "skipped: class", "skipped: coordinate", "skipped: inverted"
SKIP_EMPTY, SKIP_MIN_SIDE, SKIP_FIT = "skipped: outside the frame", "skipped: min_side", "skipped: fit"
OVERFLOW = "overflow"
UNREAD = "not read: past rec_capacity"
SKIPS = (SKIP_CLASS, SKIP_COORD, SKIP_INVERTED, SKIP_EMPTY, SKIP_MIN_SIDE, SKIP_FIT)
MODES = ("copy", "box", "linear")


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


def fit(sw, sh, cw, ch, mode):
    """-> (rw, rh, left, top) of the source rectangle sw x sh inside the cw x ch chip; rw or rh may be 0."""
    if mode == FIT_STRETCH:
        return cw, ch, 0, 0
    p, q = sh * cw, sw * ch                                    # Python integers
    if p > q:
        rw = int(float(sw) / float(sh) * float(ch))
        return rw, ch, (cw - rw) // 2, 0
    if p < q:
        rh = int(float(sh) / float(sw) * float(cw))
        return cw, rh, 0, (ch - rh) // 2
    return cw, ch, 0, 0


def resize_mode(sh, sw, rw, rh):
    return 0 if (rw == sw and rh == sh) else (1 if (sw == 2 * rw and sh == 2 * rh) else 2)


def examine(r, geom, space, p, num_classes, keep):
    """One record -> (reason, rect or None); rect = x, y, sw, sh, rw, rh, left, top.  p: cw, ch, fit, margin_px, margin_permille,
    min_side, min_score."""
    r = np.asarray(r, dtype=np.float32)
    if not (r[4] > np.float32(p["min_score"])):                # strict; False for NaN
        return LOW_SCORE, None
    c = float(r[5])
    if not (math.isfinite(c) and c == math.floor(c) and 0 <= c < num_classes):
        return SKIP_CLASS, None
    if keep is not None and not keep[int(c)]:
        return CLASS_OFF, None
    w0, h0 = int(geom[0]), int(geom[1])
    m = map_box(r[:4], geom, space)
    if not all(math.isfinite(float(v)) and abs(float(v)) < 2.0 ** 30 for v in m):
        return SKIP_COORD, None
    X1, Y1, X2, Y2 = (int(v) for v in m)                       # toward zero
    if X2 < X1 or Y2 < Y1:
        return SKIP_INVERTED, None
    mx = p["margin_px"] + ((X2 - X1 + 1) * p["margin_permille"] + 500) // 1000
    my = p["margin_px"] + ((Y2 - Y1 + 1) * p["margin_permille"] + 500) // 1000
    xa, xb = max(X1 - mx, 0), min(X2 + mx, w0 - 1)
    ya, yb = max(Y1 - my, 0), min(Y2 + my, h0 - 1)
    sw, sh = xb - xa + 1, yb - ya + 1
    if sw < 1 or sh < 1:
        return SKIP_EMPTY, None
    if sw < p["min_side"] or sh < p["min_side"]:
        return SKIP_MIN_SIDE, None
    rw, rh, left, top = fit(sw, sh, p["cw"], p["ch"], p["fit"])
    if rw == 0 or rh == 0:
        return SKIP_FIT, None
    return CHIP, (xa, ya, sw, sh, rw, rh, left, top)


def render(frame, rect, p):
    """The chip of one rectangle: uint8 [ch][cw][3] BGR, or float32 [3][ch][cw] RGB normalised."""
    x, y, sw, sh, rw, rh, left, top = rect
    crop = np.ascontiguousarray(frame[y:y + sh, x:x + sw])
    res = cv2_resize_linear_u8(crop, (rw, rh))
    fill = np.asarray(p["fill"], dtype=np.float32)
    if p["format"] == U8:
        chip = np.empty((p["ch"], p["cw"], 3), dtype=np.uint8)
        chip[:] = fill.astype(np.uint8)
        chip[top:top + rh, left:left + rw] = res
        return chip
    img = np.empty((p["ch"], p["cw"], 3), dtype=np.float32)
    img[:] = fill
    img[top:top + rh, left:left + rw] = res.astype(np.float32)
    img /= np.float32(255.0)                                   # Normalize, each step rounded to float32
    img -= np.asarray(p["mean"], dtype=np.float32)
    img /= np.asarray(p["std"], dtype=np.float32)
    return np.ascontiguousarray(np.transpose(img[..., (2, 1, 0)], (2, 0, 1)))


def extract(frames, geoms, space, rec, offsets, rec_capacity, p, num_classes, keep, max_chips):
    """The whole call -> dict(chips [n] arrays, index [n], rects [n][8], offsets [B+1], counters (chips, skipped, overflow, range_mark),
    reasons: one (frame, record index, reason, resize mode or None) per record the offsets name, modes)."""
    B = len(frames)
    offsets = [int(v) for v in offsets]
    if B == 0:
        return {"chips": [], "index": [], "rects": [], "offsets": [0], "counters": (0, 0, 0, 0), "reasons": []}
    if offsets[B] < 0:
        return {"chips": [], "index": [], "rects": [], "offsets": [0] * B + [-1], "counters": (0, 0, 0, 1), "reasons": []}
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, 6)
    chips, index, rects, reasons, out_off = [], [], [], [], [0]
    usable = skipped = 0
    for b in range(B):
        lo = min(max(offsets[b], 0), rec_capacity)
        hi = min(max(offsets[b + 1], lo), rec_capacity)
        for i in range(offsets[b], offsets[b + 1]):
            if not lo <= i < hi:
                reasons.append((b, i, UNREAD, None))
        for i in range(lo, hi):
            why, rect = examine(rec[i], geoms[b], space, p, num_classes, keep)
            mode = None
            if why in SKIPS:
                skipped += 1
            if why == CHIP:
                usable += 1
                mode = MODES[resize_mode(rect[3], rect[2], rect[4], rect[5])]
                if usable > max_chips:
                    why = OVERFLOW
                else:
                    chips.append(render(frames[b], rect, p))
                    index.append(i)
                    rects.append(list(rect))
            reasons.append((b, i, why, mode))
        out_off.append(min(usable, max_chips))
    n = min(usable, max_chips)
    return {"chips": chips, "index": index, "rects": rects, "offsets": out_off, "counters": (n, skipped, usable - n, 0), "reasons": reasons}
