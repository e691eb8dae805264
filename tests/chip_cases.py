"""The case table of the chip route, shared by tests/test_chip_cpu.py (the oracle's reasons must reach every path) and
tests/test_gpu_chip.py (the device against the oracle).  The smallest shapes that reach each path: frames of 61x47, 64x64 and 130x37
(odd widths: a row end falls inside a dword) plus one 300x2 strip for the letterbox that truncates to nothing, chips of 8x8, 16x8,
12x20 and 32x32, both fits, both formats, both spaces.

A case is a dict: name, shapes [(w0, h0)], recs (one [n][6] list per frame), space, params (chip_oracle's p), num_classes, keep (list or
None), max_chips, and optionally offsets (overriding the cumulative counts), rec_capacity (default: the rows of the record buffer).
"""
import numpy as np

import chip_oracle as orc
from oracle.preprocess import letterbox_geometry

MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)
C = 20
THR = np.float32(0.3)


def params(size, fit, fmt, margin_px=0, margin_permille=0, min_side=1, min_score=THR, fill=None):
    mean32 = np.asarray(MEAN, dtype=np.float32)
    if fill is None:
        fill = mean32 * np.float32(255) if fmt == orc.F32 else (7.0, 200.0, 31.0)
    return {"cw": size[0], "ch": size[1], "fit": fit, "format": fmt, "margin_px": margin_px, "margin_permille": margin_permille,
            "min_side": min_side, "min_score": np.float32(min_score), "fill": np.asarray(fill, dtype=np.float32), "mean": mean32,
            "std": np.asarray(STD, dtype=np.float32)}


def geometry(w0, h0, side):
    rw, rh, left, top, s = letterbox_geometry(h0, w0, side)[:5]
    return (w0, h0, rw, rh, left, top, s)


def frame_pixels(seed, w0, h0):
    return np.random.RandomState(seed).randint(0, 256, size=(h0, w0, 3)).astype(np.uint8)


def box(x1, y1, x2, y2, score=0.9, cls=3):
    return [x1, y1, x2, y2, score, cls]


def random_recs(rng, n, w0, h0, lo=-8.0):
    x = np.sort(rng.uniform(lo, w0 - lo, size=(n, 2)), axis=1)
    y = np.sort(rng.uniform(lo, h0 - lo, size=(n, 2)), axis=1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1], rng.uniform(0.2, 1.0, size=n), rng.randint(0, C, size=n)], axis=1).astype(np.float32)


def _cases():
    out = []

    def add(name, shapes, recs, space, p, keep=None, max_chips=64, **kw):
        out.append(dict(name=name, shapes=shapes, recs=recs, space=space, params=p, num_classes=C, keep=keep, max_chips=max_chips, **kw))

    above = float(np.nextafter(THR, np.float32(1)))
    # resize modes into an 8x8 stretch chip, pixel space: copy (8x8), the exact 2:1 (16x16), up (5x4), down (50x40), a 1-pixel-wide source
    # (the sx >= w0 - 1 branch), a box on the frame's edge on either corner, one that leaves it, two wholly outside
    modes = [box(10, 10, 17, 17), box(10, 10, 25, 25), box(5, 5, 9, 8), box(0, 0, 49, 39), box(20, 5, 20, 30), box(0, 0, 7, 7),
             box(56, 56, 63, 63), box(-5, -5, 6, 6), box(70, 10, 90, 30), box(-30, -30, -10, -10), box(10.9, 10.2, 17.99, 17.5)]
    add("modes_u8_stretch_8x8", [(64, 64)], [modes], orc.PIXELS, params((8, 8), orc.FIT_STRETCH, orc.U8))
    add("modes_f32_stretch_8x8", [(64, 64)], [modes], orc.PIXELS, params((8, 8), orc.FIT_STRETCH, orc.F32))
    # the selection: degenerate boxes, scores, classes; class 5 is switched off
    keep = [1] * C
    keep[5] = 0
    select = [box(30, 10, 20, 20), box(10, 30, 20, 20), box(np.nan, 5, 20, 20), box(5, 5, np.inf, 20), box(5, -np.inf, 20, 20),
              box(5, 5, 20, 2.0 ** 30), box(-2.0 ** 30, 5, 20, 20), box(5, 5, 20, 20, score=float(THR)), box(5, 5, 20, 20, score=above),
              box(5, 5, 20, 20, score=np.nan), box(5, 5, 20, 20, cls=1.5), box(5, 5, 20, 20, cls=C), box(5, 5, 20, 20, cls=-1),
              box(5, 5, 20, 20, cls=np.nan), box(5, 5, 20, 20, cls=5), box(np.nan, 5, 20, 20, cls=5), box(5, 5, 20, 20, cls=C - 1),
              box(5, 5, 20, 20, cls=0), box(np.nan, 5, 20, 20, cls=C), box(5, 5, 20, 20, score=0.1, cls=77)]
    add("selection_u8_letterbox_16x8", [(61, 47)], [select], orc.PIXELS, params((16, 8), orc.FIT_LETTERBOX, orc.U8), keep=keep)
    # the margin leaves the frame on each side; margin_permille rounds: 11 * 250 -> 2.75 + 0.5 -> 3
    margins = [box(2, 20, 12, 30), box(50, 20, 58, 30), box(25, 1, 35, 9), box(25, 38, 35, 45), box(20, 15, 30, 25), box(0, 0, 60, 46)]
    add("margin_f32_letterbox_16x8", [(61, 47)], [margins], orc.PIXELS, params((16, 8), orc.FIT_LETTERBOX, orc.F32, margin_px=6, margin_permille=250))
    add("margin_u8_letterbox_12x20", [(61, 47)], [margins], orc.PIXELS, params((12, 20), orc.FIT_LETTERBOX, orc.U8, margin_px=0, margin_permille=4000))
    # min_side 5: at it, one below it on either axis, and below it only after the clip
    sides = [box(10, 10, 14, 18), box(10, 10, 13, 18), box(10, 10, 18, 13), box(-10, 5, 3, 20), box(-10, 5, 4, 20), box(10, 10, 14, 14)]
    add("min_side_u8_stretch_16x8", [(130, 37)], [sides], orc.PIXELS, params((16, 8), orc.FIT_STRETCH, orc.U8, min_side=5))
    # a 300x1 source into an 8x8 letterbox: int(r * size) == 0; its transpose on a tall frame; and one that just survives (rh == 1)
    add("fit_truncates_to_nothing", [(300, 2), (2, 300), (130, 37)], [[box(0, 0, 299, 0), box(0, 0, 299, 1)], [box(0, 0, 0, 299)], [box(0, 3, 129, 3), box(0, 3, 7, 3), box(0, 0, 129, 16)]],
        orc.PIXELS, params((8, 8), orc.FIT_LETTERBOX, orc.U8))
    # letterbox fits: tall, wide and equal aspect into a rectangular and a square chip, both formats
    aspects = [box(5, 5, 14, 34), box(5, 5, 54, 14), box(5, 5, 28, 44), box(5, 5, 16, 24), box(0, 0, 31, 31), box(3, 3, 34, 34), box(1, 1, 64, 32)]
    for size in ((12, 20), (32, 32)):
        for fmt in (orc.U8, orc.F32):
            add("aspects_%s_letterbox_%dx%d" % ("u8" if fmt == orc.U8 else "f32", size[0], size[1]), [(130, 37), (64, 64)], [aspects[:2] + aspects[6:], aspects],
                orc.PIXELS, params(size, orc.FIT_LETTERBOX, fmt))
    # letterbox space: normalised boxes of the 96-pixel square, three frames, random boxes, every chip size
    rng = np.random.RandomState(41)
    shapes = [(61, 47), (64, 64), (130, 37)]
    for k, (size, fit, fmt) in enumerate((((8, 8), orc.FIT_LETTERBOX, orc.F32), ((16, 8), orc.FIT_STRETCH, orc.F32), ((12, 20), orc.FIT_STRETCH, orc.U8), ((32, 32), orc.FIT_LETTERBOX, orc.U8))):
        recs = []
        for _ in shapes:
            n = 12
            xy = np.sort(rng.uniform(-0.1, 1.1, size=(n, 2, 2)), axis=1).reshape(n, 4)
            recs.append(np.concatenate([xy, rng.uniform(0.2, 1.0, size=(n, 1)), rng.randint(0, C, size=(n, 1))], axis=1).astype(np.float32))
        add("letterbox_space_%d" % k, shapes, recs, orc.LETTERBOX, params(size, fit, fmt, margin_px=k, margin_permille=100 * k, min_side=2), side=96)
    # frame layout: an empty frame between two full ones; 257 and 513 records in one frame (the 256-slot chunk boundary)
    rng = np.random.RandomState(42)
    add("empty_frame_between", shapes, [random_recs(rng, 9, 61, 47), np.zeros((0, 6), np.float32), random_recs(rng, 7, 130, 37)], orc.PIXELS,
        params((8, 8), orc.FIT_LETTERBOX, orc.U8, min_side=2))
    add("chunks_257_513", [(61, 47), (130, 37)], [random_recs(rng, 257, 61, 47), random_recs(rng, 513, 130, 37)], orc.PIXELS,
        params((8, 8), orc.FIT_STRETCH, orc.U8, min_side=2), max_chips=1024)
    # 70 frames: three selection launches of 32 frames' descriptors, every third frame empty, the scan over more than one wavefront's frames
    many = [shapes[i % 3] for i in range(70)]
    add("seventy_frames", many, [np.zeros((0, 6), np.float32) if i % 3 == 1 else random_recs(rng, 1 + i % 4, many[i][0], many[i][1]) for i in range(70)],
        orc.PIXELS, params((8, 8), orc.FIT_LETTERBOX, orc.F32, min_side=2), max_chips=128)
    # capacity: the cut inside a frame, and on a frame boundary; a record buffer shorter than the offsets say
    full = [[box(3 + i, 4, 20 + i, 30, cls=i) for i in range(4)], [box(5, 5 + i, 40, 30 + i, cls=i) for i in range(5)], [box(6 + 2 * i, 2, 40, 30) for i in range(3)]]
    add("overflow_inside_a_frame", shapes, full, orc.PIXELS, params((16, 8), orc.FIT_STRETCH, orc.U8), max_chips=6)
    add("overflow_on_a_frame_boundary", shapes, full, orc.PIXELS, params((16, 8), orc.FIT_STRETCH, orc.F32), max_chips=4)
    add("overflow_in_the_first_frame", shapes, full, orc.PIXELS, params((16, 8), orc.FIT_STRETCH, orc.U8), max_chips=1)
    add("short_record_buffer", shapes, full, orc.PIXELS, params((16, 8), orc.FIT_STRETCH, orc.U8), rec_capacity=6)
    add("short_record_buffer_on_a_boundary", shapes, full, orc.PIXELS, params((16, 8), orc.FIT_STRETCH, orc.U8), rec_capacity=4)
    # totals
    add("total_zero", shapes[:2], [np.zeros((0, 6), np.float32)] * 2, orc.PIXELS, params((8, 8), orc.FIT_STRETCH, orc.U8))
    add("no_frames", [], [], orc.PIXELS, params((8, 8), orc.FIT_STRETCH, orc.U8))
    add("range_mark", shapes, full, orc.PIXELS, params((16, 8), orc.FIT_STRETCH, orc.U8), offsets=[0, 4, 9, -1])
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]


def materialise(case):
    """-> (frames, geoms, rec [rows][6] float32, offsets [B+1] int32, rec_capacity).  The record buffer carries one row more than the
    offsets name (a decoy that would make a chip), unless the case cuts it short."""
    shapes = case["shapes"]
    frames = [frame_pixels(100 + i + 7 * len(shapes), w0, h0) for i, (w0, h0) in enumerate(shapes)]
    side = case.get("side")
    geoms = [geometry(w0, h0, side) if side else (w0, h0, 0, 0, 0, 0, 0) for w0, h0 in shapes]
    recs = [np.asarray(r, dtype=np.float32).reshape(-1, 6) for r in case["recs"]]
    off = np.zeros(len(shapes) + 1, dtype=np.int32)
    if recs:
        off[1:] = np.cumsum([len(r) for r in recs])
    rows = np.concatenate(recs + [np.asarray([box(1, 1, 9, 9)], dtype=np.float32)])
    if "offsets" in case:
        off = np.asarray(case["offsets"], dtype=np.int32)
    cap = case.get("rec_capacity", len(rows))
    return frames, geoms, rows, off, cap


def expected(case):
    frames, geoms, rows, off, cap = materialise(case)
    return orc.extract(frames, geoms, case["space"], rows, off, cap, case["params"], case["num_classes"], case["keep"], case["max_chips"])


# yn_chip_create's refusals: ChipExtractor's keyword arguments (out defaults to "f32" here) -> the message, in create's order of checks
REFUSALS = [
    (dict(num_classes=0), "yn_chip_create: num_classes 0 outside 1..2000"),
    (dict(num_classes=2001), "yn_chip_create: num_classes 2001 outside 1..2000"),
    (dict(max_chips=0), "yn_chip_create: max_chips 0 outside 1..65536"),
    (dict(max_chips=65537), "yn_chip_create: max_chips 65537 outside 1..65536"),
    (dict(size=(4, 8)), "yn_chip_create: cw 4 outside 8..1024"),
    (dict(size=(8, 1025)), "yn_chip_create: ch 1025 outside 8..1024"),
    (dict(margin_px=4097), "yn_chip_create: margin_px 4097 outside 0..4096"),
    (dict(margin=4.001), "yn_chip_create: margin_permille 4001 outside 0..4000"),
    (dict(margin=-0.001), "yn_chip_create: margin_permille -1 outside 0..4000"),
    (dict(min_side=0), "yn_chip_create: min_side 0 outside 1..16384"),
    (dict(size=(10, 8)), "yn_chip_create: cw 10 is no multiple of 4"),
    (dict(min_score=float("nan")), "yn_chip_create: min_score is not finite"),
    (dict(fill=(0, float("inf"), 0)), "yn_chip_create: fill[1] is not finite"),
    (dict(mean=(0.4, 0.4, float("nan"))), "yn_chip_create: fill[2] is not finite"),          # out="f32": the default fill is mean * 255
    (dict(mean=(0.4, 0.4, float("nan")), fill=(0, 0, 0)), "yn_chip_create: mean[2] is not finite"),
    (dict(std=(0.2, float("inf"), 0.2)), "yn_chip_create: std[1] is not finite"),
    (dict(std=(0.0, 0.2, 0.2)), "yn_chip_create: std[0] is not positive"),
    (dict(std=(0.2, 0.2, -1.0)), "yn_chip_create: std[2] is not positive"),
    (dict(out="u8", fill=(0, 0, 0.5)), "yn_chip_create: fill[2] is no integer in 0..255 (u8 chips)"),
    (dict(out="u8", fill=(256, 0, 0)), "yn_chip_create: fill[0] is no integer in 0..255 (u8 chips)"),
    # the order: a limit before a float, a float's finiteness before std's sign, std's sign before the u8 fill
    (dict(size=(10, 8), min_score=float("nan")), "yn_chip_create: cw 10 is no multiple of 4"),
    (dict(num_classes=0, max_chips=0), "yn_chip_create: num_classes 0 outside 1..2000"),
    (dict(std=(0.0, 0.2, float("nan"))), "yn_chip_create: std[2] is not finite"),
    (dict(out="u8", fill=(0.5, 0, 0), std=(0.0, 0.2, 0.2)), "yn_chip_create: std[0] is not positive"),
]
