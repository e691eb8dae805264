"""CPU checks of the drawing route (yolo_nano_amd.draw): the class colours, the built-in font against its requirements, and
the two pieces of the oracle (tests/draw_oracle.py) that are pinned to the reference - the score digits ('%.2f') and the mapping of a
box to integer pixels (rescale_boxes on a float32 array, then int())."""
import json
import os

import numpy as np

import draw_oracle as orc
from yolo_nano_amd import draw

HERE = os.path.dirname(os.path.abspath(__file__))
OWN = "abcdefghijklmnopqrstuvwxyz0123456789:.-"


def test_class_colors_are_the_reference_sequence():
    state = np.random.get_state()
    np.random.seed(0)
    ref = [(np.random.randint(255), np.random.randint(255), np.random.randint(255)) for _ in range(80)]     # test.py:192-195
    np.random.set_state(state)
    mark = np.random.get_state()[1].copy()
    assert draw.class_colors(80) == ref
    assert np.array_equal(np.random.get_state()[1], mark), "class_colors moved numpy's global generator"
    assert draw.class_colors(20) == ref[:20]
    assert draw.class_colors(5, seed=3) != ref[:5]


def test_default_font_meets_its_requirements():
    font = draw.default_font()
    assert font.dtype == np.uint8 and font.shape == (95, draw.GLYPH_H, draw.GLYPH_W)
    assert 4 <= draw.GLYPH_W <= 32 and 4 <= draw.GLYPH_H <= 32

    def g(ch):
        return font[ord(ch) - 32]

    hollow = g("~")
    assert hollow.any() and not any(np.array_equal(hollow, g(c)) for c in OWN)
    ys, xs = np.nonzero(hollow)                                 # a box: its border is set, its inside is not
    box = hollow[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
    assert box.shape[0] >= 3 and box.shape[1] >= 3
    assert box[0].all() and box[-1].all() and box[:, 0].all() and box[:, -1].all() and not box[1:-1, 1:-1].any()
    assert not g(" ").any()
    for i, a in enumerate(OWN):
        assert g(a).any(), a
        for b in OWN[i + 1:]:
            assert not np.array_equal(g(a), g(b)), (a, b)
    for c in "abcdefghijklmnopqrstuvwxyz":
        assert np.array_equal(g(c.upper()), g(c)), c
    assert np.array_equal(g("A"), g("a"))
    names = json.load(open(os.path.join(HERE, "golden", "class_names.json")))
    assert len(names["voc"]) == 20 and len(names["coco"]) == 80
    text = "".join(names["voc"] + names["coco"]) + ": 0.123456789"
    for ch in sorted(set(text)):
        assert 32 <= ord(ch) <= 126, ch
        if ch == " ":
            assert not g(ch).any()
        elif ch.lower() in OWN:
            assert np.array_equal(g(ch), g(ch.lower())) and g(ch).any(), ch
        else:
            assert np.array_equal(g(ch), hollow), ch
    assert max(len(n) for n in names["voc"] + names["coco"]) <= 32


def score_set():
    """200 208 float32 scores: a random sample, every k / 200, and the two ends with their neighbours."""
    rng = np.random.RandomState(23)
    one, zero = np.float32(1.0), np.float32(0.0)
    ends = [zero, one, np.float32(0.005), np.nextafter(zero, one), np.nextafter(one, zero), np.nextafter(one, np.float32(2.0)), np.float32(1.0049999)]
    s = np.concatenate([rng.random_sample(200000).astype(np.float32), (np.arange(201) / 200.0).astype(np.float32), np.array(ends, dtype=np.float32)])
    assert s.shape == (200208,)
    return s


def test_oracle_score_digits_are_percent_2f():
    bad = 0
    for s in score_set():
        k = orc.score_digits(s)
        assert k is not None
        bad += ("%d.%02d" % (k // 100, k % 100)) != ("%.2f" % float(np.float32(s)))
    assert bad == 0
    assert orc.score_digits(np.float32(1.0051)) is None and orc.score_digits(np.float32(-0.006)) is None
    assert orc.score_digits(np.float32(np.inf)) is None and orc.score_digits(np.float32(np.nan)) is None
    assert orc.score_digits(np.float32(-0.001)) == 0            # the one sign the digits drop: '%.2f' gives '-0.00' (needs vis_thresh < 0)
    assert orc.label_text("dog", 7) == "dog: 0.07" and orc.label_text("dog", 100) == "dog: 1.00"


def test_oracle_mapping_is_rescale_boxes_then_int():
    from yolo_nano_amd.model import ValTransforms, rescale_boxes
    rng = np.random.RandomState(5)
    for (h0, w0), size in (((375, 500), 416), ((500, 333), 416), ((320, 320), 320), ((97, 1279), 128), ((720, 1280), 640), ((1281, 31), 608)):
        rw, rh, left, top, scale, offset = ValTransforms(size).geometry(h0, w0)
        geom = (w0, h0, rw, rh, left, top, size)
        boxes = (rng.random_sample((300, 4)) * 1.4 - 0.2).astype(np.float32)
        ref = rescale_boxes(boxes.copy(), scale, offset, np.array([[w0, h0, w0, h0]]))
        assert ref.dtype == np.float32
        for b, r in zip(boxes, ref):
            m = orc.map_box(b, geom, orc.LETTERBOX)
            assert [int(v) for v in m] == [int(v) for v in r]
            assert [np.float32(v).tobytes() for v in m] == [np.float32(v).tobytes() for v in r]
        assert [float(v) for v in orc.map_box(boxes[0], geom, orc.PIXELS)] == [float(v) for v in boxes[0]]
    assert int(np.float32(-0.5)) == 0                          # int() truncates toward zero
    prims, skipped = orc.select(np.array([[-0.5, -1.5, 3.9, 4.2, 0.9, 0]], np.float32), (8, 8, 0, 0, 0, 0, 0), orc.PIXELS, 0.3, 1)
    assert prims == [(0, 0, -1, 3, 4, 90)] and skipped == 0
