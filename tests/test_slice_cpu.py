"""Sliced inference, the host part (yolo-nano_amd/slicing.py): slice_grid's properties over a sweep, its refusals, the 1280x720 example,
tile_table against ValTransforms.geometry, the restatement tests/slice_oracle.py on hand-worked values, and the ABI's three tables."""
import os
import re
import sys

import numpy as np
import pytest

from yolo_nano_amd import slicing
from yolo_nano_amd.slicing import slice_grid, tile_table

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slice_oracle as so  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["yn_slice_create", "yn_slice_destroy", "yn_slice_preprocess", "yn_slice_append", "yn_slice_merge", "yn_slice_infer", "yn_slice_result",
               "yn_slice_lists"]


# ---- slice_grid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [32, 64, 96, 416])
def test_slice_grid_axis_properties(tile):
    """Per axis (a w0 = n, h0 = 1 frame): every pixel covered, every tile inside the frame, neighbours overlap by at least int(tile * overlap),
    the count is 1 or ceil((n - tile) / step) + 1."""
    for overlap in (0, 0.2, 0.5, 0.9):
        ov = int(tile * overlap)
        step = tile - ov
        for n in range(1, 700):
            rects = slice_grid(1, n, tile, overlap, full_frame=False)
            xs = [r[0] for r in rects]
            assert all(r[1] == 0 and r[3] == 1 and r[2] == min(tile, n) for r in rects)
            assert xs == sorted(set(xs)) and xs[0] == 0
            assert all(0 <= x and x + min(tile, n) <= n for x in xs)
            assert xs[-1] + min(tile, n) == n                                            # the last tile ends on the frame's edge
            covered = np.zeros(n, dtype=bool)
            for x in xs:
                covered[x:x + tile] = True
            assert covered.all()
            for a, b in zip(xs, xs[1:]):
                assert a + tile - b >= ov, (n, tile, overlap, a, b)
            assert len(xs) == (1 if n <= tile else -(-(n - tile) // step) + 1)
            assert xs == so.axis_origins(n, tile, overlap)


def test_slice_grid_two_axes_order_and_full_frame():
    for (h0, w0) in ((100, 150), (64, 64), (37, 90), (720, 1280), (500, 90), (1, 1)):
        for tile in (64, 416):
            for overlap in (0, 0.25):
                for full in (False, True):
                    rects = slice_grid(h0, w0, tile, overlap, full)
                    assert rects == so.slice_grid(h0, w0, tile, overlap, full)
                    body = rects[1:] if (full and len(rects) > 1) else rects
                    assert body == sorted(body, key=lambda r: (r[1], r[0]))              # row-major, y outer
                    if full:
                        assert rects[0] == (0, 0, w0, h0) and rects.count((0, 0, w0, h0)) == 1
    assert slice_grid(64, 64, 64) == [(0, 0, 64, 64)]                                    # the only tile anyway: not doubled
    assert slice_grid(30, 40, 64) == [(0, 0, 40, 30)]
    assert len(slice_grid(100, 150, 64, 0.25)) == 7 and len(slice_grid(37, 90, 64, 0.25)) == 3


def test_the_1280x720_example():
    rects = slice_grid(720, 1280, 416, 0.2)
    assert len(rects) == 9 and rects[0] == (0, 0, 1280, 720)
    assert [r[0] for r in rects[1:5]] == [0, 333, 666, 864] and sorted({r[1] for r in rects[1:]}) == [0, 304]
    assert all(r[2:] == (416, 416) for r in rects[1:])
    assert len(tile_table([(720, 1280)] * 32, 416, 0.2, True, 416)) == 288


def test_slice_grid_refusals():
    for bad in (1.0, 1.5, -0.5):
        with pytest.raises(ValueError, match="step"):
            slice_grid(100, 100, 64, bad)
    for args in ((0, 10, 64), (10, 0, 64), (10, 10, 0)):
        with pytest.raises(ValueError, match="positive"):
            slice_grid(*args)
    with pytest.raises(ValueError):
        slicing.SlicedInference(tile=64, overlap=1.0)


# ---- tile_table ---------------------------------------------------------------------------------------------------------------------------
def test_tile_table_against_val_transforms_geometry():
    from yolo_nano_amd import ValTransforms
    shapes = [(100, 150), (64, 64), (37, 90), (720, 1280), (333, 7)]
    for side, tile in ((64, 64), (416, 416), (96, 64)):
        tab = tile_table(shapes, tile, 0.25, True, side)
        assert tab.dtype == np.int32 and tab.shape[1] == 9
        assert np.array_equal(tab, so.tile_table(shapes, tile, 0.25, True, side))
        vt = ValTransforms(side)
        t = 0
        for f, (h0, w0) in enumerate(shapes):
            for (x, y, tw, th) in slice_grid(h0, w0, tile, 0.25, True):
                assert tab[t].tolist() == [f, x, y, tw, th] + [int(v) for v in vt.geometry(th, tw)[:4]]
                t += 1
        assert t == len(tab)
    tab = tile_table([(100, 150), (64, 64), (37, 90)], 64, 0.25, True, 64)
    assert [int((tab[:, 0] == f).sum()) for f in range(3)] == [7, 1, 3]
    assert tab[8].tolist() == [2, 0, 0, 90, 37, 64, 26, 0, 19]                           # the 37 x 90 frame whole: int(37 / 90 * 64) = 26 rows
    assert tab[9].tolist() == [2, 0, 0, 64, 37, 64, 37, 0, 13]                           # its 64 x 37 tiles: 13 + 14 rows of pad
    assert tile_table([], 64).shape == (0, 9)


# ---- the remap, hand-worked -----------------------------------------------------------------------------------------------------------------
def test_remap_on_hand_worked_values():
    # a 64 x 64 tile at (86, 36) of a 100 x 150 frame, side 64: p = b * 64 exactly, q = p + (86, 36), v = q / 150
    tile = (0, 86, 36, 64, 64, 64, 64, 0, 0)
    b = np.array([[0.25, 0.5, 0.75, 1.0], [0.0, 0.0, 1.0, 1.0], [-0.5, -1.0, 2.0, 2.0]], dtype=np.float32)
    v, keep = so.remap(b, tile, (100, 150), 64, -1.0)
    want = np.array([[102, 68, 134, 100], [86, 36, 150, 100], [54, 0, 150, 100]], dtype=np.float32) / np.float32(150)
    assert keep.all() and np.array_equal(v, want)
    # margin 2.5: left and top sides are cut (x, y > 0), right and bottom lie on the frame's edge and never drop
    b = np.array([[2.5 / 64, 0.5, 1.0, 1.0],        # x1 exactly at x + m: stays (strict compare)
                  [2.0 / 64, 0.5, 1.0, 1.0],        # inside the margin: dropped
                  [0.5, 2.5 / 64, 1.0, 1.0],        # y1 exactly at y + m: stays
                  [0.5, 0.0, 1.0, 1.0],             # dropped
                  [0.5, 0.5, 1.0, 1.0]], dtype=np.float32)
    _, keep = so.remap(b, tile, (100, 150), 64, 2.5)
    assert keep.tolist() == [True, False, True, False, True]
    # the same tile at the frame's origin: left / top exempt, right / bottom cut
    tile0 = (0, 0, 0, 64, 64, 64, 64, 0, 0)
    b = np.array([[0.0, 0.0, 61.5 / 64, 0.5], [0.0, 0.0, 62.0 / 64, 0.5], [0.0, 0.0, 0.5, 62.0 / 64], [0.0, 0.0, 0.5, 0.5]], dtype=np.float32)
    _, keep = so.remap(b, tile0, (100, 150), 64, 2.5)
    assert keep.tolist() == [True, False, False, True]
    # a letterboxed tile: the 37 x 90 frame whole in 64 (26 rows at top 19): y = (b - 19/64) / (26/64) * 37, x = b * 90
    full = (0, 0, 0, 90, 37, 64, 26, 0, 19)
    b = np.array([[0.5, 19 / 64, 1.0, 45 / 64], [0.0, 0.0, 1.0, 1.0]], dtype=np.float32)      # the second reaches into the pad: clamped
    v, keep = so.remap(b, full, (37, 90), 64, 2.5)
    assert keep.all()                                                                    # every side on the frame's edge
    assert np.array_equal(v, np.array([[45, 0, 90, 37], [0, 0, 90, 37]], dtype=np.float32) / np.float32(90))
    # float64 steps, float32 results: not the float32 chain
    p = so.unletterbox(np.array([[0.3, 0.3, 0.7, 0.7]], dtype=np.float32), (0, 0, 0, 64, 37, 64, 37, 0, 13), 64)
    y = np.float32(np.float64(np.float32(np.float64(np.float32(np.float64(np.float32(0.3)) - 13 / 64)) / (37 / 64))) * 37.0)
    assert p.dtype == np.float32 and p[0, 1] == y


def test_build_lists_order_and_range_mark():
    tiles = np.array([(0, 0, 0, 64, 64, 64, 64, 0, 0), (1, 0, 0, 64, 64, 64, 64, 0, 0), (0, 36, 0, 64, 64, 64, 64, 0, 0)], dtype=np.int32)
    one = (np.array([[0.25, 0.25, 0.5, 0.5]], np.float32), np.array([0.9], np.float32), np.array([3]))
    lists, start, mark = so.build_lists(2, [(64, 100), (64, 64)], tiles, [one, None, one], 64, -1.0)
    assert mark and start.tolist() == [0, 0, 1]
    assert len(lists[0][1]) == 2 and len(lists[1][1]) == 0
    assert np.array_equal(lists[0][0], np.array([[16, 16, 32, 32], [52, 16, 68, 32]], np.float32) / np.float32(100))


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_header_table_and_binding():
    header = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from yolo_nano_amd import capi
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    for method in ("preprocess", "append", "merge", "infer", "result", "lists_to_host"):
        assert hasattr(capi.Slice, method), method
    import yolo_nano_amd
    assert yolo_nano_amd.SlicedInference is slicing.SlicedInference and yolo_nano_amd.slice_grid is slice_grid


def test_evaluate_exclusions_need_no_device():
    from yolo_nano_amd import evaluate, evaluate_coco

    class M:
        input_size = 64
    sl = slicing.SlicedInference(tile=64)
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate(M(), [], [], sliced=sl, rect=True)
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate(M(), [], [], sliced=sl, test_aug=object())
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate_coco(M(), [], [], [], sliced=sl, rect=True)
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate_coco(M(), [], [], [], sliced=sl, test_aug=object())
