"""Without a GPU: tests/rect_cases.py's float64 restatement of rectangular grids is tied to the project's pinned decode reference
(decode_cases.decode_ref), rect_window does what its contract says, and the new entries are declared in the header and in capi.py."""
import os
import re

import numpy as np
import pytest

import decode_cases as dc
import rect_cases as rc
from yolo_nano_amd import rect_window
from yolo_nano_amd.model import ValTransforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("yn_set_grid_rect", "yn_grid_shape", "yn_create_grid_rect", "yn_preprocess_batch_rect")


@pytest.mark.parametrize("C", [20, 80])
@pytest.mark.parametrize("S", dc.DECODE_S)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_whole_square_is_decode_ref(C, S, dtype):
    heads = dc.random_heads(C, S)
    a, b = rc.rect_ref(heads, S, S, S, 0, 0, C, dtype), dc.decode_ref(heads, S, C, dtype)
    for k in b:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert rc.num_pred(S, S) == dc.num_pred(S)
    for u, v in zip(rc.geometry(S, S), dc.geometry(S)):
        assert np.array_equal(u, v)
    o, c, t = dc.unpack_heads(heads, C)
    for u, v in zip(rc.pack_heads(o, c, t, S, S), heads):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("win", [(32, 96, 64, 32), (96, 32, 0, 96), (64, 160, 32, 64), (192, 192, 0, 0)])
def test_window_shifted_by_whole_cells_is_the_square_decode(win):
    """the H x W window at (left, top), both multiples of 32, of a 192 square: its candidates are the square's candidates of those cells - the
    class scores bit for bit, the boxes to float64 rounding ((sigmoid + gx) * stride + left against (sigmoid + gx + left / stride) * stride)"""
    H, W, left, top = win
    S, C = 192, 20
    heads = dc.random_heads(C, S)
    sq = dc.decode_ref(heads, S, C)
    sub = rc.window_of_square(heads, S, H, W, left, top)
    r = rc.rect_ref(sub, H, W, S, left, top, C)
    idx = rc.window_candidates(S, H, W, left, top)
    assert len(idx) == rc.num_pred(H, W) and len(np.unique(idx)) == len(idx)
    assert np.array_equal(r["all_class"], sq["all_class"][:, idx])
    assert np.array_equal(r["best"], sq["best"][:, idx])
    assert np.abs(r["pre_clamp"] - sq["pre_clamp"][:, idx]).max() < 1e-12
    assert np.abs(r["all_bbox"] - sq["all_bbox"][:, idx]).max() < 1e-12


def test_rect_ref_normalises_both_axes_by_the_side():
    """a box of known canvas pixels: x moves by left, y by top, both divide by side"""
    H, W, C = 32, 96, 20
    side, left, top = 192, 13, 71
    heads = rc.random_heads(C, H, W)
    r = rc.rect_ref(heads, H, W, side, left, top, C)
    want = (r["pixels"] + np.asarray([left, top, left, top], np.float64)) / side
    assert np.array_equal(r["pre_clamp"], want)
    assert np.array_equal(r["all_bbox"], np.clip(want, 0.0, 1.0))
    assert r["all_bbox"].shape == (rc.B, rc.num_pred(H, W), 4) and rc.num_pred(H, W) == 3 * (4 * 12 + 2 * 6 + 1 * 3)
    d = rc.rect_ref(heads, H, W, *rc.default_window(H, W), C)
    assert rc.default_window(H, W) == (96, 0, 32)
    assert np.array_equal(d["pre_clamp"], (r["pixels"] + np.asarray([0, 32, 0, 32], np.float64)) / 96)


def test_steered_heads_reach_the_borders():
    for H, W in rc.DECODE_GRIDS:
        heads = rc.steered_heads(20, H, W)
        assert [h.shape for h in heads] == [(rc.B, h, w, 75) for h, w in rc.maps(H, W)]
        _, _, t = rc.unpack_heads(heads, 20)
        sc, gx, gy, an = rc.geometry(H, W)
        for s, (h, w) in enumerate(rc.maps(H, W)):
            for name, m in (("col0", gx == 0), ("row0", gy == 0), ("colw", gx == w - 1), ("rowh", gy == h - 1)):
                assert np.isin(t[:, m & (sc == s), 2], dc.TWH).all(), (H, W, s, name)


# ---- rect_window ----------------------------------------------------------------------------------------------------------------------
def _geoms(frames, side):
    tf = ValTransforms(side)
    out = []
    for h0, w0 in frames:
        rw, rh, left, top = tf.geometry(h0, w0)[:4]
        out.append((w0, h0, rw, rh, left, top, side))
    return out


def _check_window(geoms, side, win, multiple=32):
    left, top, W, H = win
    assert W % multiple == 0 and H % multiple == 0 and W > 0 and H > 0
    assert 0 <= left and left + W <= side and 0 <= top and top + H <= side
    for g in geoms:
        assert left <= g[4] and g[4] + g[2] <= left + W and top <= g[5] and g[5] + g[3] <= top + H, (g, win)


def test_rect_window_of_16_9_frames():
    geoms = _geoms(rc.FRAMES_16_9, 160)
    assert [g[2:6] for g in geoms] == [(160, 90, 0, 35)] * 3
    win = rect_window(geoms, 160)
    assert win == (0, 32, 160, 96)
    _check_window(geoms, 160, win)
    assert rect_window([g[2:6] for g in geoms], 160) == win            # the 4-field rows ValTransforms.geometry gives


def test_rect_window_with_a_portrait_frame_is_the_whole_square():
    geoms = _geoms(rc.FRAMES_16_9 + ((160, 90),), 160)
    assert rect_window(geoms, 160) == (0, 0, 160, 160)


def test_rect_window_properties():
    rs = np.random.RandomState(5)
    for side in (160, 320, 416, 640):
        for _ in range(40):
            frames = [(int(rs.randint(8, 900)), int(rs.randint(8, 900))) for _ in range(rs.randint(1, 5))]
            frames = [(h, w) for h, w in frames if min(h, w) * side // max(h, w) >= 1]
            if not frames:
                continue
            geoms = _geoms(frames, side)
            win = rect_window(geoms, side)
            _check_window(geoms, side, win)
            left, top, W, H = win
            x0, x1 = min(g[4] for g in geoms), max(g[4] + g[2] for g in geoms)
            y0, y1 = min(g[5] for g in geoms), max(g[5] + g[3] for g in geoms)
            assert W - (x1 - x0) < 32 and H - (y1 - y0) < 32               # the smallest such extents
            for lo, hi, start, n in ((x0, x1, left, W), (y0, y1, top, H)):  # centred, unless the square's edge is in the way
                centred = (lo + hi - n) // 2
                assert start == min(max(centred, 0), side - n)
    assert rect_window([(1280, 720, 640, 360, 0, 140, 640)], 640) == (0, 128, 640, 384)
    assert rect_window([(10, 10, 100, 100, 30, 30, 160)], 160, multiple=64) == (16, 16, 128, 128)
    with pytest.raises(ValueError):
        rect_window([], 160)
    with pytest.raises(ValueError):
        rect_window([(10, 10, 100, 100, 100, 30, 160)], 160)               # an extent outside the square


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared():
    header = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    from yolo_nano_amd import capi
    table = capi.SIGNATURES
    src = open(os.path.join(ROOT, "yolo-nano_amd", "capi.py")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert re.search(r'"%s"\s*:' % name, src), name
        assert name in table, name
    for method in ("set_grid_rect", "shape", "preprocess_batch_rect"):
        assert hasattr(capi.Handle, method), method
