"""Sliced inference on the device (yn_slice_*, kernels_slice.hip) against yn_preprocess_batch on contiguous crops and the host restatement
tests/slice_oracle.py, bit for bit - every comparison is equality.

Shapes: side = tile = 64 (N = 252 predictions per tile), 1.0x, C = 20, random weights, handles with max_batch 4 and 8; frames 100 x 150
(7 tiles), 64 x 64 (1) and 37 x 90 (3: the whole frame resized to 64 x 26, two 64 x 37 tiles with 13 + 14 rows of pad)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights
from yolo_nano_amd.slicing import tile_table, identity_geometry, to_pixels

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slice_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

S, C, N = 64, 20, 252
SHAPES = [(100, 150), (64, 64), (37, 90)]
MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)
CAP = 7 * N                                                      # every prediction of every tile of the largest frame
NMS = 0.5
F = len(SHAPES)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _model(conf, batch):
    import yolo_nano_amd
    model = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, trainable=False, conf_thresh=conf, nms_thresh=NMS,
                                   anchor_size=arch.MULTI_ANCHOR_SIZE, backbone="1.0x")
    model.load_state_dict({k: torch.as_tensor(v) for k, v in weights.make_state_dict("1.0x", C).items()}, strict=False)
    model = model.to("cuda").eval()
    assert model.handle(batch).max_batch == batch
    return model


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    from yolo_nano_amd import capi
    c = Ctx()
    rng = np.random.default_rng(28)
    c.frames = [rng.integers(0, 256, shp + (3,), dtype=np.uint8) for shp in SHAPES]
    c.dev = [torch.from_numpy(f).cuda() for f in c.frames]
    c.tiles = tile_table(SHAPES, S, 0.25, True, S)
    assert [int((c.tiles[:, 0] == f).sum()) for f in range(F)] == [7, 1, 3]
    c.m8, c.m4 = _model(0.001, 8), _model(0.001, 4)
    c.h8, c.h4 = c.m8.handle(8), c.m4.handle(4)
    assert c.h8.N == N
    yield c


def _row(f, x, y, tw, th):
    return (f, x, y, tw, th) + so.letterbox(th, tw, S)


# ---- 1. the tile kernel -----------------------------------------------------------------------------------------------------------------------
def _crops_reference(h, dev, tiles):
    crops = [dev[int(r[0])][int(r[2]):int(r[2]) + int(r[4]), int(r[1]):int(r[1]) + int(r[3])].contiguous() for r in tiles]
    return h.preprocess_batch(crops, [tuple(int(v) for v in r[5:9]) for r in tiles], S, MEAN, STD).cpu().numpy()


def test_preprocess_equals_preprocess_batch_on_contiguous_crops(ctx):
    from yolo_nano_amd import capi
    h = ctx.h8
    sl = capi.Slice(h, F, 16)
    extra = [_row(0, 5, 0, 1, 64), _row(0, 149, 36, 1, 64), _row(0, 10, 20, 128, 64),                 # 1 pixel wide; 128 x 64: the exact 2:1 path
             _row(2, 0, 0, 23, 17), _row(2, 67, 0, 23, 17), _row(2, 0, 20, 23, 17), _row(2, 67, 20, 23, 17),      # a tile in each corner (upscaled)
             _row(0, 0, 0, 1, 1), _row(0, 149, 99, 1, 1), _row(1, 0, 0, 32, 32), _row(0, 22, 36, 128, 64)]
    tiles = np.concatenate([ctx.tiles, np.array(extra, dtype=np.int32)])
    modes = {0 if (r[5] == r[3] and r[6] == r[4]) else (1 if (r[3] == 2 * r[5] and r[4] == 2 * r[6]) else 2) for r in tiles}
    assert modes == {0, 1, 2}                                    # copy, 2:1 area, linear are all in the table
    assert tiles[9].tolist() == [2, 0, 0, 64, 37, 64, 37, 0, 13]
    got = sl.preprocess(ctx.dev, tiles, S, MEAN, STD).cpu().numpy()
    want = _crops_reference(h, ctx.dev, tiles)
    for t in range(len(tiles)):
        assert np.array_equal(_bits(got[t]), _bits(want[t])), (t, tiles[t].tolist())
    # the common tiles alone (tw == th == rw == rh == side): the four-pixels-per-thread path, at every source alignment (3 * (y * 150 + x) mod 4)
    common = np.array([_row(0, x, y, 64, 64) for (x, y) in ((0, 0), (48, 0), (86, 36), (43, 0), (1, 0), (2, 35), (3, 36), (85, 7))] + [_row(1, 0, 0, 64, 64)],
                      dtype=np.int32)
    assert {(3 * (int(r[2]) * 150 + int(r[1]))) % 4 for r in common[:-1]} == {0, 1, 2, 3}
    want = _crops_reference(h, ctx.dev, common)
    got = sl.preprocess(ctx.dev, common, S, MEAN, STD).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    odd = torch.zeros(len(common) * 3 * S * S + 1, dtype=torch.float32, device="cuda")[1:].view(len(common), 3, S, S)      # a 4-byte-offset output
    sl.preprocess(ctx.dev, common, S, MEAN, STD, out=odd)
    assert np.array_equal(_bits(odd.cpu().numpy()), _bits(want))
    many = np.concatenate([common] * 8)                          # more than one launch (64 tiles each)
    got = sl.preprocess(ctx.dev, many, S, MEAN, STD).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(np.concatenate([want] * 8)))
    assert sl.preprocess(ctx.dev, np.zeros((0, 9), np.int32), S, MEAN, STD).shape == (0, 3, S, S)     # T == 0 is not an error
    sl.close()


def test_preprocess_refusals_name_the_tile(ctx):
    from yolo_nano_amd import capi
    h = ctx.h8
    sl = capi.Slice(h, F, 16)
    good = _row(0, 0, 0, 64, 64)

    def refused(row, text, std=STD, t=1):
        with pytest.raises(capi.YnError, match=text):
            sl.preprocess(ctx.dev, np.array([good, row], dtype=np.int32), S, MEAN, std)

    refused(_row(0, 87, 0, 64, 64), "tile 1.*lies outside")
    refused(_row(0, 0, 37, 64, 64), "tile 1.*lies outside")
    refused(_row(0, -1, 0, 64, 64), "tile 1.*lies outside")
    refused((0, 0, 0, 0, 64, 64, 64, 0, 0), "tile 1.*non-positive extent")
    refused((0, 0, 0, 64, -3, 64, 64, 0, 0), "tile 1.*non-positive extent")
    refused((0, 0, 0, 64, 64, 64, 64, 1, 0), "tile 1.*bad letterbox geometry")
    refused((0, 0, 0, 64, 64, 0, 64, 0, 0), "tile 1.*bad letterbox geometry")
    refused((0, 0, 0, 64, 64, 64, 60, 0, 5), "tile 1.*bad letterbox geometry")
    refused((-1, 0, 0, 64, 64, 64, 64, 0, 0), "tile 1 names frame -1")
    refused(good, "std must be positive", std=(0.2, 0.0, 0.2))
    # null pointers: a frame's, and the arrays'
    tiles = np.array([good], dtype=np.int32)
    shapes = np.array(SHAPES, dtype=np.int32)
    ptrs = (ctypes.c_void_p * F)(None, ctx.dev[1].data_ptr(), ctx.dev[2].data_ptr())
    m, sd = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    out = torch.empty((1, 3, S, S), device="cuda")
    args = [h.h, 1, ctypes.cast(ptrs, ctypes.c_void_p), shapes.ctypes.data, tiles.ctypes.data, S, ctypes.cast(m, ctypes.c_void_p),
            ctypes.cast(sd, ctypes.c_void_p), out.data_ptr()]
    assert h.lib.yn_slice_preprocess(*args) == 1 and b"tile 0: frame 0 is a null pointer" in h.lib.yn_last_error(h.h)
    for k in (2, 3, 4, 6, 7, 8):
        bad = list(args)
        bad[k] = None
        assert h.lib.yn_slice_preprocess(*bad) == 1 and b"null pointer" in h.lib.yn_last_error(h.h), k
    sl.close()


# ---- 2. the append, steered: no network --------------------------------------------------------------------------------------------------------
def _around(bound):
    """the bound, the float32 below it and the one above (around 0, where the neighbours are denormals: -2^-20 and 2^-20)"""
    if bound == 0:
        return np.float32(0), np.float32(-2.0 ** -20), np.float32(2.0 ** -20)
    return np.float32(bound), np.nextafter(bound, np.float32(-1e9)), np.nextafter(bound, np.float32(1e9))


def _edge_boxes(tile, shape, m):
    """For an identity-geometry tile (p = 64 b exactly): per side three boxes whose tested coordinate q lies exactly on the filter's bound and
    one ulp to either side of it; the other coordinates sit in the tile's middle."""
    _, x, y, tw, th = [int(v) for v in tile[:5]]
    assert tuple(int(v) for v in tile[3:9]) == (64, 64, 64, 64, 0, 0)
    m = np.float32(max(m, 0.0))
    rows = []
    for side, bound, origin in ((0, np.float32(x) + m, x), (2, np.float32(x + tw) - m, x), (1, np.float32(y) + m, y), (3, np.float32(y + th) - m, y)):
        for q in _around(bound):
            b = np.array([0.375, 0.375, 0.625, 0.625], dtype=np.float32)
            b[side] = (np.float32(q) - np.float32(origin)) / np.float32(64)
            rows.append(b)
    rows = np.array(rows, dtype=np.float32)
    add = np.array([x, y, x, y], dtype=np.float32)
    q = so.unletterbox(rows, tile, S) + add
    for k in range(4):                                           # the construction hits the bound and its two neighbours exactly
        bound = (np.float32(x) + m, np.float32(y) + m, np.float32(x + tw) - m, np.float32(y + th) - m)[k]
        j = {0: 0, 2: 3, 1: 6, 3: 9}[k]
        assert [q[j, k], q[j + 1, k], q[j + 2, k]] == list(_around(bound)), (tile, k)
    return rows


def _steered(tiles, seed=3, marked=()):
    """yn_infer-shaped outputs for the tiles of the table: per tile random boxes (some past the square: clamped at the frame's edge, some inside a
    letterboxed tile's pad), the edge boxes for margins 0 and 2.5 on identity tiles, one object seen by two overlapping tiles of frame 0."""
    rng = np.random.default_rng(seed)
    T = len(tiles)
    boxes = rng.standard_normal((T, N, 4)).astype(np.float32)    # rows past the count are never read: any finite values
    scores = np.zeros((T, N), np.float32)
    cls = np.full((T, N), 7, np.int32)
    count = np.zeros(T, np.int32)
    per = []
    for t, tile in enumerate(tiles):
        k = int(rng.integers(14, 30))
        c = rng.random((k, 2)).astype(np.float32) * np.float32(1.3) - np.float32(0.15)              # centres from -0.15 to 1.15
        wh = rng.random((k, 2)).astype(np.float32) * np.float32(0.3)
        b = np.concatenate([c - wh, c + wh], 1).astype(np.float32)
        b[0] = [-0.25, -0.5, 1.5, 1.25]                          # past every side of the square
        b[1] = [0.3, 0.01, 0.6, 0.1]                             # inside the top pad of a 64 x 37 tile
        if tuple(int(v) for v in tile[3:9]) == (64, 64, 64, 64, 0, 0):
            b = np.concatenate([b, _edge_boxes(tile, SHAPES[int(tile[0])], 0.0), _edge_boxes(tile, SHAPES[int(tile[0])], 2.5)])
        if int(tile[0]) == 0 and (int(tile[1]), int(tile[2])) in ((0, 0), (48, 0)):                  # the object at (50, 10, 62, 30) of frame 0
            x = int(tile[1])
            b = np.concatenate([b, np.array([[(50 - x) / 64, 10 / 64, (62 - x) / 64, 30 / 64]], dtype=np.float32)])
        k = len(b)
        assert k <= N
        s = (rng.permutation(k).astype(np.float32) + np.float32(1)) / np.float32(4 * N) + np.float32(t) / np.float32(4096)      # all different
        l = rng.integers(0, C, k).astype(np.int32)
        if int(tile[0]) == 0 and (int(tile[1]), int(tile[2])) in ((0, 0), (48, 0)):
            s[-1] = 0.9 if int(tile[1]) == 0 else 0.8
            l[-1] = 5
        boxes[t, :k], scores[t, :k], cls[t, :k], count[t] = b, s, l, k
        if t in marked:
            count[t] = -1 - k                                    # the split-f16 range mark
            per.append(None)
        else:
            per.append((b, s, l))
    return (boxes, scores, cls, count), per


def _to_dev(out, lo, hi):
    boxes, scores, cls, count = out
    return (torch.from_numpy(boxes[lo:hi].copy()).cuda(), torch.from_numpy(scores[lo:hi].copy()).cuda(), torch.from_numpy(cls[lo:hi].copy()).cuda(), None,
            torch.from_numpy(count[lo:hi].copy()).cuda())


def _append_all(sl, tiles, out, chunk, margin):
    for t0 in range(0, len(tiles), chunk):
        sl.append(SHAPES, tiles, t0, _to_dev(out, t0, min(t0 + chunk, len(tiles))), margin)


def _check_lists(got, lists, start, cap):
    boxes, scores, cls, count, tstart = got
    assert np.array_equal(tstart, start)
    for f in range(F):
        lb, ls, lc = lists[f]
        n = len(ls)
        assert int(count[f]) == n, f
        w = min(n, cap)
        assert np.array_equal(_bits(boxes[f, :w]), _bits(lb[:w])), f
        assert np.array_equal(_bits(scores[f, :w]), _bits(ls[:w])), f
        assert np.array_equal(cls[f, :w], lc[:w]), f
        assert (cls[f, w:] == -1).all(), f


def _check_result(res, lists):
    rec, off, total = res
    rec, off = rec.cpu().numpy(), off.cpu().numpy()
    assert off.shape == (F + 1,) and off[0] == 0 and int(off[-1]) == total and (np.diff(off) >= 0).all()
    for f in range(F):
        kb, ks, kc = so.merge(lists[f], C, NMS)
        r = rec[off[f]:off[f + 1]]
        assert len(r) == len(ks), f
        assert np.array_equal(_bits(r[:, :4]), _bits(kb)) and np.array_equal(_bits(r[:, 4]), _bits(ks)) and np.array_equal(r[:, 5].astype(np.int64), kc), f
    return rec, off


@pytest.mark.parametrize("margin", [-1.0, 0.0, 2.5])
def test_append_equals_the_oracle_whatever_the_chunking(ctx, margin):
    from yolo_nano_amd import capi
    h = ctx.h8
    out, per = _steered(ctx.tiles)
    lists, start, mark = so.build_lists(F, SHAPES, ctx.tiles, per, S, margin)
    assert not mark
    if margin >= 0:                                              # the filter dropped rows, but not on sides that lie on the frame's edge
        all_lists = so.build_lists(F, SHAPES, ctx.tiles, per, S, -1.0)[0]
        assert len(lists[0][1]) < len(all_lists[0][1]) and len(lists[1][1]) == len(all_lists[1][1])
    sl = capi.Slice(h, F, CAP)
    for chunk in (len(ctx.tiles), 4, 8, 1):
        _append_all(sl, ctx.tiles, out, chunk, margin)
        _check_lists(sl.lists_to_host(), lists, start, CAP)
    with pytest.raises(capi.YnError, match="table order"):
        sl.append(SHAPES, ctx.tiles, 3, _to_dev(out, 3, 5), margin)      # the table is complete: tile 3 does not continue it
    h.set_grid_rect(32, 64, 64, 0, 16)
    with pytest.raises(capi.YnError, match="needs a square grid"):
        sl.append(SHAPES, ctx.tiles, 0, _to_dev(out, 0, 4), margin)
    h.set_grid(S)
    sl.close()


def test_append_range_mark_and_merge(ctx):
    """A negative count sets the object's mark and appends nothing of that tile; the merge then delivers nothing.  Without it the merge equals
    the oracle's, and the object seen by two overlapping tiles is kept once."""
    from yolo_nano_amd import capi
    h = ctx.h8
    sl = capi.Slice(h, F, CAP)
    out, per = _steered(ctx.tiles, marked=(2, 9))
    lists, start, mark = so.build_lists(F, SHAPES, ctx.tiles, per, S, -1.0)
    assert mark
    _append_all(sl, ctx.tiles, out, 4, -1.0)
    _check_lists(sl.lists_to_host(), lists, start, CAP)
    with pytest.raises(capi.YnRangeError):
        sl.merge(F, NMS)
    with pytest.raises(capi.YnError):
        sl.result()
    assert h.range_status() == (False, False)                    # the mark was the object's, not the handle's
    out, per = _steered(ctx.tiles)
    lists, start, _ = so.build_lists(F, SHAPES, ctx.tiles, per, S, -1.0)
    _append_all(sl, ctx.tiles, out, 8, -1.0)
    sl.merge(F, NMS)
    rec, off = _check_result(sl.result(total=True), lists)
    # the duplicate: both rows are in frame 0's list, the 0.9 one survives alone among class 5 boxes that overlap it
    obj = (np.array([50, 10, 62, 30], dtype=np.float32) / np.float32(150))
    in_list = [(s, c) for b, s, c in zip(*lists[0]) if np.array_equal(b, obj)]
    assert sorted(s for s, _ in in_list) == [np.float32(0.8), np.float32(0.9)] and all(c == 5 for _, c in in_list)
    kept = [r for r in rec[off[0]:off[1]] if np.array_equal(r[:4], obj)]
    assert len(kept) == 1 and kept[0][4] == np.float32(0.9)
    with pytest.raises(capi.YnError, match="lists hold 3 frames"):
        sl.merge(2, NMS)
    sl.close()


def test_list_capacity_exactly_and_one_short(ctx):
    from yolo_nano_amd import capi
    h = ctx.h8
    out, per = _steered(ctx.tiles)
    lists, start, _ = so.build_lists(F, SHAPES, ctx.tiles, per, S, -1.0)
    sizes = [len(l[1]) for l in lists]
    need = max(sizes)
    assert sizes[0] == need and need > sizes[2] > sizes[1]       # frame 0 holds the longest list
    exact = capi.Slice(h, F, need)
    _append_all(exact, ctx.tiles, out, 4, -1.0)
    _check_lists(exact.lists_to_host(), lists, start, need)
    exact.merge(F, NMS)
    _check_result(exact.result(total=True), lists)
    exact.close()
    short = capi.Slice(h, F, need - 1)
    _append_all(short, ctx.tiles, out, 4, -1.0)
    with pytest.raises(capi.YnError) as e:
        short.merge(F, NMS)
    assert "frame 0 needs %d rows" % need in str(e.value) and "list_capacity is %d" % (need - 1) in str(e.value)
    with pytest.raises(capi.YnError):
        short.result()                                           # nothing is delivered
    _check_lists(short.lists_to_host(), lists, start, need - 1)  # nothing was written past the list; the sizes are the needed ones
    short.close()
    with pytest.raises(capi.YnError, match="list_capacity 0 outside"):
        capi.Slice(h, F, 0)
    with pytest.raises(capi.YnError, match="list_capacity 131073 outside"):
        capi.Slice(h, F, 131073)


# ---- 3. the whole route -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route(ctx):
    """yn_slice_infer on the handle with max_batch 8, and its reference: the per-tile kept rows of yn_infer on the identical tile batches."""
    from yolo_nano_amd import capi
    c = ctx
    c.margin = 2.5
    c.sl8 = capi.Slice(c.h8, F, CAP)
    c.sl8.infer(c.dev, c.tiles, MEAN, STD, NMS, c.margin)
    assert c.h8.S == S and c.h8.shape == (S, S, S, 0, 0)        # the grid is as it was
    c.res8 = c.sl8.result(total=True)
    c.lists8 = c.sl8.lists_to_host()
    x = c.sl8.preprocess(c.dev, c.tiles, S, MEAN, STD)
    c.per = []
    for t0 in range(0, len(c.tiles), 8):
        boxes, scores, cls, _, count = [t.cpu().numpy() for t in c.h8.infer(x[t0:t0 + 8])]
        assert (count >= 0).all()
        for j in range(len(count)):
            k = int(count[j])
            c.per.append((boxes[j, :k].copy(), scores[j, :k].copy(), cls[j, :k].copy()))
    c.lists, c.start, _ = so.build_lists(F, SHAPES, c.tiles, c.per, S, c.margin)
    return c


def test_infer_equals_the_oracle_on_the_per_tile_rows(route):
    c = route
    assert sum(len(p[1]) for p in c.per) > 50 and all(len(l[1]) > 0 for l in c.lists)
    _check_lists(c.lists8, c.lists, c.start, CAP)
    rec, off = _check_result(c.res8, c.lists)
    assert int(off[-1]) > 0
    assert (rec[: off[-1], :4] >= 0).all() and (rec[: off[-1], :4] <= 1).all()
    px = to_pixels(rec[off[0]:off[1], :4], *SHAPES[0])
    assert px[:, [0, 2]].max() <= 150 and px[:, [1, 3]].max() <= 100


def test_chunk_boundaries_do_not_matter(route):
    from yolo_nano_amd import capi
    c = route
    sl4 = capi.Slice(c.h4, F, CAP)
    sl4.infer(c.dev, c.tiles, MEAN, STD, NMS, c.margin)
    r4, o4, n4 = sl4.result(total=True)
    r8, o8, n8 = c.res8
    assert n4 == n8 and np.array_equal(o4.cpu().numpy(), o8.cpu().numpy())
    assert np.array_equal(_bits(r4[:n4].cpu().numpy()), _bits(r8[:n8].cpu().numpy()))
    got = sl4.lists_to_host()
    for a, b in zip(got, c.lists8):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    sl4.close()


def test_refusals_and_empty_calls(route):
    from yolo_nano_amd import capi
    c = route
    h = c.h4
    sl = capi.Slice(h, F, CAP)
    h.set_grid_rect(32, 64, 64, 0, 16)
    with pytest.raises(capi.YnError, match="yn_slice_infer needs a square grid"):
        sl.infer(c.dev, c.tiles, MEAN, STD, NMS)
    assert h.shape == (32, 64, 64, 0, 16)                        # refused before anything was touched
    h.set_grid(S)
    with pytest.raises(capi.YnError):
        sl.result()
    sl.infer([], np.zeros((0, 9), np.int32), MEAN, STD, NMS)     # F == 0
    assert sl.result(total=True)[2] == 0
    sl.infer(c.dev, np.zeros((0, 9), np.int32), MEAN, STD, NMS)  # T == 0
    rec, off, total = sl.result(total=True)
    assert total == 0 and off.cpu().numpy().tolist() == [0] * (F + 1)
    assert (sl.lists_to_host()[3] == 0).all()
    bad = c.tiles.copy()
    bad[4, 1] = 90                                               # 90 + 64 > 150
    with pytest.raises(capi.YnError, match="tile 4.*lies outside"):
        sl.infer(c.dev, bad, MEAN, STD, NMS)
    bad = c.tiles.copy()
    bad[10, 0] = 3
    with pytest.raises(capi.YnError, match="tile 10 names frame 3 of 3"):
        sl.infer(c.dev, bad, MEAN, STD, NMS)
    with pytest.raises(capi.YnError, match="max_frames is 3"):
        sl.infer(c.dev + c.dev, c.tiles, MEAN, STD, NMS)
    sl.infer(c.dev, c.tiles, MEAN, STD, NMS, c.margin)           # and the object still works
    assert sl.result(total=True)[2] == c.res8[2]
    sl.close()


def test_shim_batch_records_evaluators_and_painter(route):
    import yolo_nano_amd
    from yolo_nano_amd import VOCEval, Visualizer, evaluate
    c = route
    model = c.m8
    sl = yolo_nano_amd.SlicedInference(tile=S, overlap=0.25, nms_thresh=NMS, edge_margin=c.margin, list_capacity=CAP)
    sl.chunk = 8                                                 # the model's handle takes 8 tiles per forward
    rec, off, geoms = sl.records(c.frames, model)
    assert geoms == [identity_geometry(*shp) for shp in SHAPES] and geoms[0] == (150, 100, 150, 100, 0, 0, 150)
    r8, o8, n8 = c.res8
    assert np.array_equal(off.cpu().numpy(), o8.cpu().numpy()) and np.array_equal(_bits(rec[:n8].cpu().numpy()), _bits(r8[:n8].cpu().numpy()))
    trip = sl.batch(c.dev, model)                                # device tensors go in as they are
    host, o = r8[:n8].cpu().numpy(), o8.cpu().numpy()
    for f in range(F):
        q = host[o[f]:o[f + 1]]
        assert np.array_equal(_bits(trip[f][0]), _bits(q[:, :4])) and np.array_equal(_bits(trip[f][1]), _bits(q[:, 4]))
        assert np.array_equal(trip[f][2], q[:, 5].astype(np.int64)) and trip[f][2].dtype == np.int64
    model.set_grid(96)
    with pytest.raises(yolo_nano_amd.YnError, match="set_grid"):
        sl.records(c.frames, model)
    model.set_grid(S)
    # the records go into the evaluator and the painter unchanged, with the identity geometry
    rng = np.random.default_rng(21)
    annots = []
    for (h0, w0) in SHAPES:
        x1, y1 = rng.integers(0, w0 - 30, 3), rng.integers(0, h0 - 30, 3)
        annots.append(np.stack([x1, y1, x1 + rng.integers(5, 30, 3), y1 + rng.integers(5, 30, 3), rng.integers(0, C, 3), np.zeros(3, dtype=np.int64)],
                               1).astype(np.int32))
    h = model.handle(8)
    rec, off, geoms = sl.records(c.frames, model)
    ev = VOCEval(C, 0.5, handle=h)
    ev.add(rec, off, geoms, annots, handle=h)
    aps, mAP = ev.compute(True, handle=h)
    ev.close()
    ref = VOCEval(C, 0.5, handle=h)
    ref.add_host(trip, geoms, annots, handle=h)
    raps, rmAP = ref.compute(True, handle=h)
    ref.close()
    assert np.array_equal(aps, raps) and (mAP == rmAP or (np.isnan(mAP) and np.isnan(rmAP)))
    eaps, emAP = evaluate(model, c.frames, annots, batch=2, use_07_metric=True, sliced=sl)      # two batches: 2 + 1 frames
    assert np.array_equal(eaps, raps) and (emAP == rmAP or (np.isnan(emAP) and np.isnan(rmAP)))
    # the COCO route: evaluate_coco(sliced=...) == COCOEval fed with batch()'s triples and the identity geometry
    from yolo_nano_amd import COCOEval, evaluate_coco
    ids = [7, 3, 11]
    cgt = [np.stack([a[:, 0], a[:, 1], a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), a[:, 4], np.zeros(len(a))],
                    1).astype(np.float64) for a in annots]
    ap50, ap = evaluate_coco(model, c.frames, ids, cgt, batch=2, sliced=sl)
    cref = COCOEval(C, handle=h)
    cref.add_host(trip, geoms, ids, cgt, handle=h)
    stats = cref.compute(handle=h)
    cref.close()
    assert ap50 == stats[1] and ap == stats[0]
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate(model, c.frames, annots, sliced=sl, rect=True)
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate(model, c.frames, annots, sliced=sl, test_aug=yolo_nano_amd.TestTimeAugmentation(num_classes=C))
    rec, off, geoms = sl.records(c.frames, model)
    vis = Visualizer([], vis_thresh=0.0, handle=h, num_classes=C)
    painted = [d.clone() for d in c.dev]
    vis.batch(painted, rec, off, geoms, handle=h)
    st = vis.status(h)
    assert st["drawn"] == int(off[-1].item()) > 0 and st["skipped"] == 0 and not st["range_mark"]
    assert any(not torch.equal(p, d) for p, d in zip(painted, c.dev))
    vis.close()


def test_a_small_handle_is_used_as_it_is_and_said_so(route):
    """The model made for 4 images per forward keeps its handle: the tiles run 4 at a time, the result is the same, one warning says so."""
    import yolo_nano_amd
    c = route
    sl = yolo_nano_amd.SlicedInference(tile=S, overlap=0.25, nms_thresh=NMS, edge_margin=c.margin, list_capacity=CAP)
    with pytest.warns(UserWarning, match="4 at a time instead of 32"):
        rec, off, _ = sl.records(c.dev, c.m4)
    r8, o8, n8 = c.res8
    assert np.array_equal(off.cpu().numpy(), o8.cpu().numpy()) and np.array_equal(_bits(rec[:n8].cpu().numpy()), _bits(r8[:n8].cpu().numpy()))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sl.records(c.dev, c.m4)                                  # once
