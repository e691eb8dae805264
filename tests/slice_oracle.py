"""Host restatement of sliced inference (yn_slice_*, kernels_slice.hip) in numpy: the tile grid and table, the remap of a tile's
boxes into its frame operation by operation, the list building, and the per-frame merge (oracle.tta_merge with one forward: per-class NMS
in YOLONano.nms' arithmetic, kept rows in list order).

The remap of a box b in [0,1] of the tile's side x side square, tile (x, y, tw, th, rw, rh, left, top) of an h0 x w0 frame:
    p = b - off; p /= scale; p *= size     the evaluators' three steps: float64 operands, each result rounded to float32
                                           (off = left/side, top/side; scale = rw/side, rh/side; size = tw, th)
    q = p + float32(x or y)                one float32 add
    edge filter (margin m >= 0 only)       dropped if  x > 0 and q.x1 < float32(x) + m,  x + tw < w0 and q.x2 > float32(x + tw) - m, same in y
    q = 0 if q < 0 else (hi if q > hi else q),  hi = w0 or h0
    v = q / float32(max(h0, w0))           one float32 divide
numpy rounds every ufunc call on its own, so each line below is one rounding."""
import numpy as np

F32 = np.float32


# ---- the grid (written from the specification, not from slicing.py) -------------------------------------------------------------------------
def axis_origins(n, tile, overlap):
    step = tile - int(tile * overlap)
    assert 1 <= step <= tile
    last = max(n - tile, 0)
    o = list(range(0, last + 1, step))
    if o[-1] != last:
        o.append(last)
    return o


def slice_grid(h0, w0, tile, overlap=0.2, full_frame=True):
    tw, th = min(tile, w0), min(tile, h0)
    rects = [(x, y, tw, th) for y in axis_origins(h0, tile, overlap) for x in axis_origins(w0, tile, overlap)]
    if full_frame and rects != [(0, 0, w0, h0)]:
        rects = [(0, 0, w0, h0)] + rects
    return rects


def letterbox(th, tw, side):
    """Resize.__call__ (data/transforms.py:79-116) on a th x tw image: (rw, rh, left, top)"""
    if th > tw:
        r = tw / th
        w = int(r * side)
        return w, side, (side - w) // 2, 0
    if th < tw:
        r = th / tw
        h = int(r * side)
        return side, h, 0, (side - h) // 2
    return side, side, 0, 0


def tile_table(shapes, tile, overlap, full_frame, side):
    rows = []
    for f, (h0, w0) in enumerate(shapes):
        for (x, y, tw, th) in slice_grid(h0, w0, tile, overlap, full_frame):
            rows.append((f, x, y, tw, th) + letterbox(th, tw, side))
    return np.array(rows, dtype=np.int32).reshape(-1, 9)


# ---- the remap ----------------------------------------------------------------------------------------------------------------------------
def unletterbox(b, tile, side):
    """[K,4] float32 -> tile pixels, float64 steps rounded to float32 (vocapi_evaluator.py:72-74 on a float32 array)"""
    _, x, y, tw, th, rw, rh, left, top = [int(v) for v in tile]
    side = float(side)
    off = np.array([left / side, top / side] * 2, dtype=np.float64)
    sc = np.array([rw / side, rh / side] * 2, dtype=np.float64)
    size = np.array([tw, th] * 2, dtype=np.float64)
    v = np.asarray(b, dtype=np.float32).reshape(-1, 4)
    v = (v.astype(np.float64) - off).astype(np.float32)
    v = (v.astype(np.float64) / sc).astype(np.float32)
    v = (v.astype(np.float64) * size).astype(np.float32)
    return v


def remap(b, tile, shape, side, margin):
    """-> (v [K,4] float32 normalised by max(h0, w0), keep [K] bool)"""
    _, x, y, tw, th = [int(v) for v in tile[:5]]
    h0, w0 = int(shape[0]), int(shape[1])
    p = unletterbox(b, tile, side)
    add = np.array([x, y, x, y], dtype=np.float32)
    q = p + add
    assert q.dtype == np.float32
    keep = np.ones(len(q), dtype=bool)
    m = F32(margin)
    if m >= 0:
        if x > 0:
            keep &= ~(q[:, 0] < F32(x) + m)
        if x + tw < w0:
            keep &= ~(q[:, 2] > F32(x + tw) - m)
        if y > 0:
            keep &= ~(q[:, 1] < F32(y) + m)
        if y + th < h0:
            keep &= ~(q[:, 3] > F32(y + th) - m)
    hi = np.array([w0, h0, w0, h0], dtype=np.float32)
    q = np.where(q < F32(0), F32(0), np.where(q > hi, hi, q)).astype(np.float32)
    v = q / F32(max(h0, w0))
    assert v.dtype == np.float32
    return v, keep


def build_lists(F, shapes, tiles, per_tile, side, margin):
    """per_tile[t] = (boxes [K,4], scores [K], cls [K]) kept by the forward of tile t, or None for a tile whose count carried the range mark
    -> (lists [(boxes, scores, cls int64)] per frame, tile_start [T], range_mark)"""
    bb = [[] for _ in range(F)]
    sc = [[] for _ in range(F)]
    cl = [[] for _ in range(F)]
    n = [0] * F
    start = np.zeros(len(tiles), dtype=np.int64)
    mark = False
    for t, tile in enumerate(tiles):
        f = int(tile[0])
        start[t] = n[f]
        if per_tile[t] is None:
            mark = True
            continue
        b, s, c = per_tile[t]
        v, keep = remap(b, tile, shapes[f], side, margin)
        bb[f].append(v[keep]); sc[f].append(np.asarray(s, dtype=np.float32)[keep]); cl[f].append(np.asarray(c).astype(np.int64)[keep])
        n[f] += int(keep.sum())
    lists = []
    for f in range(F):
        lists.append((np.concatenate(bb[f] + [np.zeros((0, 4), np.float32)]), np.concatenate(sc[f] + [np.zeros(0, np.float32)]),
                      np.concatenate(cl[f] + [np.zeros(0, np.int64)])))
    return lists, start, mark


def merge(lst, num_classes, nms_thresh):
    """One frame's list -> kept (boxes, scores, cls) in list order: the per-class NMS the TTA tests use (oracle.tta_merge, one forward)."""
    from oracle import oracle as orc
    b, s, c = lst
    if len(s) == 0:
        return b, s, c
    kb, ks, kc, _ = orc.tta_merge([(b, s, c)], num_classes, nms_thresh)
    return kb, ks, kc
