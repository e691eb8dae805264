"""Rectangular inference: the window of the letterboxed square that a batch of frames needs (host arithmetic only, no torch).

A rectangular grid (yn_set_grid_rect) is an H x W window whose top-left pixel sits at (left, top) of the side x side square that
ValTransforms letterboxes every frame into.  Boxes stay normalised to the square, so the evaluators and the painter keep their ordinary
7-field geometry; only pad is cut off."""


def _extent(g):
    """(x0, y0, x1, y1) of a frame's resized extent: g = (w0, h0, rw, rh, left, top, side) (voc_geometry) or (rw, rh, left, top)."""
    if len(g) == 7:
        rw, rh, left, top = g[2:6]
    elif len(g) == 4:
        rw, rh, left, top = g
    else:
        raise ValueError("rect_window: a geometry row has 7 fields (w0, h0, rw, rh, left, top, side) or 4 (rw, rh, left, top), got %d" % len(g))
    return int(left), int(top), int(left) + int(rw), int(top) + int(rh)


def rect_window(geoms, side, multiple=32):
    """-> (left, top, W, H): the smallest window of the side x side square with extents that are multiples of `multiple` and that holds
    every frame's resized extent, centred on their union and shifted to lie inside the square."""
    side, multiple = int(side), int(multiple)
    ext = [_extent(g) for g in geoms]
    if not ext:
        raise ValueError("rect_window: no frames")
    x0, y0 = min(e[0] for e in ext), min(e[1] for e in ext)
    x1, y1 = max(e[2] for e in ext), max(e[3] for e in ext)
    if x0 < 0 or y0 < 0 or x1 > side or y1 > side or x1 <= x0 or y1 <= y0:
        raise ValueError("rect_window: the frames' extents [%d, %d) x [%d, %d) do not lie inside the %d square" % (x0, x1, y0, y1, side))

    def axis(lo, hi):
        n = -(-(hi - lo) // multiple) * multiple              # the extent rounded up
        if n > side:
            raise ValueError("rect_window: %d rounded up to a multiple of %d exceeds the square's %d" % (hi - lo, multiple, side))
        start = (lo + hi - n) // 2                             # centred on [lo, hi) ...
        return min(max(start, 0), side - n), n                 # ... and shifted into the square (it still holds [lo, hi): n >= hi - lo)

    left, W = axis(x0, x1)
    top, H = axis(y0, y1)
    return left, top, W, H
