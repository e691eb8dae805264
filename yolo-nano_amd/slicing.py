"""Sliced inference: a frame larger than the network input runs as overlapping tiles at native resolution, plus the whole frame once; every
tile's boxes go back into the frame and are merged per frame with per-class NMS (yn_slice_*, kernels_slice.hip).

slice_grid / tile_table are host arithmetic only (no torch); SlicedInference needs the device.

    sl = SlicedInference(tile=416, overlap=0.2)
    model.set_grid(416)
    rec, offsets, geoms = sl.records(frames, model)     # on the device: what VOCEval.add / COCOEval.add / Visualizer.batch take
    dets = sl.batch(frames, model)                      # one (bboxes, scores, cls_inds) numpy triple per frame

Boxes are normalised by max(h0, w0) of their frame: with the identity geometry row (w0, h0, w0, h0, 0, 0, max(h0, w0)) they are what the
evaluators and the painter take, and to_pixels() gives frame pixels."""
import numpy as np


def _axis(n, tile, step):
    """Origins and the extent of the tiles along one axis of length n: the last tile is shifted back instead of being cut."""
    last = max(n - tile, 0)
    origins = list(range(0, last + 1, step))
    if origins[-1] != last:
        origins.append(last)
    return origins, min(tile, n)


def slice_grid(h0, w0, tile, overlap=0.2, full_frame=True):
    """-> the tile rectangles [(x, y, tw, th), ...] of an h0 x w0 frame in frame pixels, row-major (y outer).  Neighbouring tiles share at
    least int(tile * overlap) pixels; every tile is tile x tile unless the frame is smaller.  full_frame: the rectangle (0, 0, w0, h0) comes
    first, unless it is the only tile anyway."""
    h0, w0, tile = int(h0), int(w0), int(tile)
    if h0 < 1 or w0 < 1 or tile < 1:
        raise ValueError("slice_grid: frame %d x %d and tile %d must be positive" % (h0, w0, tile))
    step = tile - int(tile * overlap)
    if not 1 <= step <= tile:
        raise ValueError("slice_grid: overlap %r of tile %d gives the step %d, outside 1..%d" % (overlap, tile, step, tile))
    xs, tw = _axis(w0, tile, step)
    ys, th = _axis(h0, tile, step)
    rects = [(x, y, tw, th) for y in ys for x in xs]
    if full_frame and rects != [(0, 0, w0, h0)]:
        rects.insert(0, (0, 0, w0, h0))
    return rects


def _geometry(th, tw, side):
    """ValTransforms(side).geometry(th, tw)[:4] - Resize's own `int(r * size)` / `//` expressions (data/transforms.py:79-116) - without torch."""
    if th > tw:
        w = int(tw / th * side)
        return w, side, (side - w) // 2, 0
    if th < tw:
        h = int(th / tw * side)
        return side, h, 0, (side - h) // 2
    return side, side, 0, 0


def tile_table(frames_shapes, tile, overlap=0.2, full_frame=True, side=None):
    """frames_shapes: (h0, w0) per frame -> int32 [T, 9], the table the C entries take: frame, x, y, tw, th, rw, rh, left, top per tile,
    frame by frame in slice_grid's order.  (rw, rh, left, top) is the letterbox of the tile, taken as an image, into the side x side input
    (side defaults to tile)."""
    side = int(tile if side is None else side)
    rows = []
    for f, (h0, w0) in enumerate(frames_shapes):
        for x, y, tw, th in slice_grid(h0, w0, tile, overlap, full_frame):
            rows.append((f, x, y, tw, th) + _geometry(th, tw, side))
    return np.array(rows, dtype=np.int32).reshape(-1, 9)


def identity_geometry(h0, w0):
    """The geometry row under which a sliced record is frame pixels / max(h0, w0): (w0, h0, rw, rh, left, top, side) with nothing moved."""
    return (int(w0), int(h0), int(w0), int(h0), 0, 0, max(int(h0), int(w0)))


def to_pixels(bboxes, h0, w0):
    """Boxes of batch() / records() -> frame pixels (float32 [K, 4]); a fresh array."""
    return np.asarray(bboxes, dtype=np.float32).reshape(-1, 4) * np.float32(max(int(h0), int(w0)))


class SlicedInference(object):
    """tile / overlap / full_frame: slice_grid's; nms_thresh: of the per-frame merge; edge_margin (pixels, < 0 off): a tile's box that comes
    within the margin of a side where the tile was cut out of the frame is dropped - the neighbouring tile sees that object whole;
    list_capacity: rows of one frame's merge list; mean / std: ValTransforms' (BGR order); merge: "nms" (per-class NMS) or "wbf" (weighted box
    fusion, yn_wbf_merge's rule: nms_thresh is then its IoU threshold) with `expected` votes (None: 1); soft: None, or "hard" / "linear" /
    "gaussian" - the "nms" merge then suppresses by Soft-NMS with sigma and score_floor (None: the model's conf_thresh).

    Tiles run through the MODEL'S handle, `max_batch` of them per forward.  A handle is made for `chunk` (32) tiles only when the model has
    none yet: a model that already ran at batch 1 keeps that handle and slices one tile per forward - the same result (it does not depend on
    the chunking), more launches; records() warns once when that happens.  Call model.handle(n) before the model's first forward, or
    slice first, to choose."""

    def __init__(self, tile=416, overlap=0.2, full_frame=True, nms_thresh=0.5, edge_margin=-1.0, list_capacity=8192,
                 mean=(0.406, 0.456, 0.485), std=(0.225, 0.224, 0.229), merge="nms", expected=None, soft=None, sigma=0.5, score_floor=None):
        from .capi import check_soft_with_merge, merge_rule_id
        check_soft_with_merge("SlicedInference", merge, soft)
        self.soft, self.sigma, self.score_floor = soft, float(sigma), None if score_floor is None else float(score_floor)
        self.merge, self._rule = merge, merge_rule_id(merge)
        self.expected = None if expected is None else int(expected)
        self.tile, self.overlap, self.full_frame = int(tile), overlap, bool(full_frame)
        self.nms_thresh, self.edge_margin, self.list_capacity = float(nms_thresh), float(edge_margin), int(list_capacity)
        self.mean = np.array(mean, dtype=np.float32)
        self.std = np.array(std, dtype=np.float32)
        self.chunk = 32                                        # the max_batch of a handle this object has to make (tiles per forward)
        self._obj = None
        slice_grid(self.tile, self.tile, self.tile, self.overlap, self.full_frame)      # refuses a bad tile / overlap here

    def table(self, frames):
        return tile_table([(int(im.shape[0]), int(im.shape[1])) for im in frames], self.tile, self.overlap, self.full_frame, self.tile)

    def device_handle(self, model, F):
        """The model's handle (made for `chunk` tiles per forward if the model has none yet) with this object's yn_slice for at least F frames.
        model.set_grid(tile) is the caller's."""
        from . import capi
        if model.input_size != self.tile:
            raise capi.YnError("SlicedInference: the model's grid is %r, the tiles are %d x %d; call model.set_grid(%d) first"
                               % (model.input_size, self.tile, self.tile, self.tile))
        h = model.handle(self.chunk)
        if h.max_batch < self.chunk and not getattr(self, "_warned", False):
            import warnings
            self._warned = True
            warnings.warn("SlicedInference: the model's handle was made for %d images per forward, so the tiles run %d at a time instead of %d "
                          "(the same result, more launches); call model.handle(%d) before the model's first forward"
                          % (h.max_batch, h.max_batch, self.chunk, self.chunk))
        obj = self._obj
        if obj is None or obj.handle is not h or obj.max_frames < F or obj.list_capacity != self.list_capacity:
            if obj is not None:
                obj.close()
            self._obj = None
            obj = self._obj = capi.Slice(h, max_frames=max(int(F), 1), list_capacity=self.list_capacity)
        obj.merge_rule(self._rule, 0 if self.expected is None else self.expected, handle=h)
        obj.merge_soft(self.soft, self.sigma, float(model.conf_thresh) if self.score_floor is None else self.score_floor, handle=h)
        return h

    def records(self, frames, model):
        """frames: uint8 HxWx3 BGR numpy arrays or CUDA uint8 tensors of any sizes -> (rec [>= total, 6] float32, offsets [F+1] int32, geoms):
        rec / offsets ON THE DEVICE in yn_pack_detections' layout, views of the yn_slice object's buffers, valid until the next records() /
        batch(); geoms the identity rows.  On the split-f16 range mark the model's own fallback runs: acknowledge, yn_exact_f32(1), once more."""
        import torch
        h = self.device_handle(model, len(frames))
        obj = self._obj
        dev = []
        for im in frames:
            if isinstance(im, torch.Tensor):
                assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3, "frames are uint8 [h,w,3]"
                dev.append(im.to(h.device, non_blocking=True).contiguous())
            else:
                dev.append(torch.as_tensor(np.ascontiguousarray(im, dtype=np.uint8)).to(h.device, non_blocking=True))
        tiles = self.table(dev)
        model._retry_exact(h, lambda: obj.infer(dev, tiles, self.mean, self.std, self.nms_thresh, self.edge_margin, handle=h))
        rec, off = obj.result()
        return rec, off, [identity_geometry(im.shape[0], im.shape[1]) for im in dev]

    def batch(self, frames, model):
        """One (bboxes [K,4] f32 normalised by max(h0, w0), scores [K] f32, cls_inds [K] i64) numpy triple per frame: two device-to-host copies."""
        from .capi import records_to_host
        rec, offsets, _ = self.records(frames, model)
        return records_to_host(rec, offsets)
