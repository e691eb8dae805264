"""Detections cut out of device frames as fixed-size chips (yn_chip_*, csrc/kernels_chip.hip).

    cut = ChipExtractor(size=(128, 256), fit="stretch", out="u8", margin=0.1)
    chips, index, chip_offsets, rects = cut.batch(frames, rec, offsets, geoms)     # device tensors of capacity max_chips, asynchronous
    n = cut.count()                                                                # one int read back; chips[:n] are valid

`frames`, `rec`, `offsets`, `geoms` and `pixels` are Visualizer.batch's: B contiguous uint8 [h0,w0,3] BGR device frames and the device
record pair of yn_pack_detections, yn_tta_result, yn_slice_result, yn_fuse_result or Tracker.update.  Slot k holds the chip of record
index[k] (so ids[index[:n]], rec[index[:n]] are one gather each), rects[k] = source x, y, sw, sh and the fitted rw, rh, left, top, and
chip_offsets[b] .. chip_offsets[b+1] are the slots of frame b.  out="u8": uint8 [max_chips, ch, cw, 3] BGR (what JPEGEncoder.batch
takes); out="f32": float32 [max_chips, 3, ch, cw] RGB, normalised with mean / std (what a network takes); a square letterbox f32 chip is,
bit for bit, ValTransforms of the cropped image.  The resize is ValTransforms' (cv2's 8-bit INTER_LINEAR); the selection, margin and
fit rules are this package's own and tests/chip_oracle.py pins them.
"""
import ctypes
import math

import numpy as np

FITS = {"letterbox": 0, "stretch": 1}
FORMATS = {"u8": 0, "f32": 1}
COUNTERS = ("chips", "skipped", "overflow", "range_mark")
INT_PARAMS = ("cw", "ch", "fit", "format", "margin_px", "margin_permille", "min_side")
INT_LIMITS = ((8, 1024), (8, 1024), (0, 1), (0, 1), (0, 4096), (0, 4000), (1, 16384))
DEFAULT_MEAN, DEFAULT_STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)      # ValTransforms' defaults, BGR order


class ChipParams(ctypes.Structure):
    """yn_chip_params"""
    _fields_ = [(k, ctypes.c_int32) for k in INT_PARAMS] + [("min_score", ctypes.c_float), ("fill", ctypes.c_float * 3),
                                                             ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


def make_params(size=(128, 128), fit="letterbox", out="u8", margin=0.0, margin_px=0, min_score=0.3, min_side=2, mean=DEFAULT_MEAN,
                std=DEFAULT_STD, fill=None):
    """The constructor's arguments as the int32 / float32 values the library will see.  fit / out may be the names or the numbers."""
    fmt = FORMATS.get(out, out)
    mean32, std32 = np.asarray(mean, dtype=np.float32).reshape(3), np.asarray(std, dtype=np.float32).reshape(3)
    if fill is None:
        fill32 = mean32 * np.float32(255) if fmt == 1 else np.zeros(3, np.float32)      # Resize.mean: float32 products
    else:
        fill32 = np.asarray(fill, dtype=np.float32).reshape(3)
    return {"cw": int(size[0]), "ch": int(size[1]), "fit": int(FITS.get(fit, fit)), "format": int(fmt), "margin_px": int(margin_px),
            "margin_permille": int(round(float(margin) * 1000)), "min_side": int(min_side), "min_score": np.float32(min_score),
            "fill": fill32, "mean": mean32, "std": std32}


def refusal(num_classes, max_chips, p):
    """The reason yn_chip_create refuses these arguments with, or None: the same checks in the same order, so that a bad configuration is
    reported without a device.  `p`: make_params()'s dictionary."""
    if not 1 <= num_classes <= 2000:
        return "yn_chip_create: num_classes %d outside 1..2000" % num_classes
    if not 1 <= max_chips <= 65536:
        return "yn_chip_create: max_chips %d outside 1..65536" % max_chips
    for k, (lo, hi) in zip(INT_PARAMS, INT_LIMITS):
        if not lo <= p[k] <= hi:
            return "yn_chip_create: %s %d outside %d..%d" % (k, p[k], lo, hi)
    if p["cw"] % 4:
        return "yn_chip_create: cw %d is no multiple of 4" % p["cw"]
    floats = [("min_score", p["min_score"])] + [("%s[%d]" % (k, i), p[k][i]) for k in ("fill", "mean", "std") for i in range(3)]
    for name, v in floats:
        if not math.isfinite(float(v)):
            return "yn_chip_create: %s is not finite" % name
    for name, v in floats[7:]:
        if not float(v) > 0.0:
            return "yn_chip_create: %s is not positive" % name
    if p["format"] == 0:
        for name, v in floats[1:4]:
            if not (0.0 <= float(v) <= 255.0 and float(v) == math.floor(float(v))):
                return "yn_chip_create: %s is no integer in 0..255 (u8 chips)" % name
    return None


def unchip_boxes(boxes, rect_row, cw, ch):
    """Boxes a second stage found in a chip, normalised to the chip (x / cw, y / ch in 0..1), -> pixels of the frame the chip was cut
    from, through the slot's `rects` row (source x, y, sw, sh, rw, rh, left, top).  Host numpy, float64; [n, 4] -> [n, 4]."""
    x, y, sw, sh, rw, rh, left, top = (float(v) for v in np.asarray(rect_row).reshape(8))
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    out = np.empty_like(b)
    out[:, 0::2] = (b[:, 0::2] * float(cw) - left) * (sw / rw) + x
    out[:, 1::2] = (b[:, 1::2] * float(ch) - top) * (sh / rh) + y
    return out


class ChipExtractor:
    """One yn_chip.  size=(cw, ch): 8..1024, cw a multiple of 4; fit "letterbox" (aspect kept, the rest `fill`) or "stretch"; out "u8" or
    "f32"; margin: a fraction of the box's width / height added on every side, margin_px: pixels on top of that; records with score >
    min_score (strict) of the classes in `classes` (None: all) whose clipped rectangle has both sides >= min_side are cut, the first
    max_chips of them in record order.  fill (BGR): None gives float32(mean) * 255 for f32 (ValTransforms' pad) and 0 for u8."""

    def __init__(self, size=(128, 128), fit="letterbox", out="u8", margin=0.0, margin_px=0, min_score=0.3, min_side=2, classes=None,
                 max_chips=1024, num_classes=20, mean=DEFAULT_MEAN, std=DEFAULT_STD, fill=None, handle=None, device=None):
        from . import capi
        if fit not in FITS or out not in FORMATS:
            raise capi.YnError("ChipExtractor: fit is 'letterbox' or 'stretch' and out is 'u8' or 'f32', got %r and %r" % (fit, out))
        self.params = make_params(size, fit, out, margin, margin_px, min_score, min_side, mean, std, fill)
        self.num_classes, self.max_chips = int(num_classes), int(max_chips)
        why = refusal(self.num_classes, self.max_chips, self.params)
        if why:
            raise capi.YnError(why)
        self.cw, self.ch, self.out = self.params["cw"], self.params["ch"], out
        self.keep = None
        if classes is not None:
            self.keep = np.zeros(self.num_classes, dtype=np.uint8)
            for c in classes:
                if not 0 <= int(c) < self.num_classes:
                    raise capi.YnError("ChipExtractor: class %d outside 0..%d" % (int(c), self.num_classes - 1))
                self.keep[int(c)] = 1
        self.lib = capi.load_library()
        self._handle, self._device = handle, device
        h = self._h()
        cp = ChipParams(**{k: self.params[k] for k in INT_PARAMS})
        cp.min_score = float(self.params["min_score"])
        for k in ("fill", "mean", "std"):
            for i in range(3):
                getattr(cp, k)[i] = float(self.params[k][i])
        c = ctypes.c_void_p()
        h._ck(self.lib.yn_chip_create(h.h, self.num_classes, self.keep.ctypes.data if self.keep is not None else None, self.max_chips,
                                      ctypes.addressof(cp), ctypes.byref(c)), "yn_chip_create")
        self.c = c
        self._out = None
        self._last = None

    def _h(self, handle=None):
        if handle is not None:
            return handle
        if self._handle is None:                               # a bare handle: only its stream / error plumbing is used
            import torch
            from . import arch, capi
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._handle = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=dev)
        return self._handle

    def close(self):
        if getattr(self, "c", None):
            self.lib.yn_chip_destroy(self.c)
            self.c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def buffers(self, device):
        """Fresh output tensors (chips, index, chip_offsets [1025], rects) of the object's capacity on `device`."""
        import torch
        if self.out == "u8":
            chips = torch.empty((self.max_chips, self.ch, self.cw, 3), dtype=torch.uint8, device=device)
        else:
            chips = torch.empty((self.max_chips, 3, self.ch, self.cw), dtype=torch.float32, device=device)
        return (chips, torch.empty((self.max_chips,), dtype=torch.int32, device=device), torch.zeros((1025,), dtype=torch.int32, device=device),
                torch.empty((self.max_chips, 8), dtype=torch.int32, device=device))

    def batch(self, frames, rec, offsets, geoms=None, pixels=False, out=None, handle=None):
        """Cuts the chips of `frames` (a list of B contiguous uint8 [h0,w0,3] BGR device tensors) from rec [>= total, 6] float32 / offsets
        [B+1] int32 on the device.  geoms: B rows (w0, h0, rw, rh, left, top, side) (voc_geometry); pixels=True: the boxes are pixels
        already and geoms may be None.  -> (chips, index, chip_offsets [B+1], rects): the object's own device tensors, valid until its next
        batch, or `out` = four caller-owned tensors of those shapes.  Slots at or past chip_offsets[B] keep what they held.  chip_offsets[B]
        < 0: the input carried the range mark.  Asynchronous; nothing is read back."""
        import torch
        h = self._h(handle)
        B = len(frames)
        assert rec.is_cuda and offsets.is_cuda and rec.dtype == torch.float32 and offsets.dtype == torch.int32
        assert rec.dim() == 2 and rec.shape[1] == 6 and int(offsets.shape[0]) == B + 1, (tuple(rec.shape), tuple(offsets.shape), B)
        geom = np.zeros((max(B, 1), 7), dtype=np.int32)
        if geoms is not None:
            geom[:B] = np.asarray(geoms, dtype=np.int32).reshape(B, 7)
        else:
            assert pixels, "letterbox mode needs the geometry rows"
        ptrs = (ctypes.c_void_p * max(B, 1))()
        for b, f in enumerate(frames):
            assert f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 3 and f.is_contiguous(), "frame %d" % b
            if geoms is None:
                geom[b, 0], geom[b, 1] = int(f.shape[1]), int(f.shape[0])
            assert (int(geom[b, 0]), int(geom[b, 1])) == (int(f.shape[1]), int(f.shape[0])), "geometry row %d does not describe frame %d" % (b, b)
            ptrs[b] = f.data_ptr()
        if out is None:
            if self._out is None:
                self._out = self.buffers(h.device)
            out = self._out
        chips, index, off, rects = out
        plane = self.max_chips * self.ch * self.cw * 3
        assert chips.is_cuda and chips.is_contiguous() and chips.dtype == (torch.uint8 if self.out == "u8" else torch.float32) and chips.numel() >= plane
        assert index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.numel() >= self.max_chips
        assert rects.is_cuda and rects.dtype == torch.int32 and rects.is_contiguous() and rects.numel() >= self.max_chips * 8
        assert off.is_cuda and off.dtype == torch.int32 and off.is_contiguous() and off.numel() >= B + 1
        rec, offsets = h._in(rec), h._in(offsets, torch.int32)
        h._ck(self.lib.yn_chip_batch(h.h, self.c, B, ctypes.cast(ptrs, ctypes.c_void_p), geom.ctypes.data, 1 if pixels else 0, rec.data_ptr(),
                                     offsets.data_ptr(), int(rec.shape[0]), chips.data_ptr(), index.data_ptr(), rects.data_ptr(), off.data_ptr()),
              "yn_chip_batch")
        self._last = (off, B, h)
        return chips, index, off[:B + 1], rects

    def count(self):
        """The number of chips of the last batch (one int32 read back; synchronises); -1: the range mark."""
        assert self._last is not None, "no batch has run"
        off, B, h = self._last
        h._torch_stream().synchronize()                # the batch ran on the handle's stream, which need not be torch's current one
        return int(off[B].item())

    def status(self, handle=None):
        """{'chips', 'skipped', 'overflow', 'range_mark'} of the last batch (yn_chip_status; synchronises)."""
        h = self._h(handle)
        c = np.zeros(4, dtype=np.int64)
        h._ck(self.lib.yn_chip_status(h.h, self.c, c.ctypes.data), "yn_chip_status")
        out = dict(zip(COUNTERS, (int(v) for v in c)))
        out["range_mark"] = bool(out["range_mark"])
        return out
