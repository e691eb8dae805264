"""Detections painted onto frames on the device: test.py:50-92 / demo.py:48-71 (visualize, plot_bbox_labels) through yn_draw_*.

    vis = Visualizer(class_names, class_colors(num_classes), vis_thresh=0.3)
    vis.batch(frames, rec, offsets, geoms)          # device uint8 frames, painted in place from yn_pack_detections' output
    img = vis(img, bboxes, scores, cls_inds)        # the reference's visualize() for one host frame and pixel-space boxes

Per detection, in list order, a later one over an earlier one: the box outline, a filled title bar and '%s: %.2f' in colors[class].
The mapping to pixels (the evaluators' un-letterboxing on a float32 array), int(), the strict score threshold, the score digits and the
order are the reference's.  The raster rules and the font are this package's own: parity with cv2's rasteriser and
Hershey font is not claimed.
"""
import ctypes

import numpy as np

GLYPH_W, GLYPH_H = 6, 10                                       # the built-in font's cell: 5 x 9 glyphs, one blank column, one blank row on top

# The built-in font, authored here: 5 columns x 9 rows per glyph (cell rows 1..9; rows 1-2 ascenders, 3-7 the x-height, 8-9 descenders).
_GLYPHS = {
    "a": (".....", ".....", ".###.", "....#", ".####", "#...#", ".####", ".....", "....."),
    "b": ("#....", "#....", "####.", "#...#", "#...#", "#...#", "####.", ".....", "....."),
    "c": (".....", ".....", ".###.", "#...#", "#....", "#...#", ".###.", ".....", "....."),
    "d": ("....#", "....#", ".####", "#...#", "#...#", "#...#", ".####", ".....", "....."),
    "e": (".....", ".....", ".###.", "#...#", "#####", "#....", ".###.", ".....", "....."),
    "f": ("..##.", ".#...", "###..", ".#...", ".#...", ".#...", ".#...", ".....", "....."),
    "g": (".....", ".....", ".####", "#...#", "#...#", "#...#", ".####", "....#", ".###."),
    "h": ("#....", "#....", "####.", "#...#", "#...#", "#...#", "#...#", ".....", "....."),
    "i": ("..#..", ".....", ".##..", "..#..", "..#..", "..#..", ".###.", ".....", "....."),
    "j": ("...#.", ".....", "..##.", "...#.", "...#.", "...#.", "...#.", "#..#.", ".##.."),
    "k": ("#....", "#....", "#..#.", "#.#..", "##...", "#.#..", "#..#.", ".....", "....."),
    "l": (".##..", "..#..", "..#..", "..#..", "..#..", "..#..", ".###.", ".....", "....."),
    "m": (".....", ".....", "##.#.", "#.#.#", "#.#.#", "#.#.#", "#.#.#", ".....", "....."),
    "n": (".....", ".....", "####.", "#...#", "#...#", "#...#", "#...#", ".....", "....."),
    "o": (".....", ".....", ".###.", "#...#", "#...#", "#...#", ".###.", ".....", "....."),
    "p": (".....", ".....", "####.", "#...#", "#...#", "#...#", "####.", "#....", "#...."),
    "q": (".....", ".....", ".####", "#...#", "#...#", "#...#", ".####", "....#", "....#"),
    "r": (".....", ".....", "#.##.", "##..#", "#....", "#....", "#....", ".....", "....."),
    "s": (".....", ".....", ".####", "#....", ".###.", "....#", "####.", ".....", "....."),
    "t": (".#...", ".#...", "###..", ".#...", ".#...", ".#..#", "..##.", ".....", "....."),
    "u": (".....", ".....", "#...#", "#...#", "#...#", "#...#", ".####", ".....", "....."),
    "v": (".....", ".....", "#...#", "#...#", "#...#", ".#.#.", "..#..", ".....", "....."),
    "w": (".....", ".....", "#...#", "#.#.#", "#.#.#", "#.#.#", ".#.#.", ".....", "....."),
    "x": (".....", ".....", "#...#", ".#.#.", "..#..", ".#.#.", "#...#", ".....", "....."),
    "y": (".....", ".....", "#...#", "#...#", "#...#", "#...#", ".####", "....#", ".###."),
    "z": (".....", ".....", "#####", "...#.", "..#..", ".#...", "#####", ".....", "....."),
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###.", ".....", "....."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###.", ".....", "....."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####", ".....", "....."),
    "3": (".###.", "#...#", "....#", "..##.", "....#", "#...#", ".###.", ".....", "....."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#.", ".....", "....."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###.", ".....", "....."),
    "6": (".###.", "#....", "#....", "####.", "#...#", "#...#", ".###.", ".....", "....."),
    "7": ("#####", "....#", "...#.", "..#..", "..#..", "..#..", "..#..", ".....", "....."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###.", ".....", "....."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "....#", ".###.", ".....", "....."),
    ":": (".....", ".....", ".....", "..#..", ".....", ".....", "..#..", ".....", "....."),
    ".": (".....", ".....", ".....", ".....", ".....", ".....", "..#..", ".....", "....."),
    "-": (".....", ".....", ".....", ".....", ".###.", ".....", ".....", ".....", "....."),
}
_HOLLOW = ("#####", "#...#", "#...#", "#...#", "#...#", "#...#", "#####", ".....", ".....")       # anything the font does not know


def default_font():
    """The built-in A8 atlas, uint8 [95][GLYPH_H][GLYPH_W] for ASCII 32..126: a-z, 0-9 and ':', '.', '-' have glyphs of their own, A-Z the
    lowercase ones, the space is empty, everything else is a hollow box.  Coverage is 0 or 255."""
    atlas = np.zeros((95, GLYPH_H, GLYPH_W), dtype=np.uint8)
    for code in range(32, 127):
        ch = chr(code)
        if ch == " ":
            continue
        rows = _GLYPHS.get(ch.lower(), _HOLLOW)
        for r, row in enumerate(rows):
            for c, v in enumerate(row):
                if v == "#":
                    atlas[code - 32, 1 + r, c] = 255
    return atlas


def class_colors(num_classes, seed=0):
    """test.py:192-195: np.random.seed(seed), then three np.random.randint(255) per class (drawn from a RandomState of the same seed, which
    gives the same numbers and leaves numpy's global generator alone)."""
    rng = np.random.RandomState(seed)
    return [(rng.randint(255), rng.randint(255), rng.randint(255)) for _ in range(num_classes)]


_reference_colors = class_colors                              # Visualizer's constructor has a parameter of that name


class Visualizer:
    """One yn_draw: the reference's visualize() with the painting on the device.  `class_names` are the label strings by class index (the
    coco class_indexs indirection of test.py:79-81 is the caller's: pass the names in class-index order); a list of length 1 or less
    gives colour (255, 0, 0) and no label (test.py:87-89), for the classes 0..num_classes-1 (`num_classes`, by default the length of
    `class_colors`, else 1: pass one of them when the network has more than one class).  `font`: an A8 atlas uint8 [95][gh][gw], by default default_font()."""

    def __init__(self, class_names, class_colors=None, vis_thresh=0.3, thickness=2, font=None, handle=None, device=None, num_classes=None):
        from . import capi
        self.lib = capi.load_library()
        names = [str(n) for n in class_names]
        colors = None if class_colors is None else [tuple(int(v) for v in c) for c in class_colors]
        if len(names) > 1:
            self.num_classes = len(names)
            if num_classes is not None and int(num_classes) != self.num_classes:
                raise capi.YnError("Visualizer: %d names for num_classes = %d" % (self.num_classes, int(num_classes)))
            if colors is None:
                colors = _reference_colors(self.num_classes)
            self.labels = names
        else:
            # the reference draws every class the network predicts in (255, 0, 0) here, so the object has to know how many there are:
            # num_classes, else the length of class_colors, else 1 (a record of any other class is skipped and counted)
            self.num_classes = int(num_classes) if num_classes is not None else (len(colors) if colors else 1)
            colors = [(255, 0, 0)] * self.num_classes
            self.labels = None
        if len(colors) != self.num_classes:
            raise capi.YnError("Visualizer: %d colours for %d classes" % (len(colors), self.num_classes))
        self.colors = np.ascontiguousarray(np.asarray(colors, dtype=np.int64).reshape(self.num_classes, 3).astype(np.uint8))
        self.vis_thresh, self.thickness = float(vis_thresh), int(thickness)
        self.font = None
        if self.labels is not None:
            self.font = np.ascontiguousarray(default_font() if font is None else np.asarray(font, dtype=np.uint8))
            if self.font.ndim != 3 or self.font.shape[0] != 95:
                raise capi.YnError("Visualizer: the font is an array [95][gh][gw], got %s" % (self.font.shape,))
        self._handle, self._device = handle, device
        h = self._h()
        lab = atlas = None
        gh = gw = 0
        if self.labels is not None:
            try:
                enc = [n.encode("ascii") for n in self.labels]
            except UnicodeEncodeError:
                raise capi.YnError("Visualizer: labels must be ASCII 32..126")
            lab = (ctypes.c_char_p * self.num_classes)(*enc)
            atlas, gh, gw = self.font.ctypes.data, int(self.font.shape[1]), int(self.font.shape[2])
        d = ctypes.c_void_p()
        h._ck(self.lib.yn_draw_create(h.h, self.num_classes, self.colors.ctypes.data, ctypes.cast(lab, ctypes.c_void_p) if lab is not None else None,
                                      atlas, gw, gh, self.thickness, ctypes.byref(d)), "yn_draw_create")
        self.d = d

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
        if getattr(self, "d", None):
            self.lib.yn_draw_destroy(self.d)
            self.d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch(self, frames, rec, offsets, geoms=None, pixels=False, vis_thresh=None, handle=None):
        """Paints `frames` (a list of B contiguous uint8 [h0,w0,3] BGR device tensors) in place from rec [>= total, 6] float32 / offsets
        [B+1] int32 on the device, as yn_pack_detections / yn_tta_result wrote them.  geoms: B rows (w0, h0, rw, rh, left, top, side)
        (voc_geometry); pixels=True: the boxes are pixels already and geoms may be None.  Asynchronous; nothing is read back."""
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
        rec, offsets = h._in(rec), h._in(offsets, torch.int32)
        h._ck(self.lib.yn_draw_batch(h.h, self.d, B, ctypes.cast(ptrs, ctypes.c_void_p), geom.ctypes.data, 1 if pixels else 0, rec.data_ptr(),
                                     offsets.data_ptr(), int(rec.shape[0]), float(self.vis_thresh if vis_thresh is None else vis_thresh)), "yn_draw_batch")
        return frames

    def status(self, handle=None):
        """{'drawn', 'skipped', 'range_mark'} of the last batch (yn_draw_status; synchronises)."""
        h = self._h(handle)
        drawn, skipped, mark = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        h._ck(self.lib.yn_draw_status(h.h, self.d, ctypes.byref(drawn), ctypes.byref(skipped), ctypes.byref(mark)), "yn_draw_status")
        return {"drawn": int(drawn.value), "skipped": int(skipped.value), "range_mark": bool(mark.value)}

    def prims(self, handle=None):
        """Testing aid (yn_draw_prims): int32 [n][7] = frame, class, x1, y1, x2, y2 (unclipped), k of every drawn record, in drawing order."""
        h = self._h(handle)
        n = self.status(h)["drawn"]
        out = np.zeros((max(n, 1), 7), dtype=np.int32)
        h._ck(self.lib.yn_draw_prims(h.h, self.d, out.ctypes.data, n), "yn_draw_prims")
        return out[:n]

    def __call__(self, img, bboxes, scores, cls_inds, handle=None):
        """The reference's visualize(img, bboxes, scores, cls_inds, ...) for one host frame and boxes in its pixels -> the painted array."""
        import torch
        h = self._h(handle)
        n = len(scores)
        rows = np.zeros((max(n, 1), 6), dtype=np.float32)
        rows[:n, :4] = np.asarray(bboxes, dtype=np.float32).reshape(-1, 4)
        rows[:n, 4] = np.asarray(scores, dtype=np.float32)
        rows[:n, 5] = np.asarray(cls_inds).astype(np.float32)
        frame = torch.as_tensor(np.ascontiguousarray(img, dtype=np.uint8)).to(h.device)
        self.batch([frame], torch.from_numpy(rows).to(h.device), torch.tensor([0, n], dtype=torch.int32).to(h.device), pixels=True, handle=h)
        return frame.cpu().numpy()
