"""VOC mAP on the device: VOCAPIEvaluator.evaluate + do_python_eval (evaluator/vocapi_evaluator.py) through yn_eval_*.

    ev = VOCEval(num_classes)                       # one evaluator, any number of batches
    ev.add(rec, offsets, geoms, gts)                # yn_pack_detections output (device) + letterbox geometry + VOC ground truth
    aps, mAP = ev.compute(use_07_metric=True)       # per-class AP (-1: no detections), np.mean(aps)

    aps, mAP = evaluate(model, images, annotations) # ValTransforms.batch -> yn_infer -> yn_pack_detections -> yn_eval_add

The numbers are the reference's bit for bit (score written with 3 decimals and box + 1 with 1 decimal, then parsed back; float64
IoU, integer counts, 11-point or area AP with numpy's summation order).  Among EQUAL 3-decimal scores of one class the detections
are taken in file order (image in add order, then position in the image's list), where the reference's unstable np.argsort
depends on the numpy build.  Ground truth is the VOC XML's integers: one int array [G][6] = x1, y1, x2, y2, class, difficult per
image (parse_rec + gt_array).
"""
import ctypes
import xml.etree.ElementTree as ET

import numpy as np
import torch

from . import capi


def voc_geometry(h0, w0, size):
    """(w0, h0, rw, rh, left, top, side) of ValTransforms(size) for an h0 x w0 image: the row yn_eval_add takes per image."""
    from .model import ValTransforms
    rw, rh, left, top = ValTransforms(size).geometry(h0, w0)[:4]
    return (int(w0), int(h0), int(rw), int(rh), int(left), int(top), int(size))


def parse_rec(filename):
    """evaluator/vocapi_evaluator.py:100-117: the objects of one PASCAL VOC annotation file."""
    tree = ET.parse(filename)
    objects = []
    for obj in tree.findall('object'):
        bbox = obj.find('bndbox')
        objects.append({'name': obj.find('name').text,
                        'pose': obj.find('pose').text,
                        'truncated': int(obj.find('truncated').text),
                        'difficult': int(obj.find('difficult').text),
                        'bbox': [int(bbox.find('xmin').text), int(bbox.find('ymin').text),
                                 int(bbox.find('xmax').text), int(bbox.find('ymax').text)]})
    return objects


def gt_array(objects, class_names):
    """parse_rec objects -> int32 [G][6] = x1, y1, x2, y2, class index in class_names, difficult (objects of other names are dropped,
    as voc_eval only looks at its own class)."""
    index = {n: i for i, n in enumerate(class_names)}
    rows = [o['bbox'] + [index[o['name']], int(o['difficult'])] for o in objects if o['name'] in index]
    return np.array(rows, dtype=np.int32).reshape(-1, 6)


class VOCEval:
    """Device state of one VOC evaluation (yn_eval).  Every method may take the capi.Handle to launch on (its stream); by default the
    evaluator's own bare handle on `device`."""

    def __init__(self, num_classes, ovthresh=0.5, device=None, handle=None):
        self.lib = capi.load_library()
        self.num_classes = int(num_classes)
        self.ovthresh = float(ovthresh)
        self._handle = handle
        self._device = device
        e = ctypes.c_void_p()
        h = self._h()
        h._ck(self.lib.yn_eval_create(h.h, self.num_classes, self.ovthresh, ctypes.byref(e)), "yn_eval_create")
        self.e = e
        self.npos = self.ndet = None

    def _h(self, handle=None):
        if handle is not None:
            return handle
        if self._handle is None:                               # a bare handle: only its stream / error plumbing is used
            from . import arch
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._handle = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=dev)
        return self._handle

    def close(self):
        if getattr(self, "e", None):
            self.lib.yn_eval_destroy(self.e)
            self.e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, handle=None):
        h = self._h(handle)
        h._ck(self.lib.yn_eval_reset(h.h, self.e), "yn_eval_reset")
        self.npos = self.ndet = None

    def size(self):
        """(records, images) added so far"""
        n, m = ctypes.c_int64(), ctypes.c_int64()
        self.lib.yn_eval_size(self.e, ctypes.byref(n), ctypes.byref(m))
        return n.value, m.value

    def add(self, rec, offsets, geoms, gts, handle=None):
        """rec [>=total, 6] float32 / offsets [B+1] int32 on the device as yn_pack_detections wrote them, geoms B rows
        (w0, h0, rw, rh, left, top, side) (voc_geometry), gts B int arrays [G_b][6] (gt_array; None or empty for none).
        Raises capi.YnRangeError, adding nothing, when offsets[B] carries the split-f16 range mark."""
        h = self._h(handle)
        B = int(offsets.shape[0]) - 1
        assert rec.is_cuda and offsets.is_cuda and rec.dtype == torch.float32 and offsets.dtype == torch.int32
        geom = np.ascontiguousarray(np.asarray(geoms, dtype=np.int32).reshape(B, 7))
        parts = [np.zeros((0, 6), np.int32) if g is None else np.asarray(g, dtype=np.int32).reshape(-1, 6) for g in gts]
        assert len(parts) == B, "one ground-truth array per image"
        gt = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 6), np.int32))
        gt_off = np.zeros(B + 1, dtype=np.int32)
        gt_off[1:] = np.cumsum([len(p) for p in parts])
        rec, offsets = h._in(rec), h._in(offsets, torch.int32)
        h._ck(self.lib.yn_eval_add(h.h, self.e, B, rec.data_ptr(), offsets.data_ptr(), geom.ctypes.data,
                                   gt.ctypes.data if len(gt) else None, gt_off.ctypes.data), "yn_eval_add")
        self.npos = self.ndet = None

    def add_host(self, dets, geoms, gts, handle=None):
        """`dets`: B (bboxes [K,4] float32 in the letterboxed square's [0,1] frame, scores [K] float32, cls_inds [K]) triples, as
        YOLONano.forward / forward_batch return them; uploaded as one record list, then add()."""
        h = self._h(handle)
        counts = [len(d[1]) for d in dets]
        off = np.zeros(len(dets) + 1, dtype=np.int32)
        off[1:] = np.cumsum(counts)
        rows = np.zeros((max(int(off[-1]), 1), 6), dtype=np.float32)
        for b, (bb, sc, cl) in enumerate(dets):
            r = rows[off[b]:off[b + 1]]
            r[:, :4] = np.asarray(bb, dtype=np.float32).reshape(-1, 4)
            r[:, 4] = np.asarray(sc, dtype=np.float32)
            r[:, 5] = np.asarray(cl).astype(np.float32)
        self.add(torch.from_numpy(rows).to(h.device), torch.from_numpy(off).to(h.device), geoms, gts, handle=h)

    def compute(self, use_07_metric=True, handle=None):
        """-> (aps float64 [C], mAP = np.mean(aps)); also sets .npos and .ndet (int64 [C])."""
        h = self._h(handle)
        C = self.num_classes
        ap = np.zeros(C, dtype=np.float64)
        npos = np.zeros(C, dtype=np.int64)
        ndet = np.zeros(C, dtype=np.int64)
        h._ck(self.lib.yn_eval_finish(h.h, self.e, int(bool(use_07_metric)), ap.ctypes.data, npos.ctypes.data, ndet.ctypes.data),
              "yn_eval_finish")
        self.npos, self.ndet = npos, ndet
        return ap, np.mean(ap)

    def curve(self, cls, handle=None):
        """voc_eval's (rec, prec) float64 arrays of class `cls` after compute(); (-1., -1.) without detections, as the reference."""
        assert self.ndet is not None, "compute() first"
        h = self._h(handle)
        nd = int(self.ndet[cls])
        if nd == 0:
            return -1., -1.
        rec = np.empty(nd, dtype=np.float64)
        prec = np.empty(nd, dtype=np.float64)
        h._ck(self.lib.yn_eval_curve(h.h, self.e, int(cls), rec.ctypes.data, prec.ctypes.data, nd), "yn_eval_curve")
        return rec, prec

    def records(self, handle=None):
        """int32 [n][7] = image, class, score bin k, x1, y1, x2, y2 in tenths: what the text-file route keeps of each detection."""
        h = self._h(handle)
        n = self.size()[0]
        out = np.zeros((n, 7), dtype=np.int32)
        if n:
            h._ck(self.lib.yn_eval_records(h.h, self.e, out.ctypes.data, n), "yn_eval_records")
        return out


def _rect_batch(model, tf, chunk):
    """One batch of rectangular inference: the frames' window of the letterboxed square (ValTransforms.batch(rect=True)), the model's grid
    set to it - only when it differs from the one it holds - -> (x [B,3,H,W], geoms).  The records keep the square's normalisation."""
    x, geoms, (left, top, W, H) = tf.batch(chunk, rect=True)
    if model._grid_target() != (H, W, tf.size, left, top):
        model.set_grid((H, W))
        model.set_window(tf.size, left, top)
    return x, geoms


def _run_batches(who, model, images, batch, test_aug, rect, sliced, consume):
    """The batch loop of evaluate / evaluate_coco (`who` names the caller in messages): per chunk of `batch` images one of the four routes - plain
    (ValTransforms.batch -> yn_infer -> yn_pack_detections), rect (_rect_batch, the model's square grid back afterwards), test_aug (its records())
    or sliced (its records()) - then consume(h, rec, offsets, geoms, lo, hi) with the chunk's records on the device and its slice lo:hi of the
    per-image arguments.  The split-f16 range mark: on the plain and rect routes the pack AND consume run inside the model's retry (an evaluator's
    add() refuses a marked batch with nothing added, so running again is safe); the other two routes retry inside their records()."""
    from .model import ValTransforms
    if rect and test_aug is not None:
        raise ValueError("%s: test-time augmentation runs on square grids; rect=True and test_aug exclude each other" % who)
    if sliced is not None and (rect or test_aug is not None):
        raise ValueError("%s: sliced inference runs its own tiles on square grids; sliced and %s exclude each other" % (who, "rect=True" if rect else "test_aug"))
    size = int(model.input_size)
    try:
        for lo in range(0, len(images), batch):
            chunk, hi = images[lo:lo + batch], lo + batch
            if sliced is not None:
                h = sliced.device_handle(model, len(chunk))
                rec, off, geoms = sliced.records(chunk, model)      # (boxes in the frame, identity geometry)
                consume(h, rec, off, geoms, lo, hi)
                continue
            h = model.handle(len(chunk)) if test_aug is None else test_aug.device_handle(model, len(chunk))
            tf = ValTransforms(size, handle=h)
            if rect:
                x, geoms = _rect_batch(model, tf, chunk)
                h = model.handle(len(chunk))
            else:
                x = tf.batch(chunk)[0]
                geoms = [voc_geometry(im.shape[0], im.shape[1], size) for im in chunk]
            if test_aug is not None:
                consume(h, *test_aug.records(x, model), geoms, lo, hi)
            else:
                model._infer_guarded(h, x, lambda out: consume(h, *h.pack_detections(out), geoms, lo, hi))
    finally:
        if rect:
            model.set_grid(size)


def evaluate(model, images, annotations, batch=32, use_07_metric=True, ovthresh=0.5, test_aug=None, rect=False, sliced=None):
    """VOCAPIEvaluator.evaluate + do_python_eval for `model` (an eval-mode yolo_nano_amd.YOLONano): `images` are decoded uint8 HxWx3
    BGR arrays, `annotations` one int array [G][6] per image (gt_array).  Per batch: ValTransforms.batch -> yn_infer ->
    yn_pack_detections -> yn_eval_add; nothing comes back to the host but each batch's 4-byte record count.  -> (aps, mAP).
    test_aug: a yolo_nano_amd.TestTimeAugmentation - every batch goes through its records() (yn_tta_infer: all scales x flip, merged
    per image on the device) instead of the single forward: the mAP eval.py's -tta flag promises (eval.py:132 builds the object,
    the evaluator never calls it).
    rect=True: rectangular inference - each batch runs on its own window of the letterboxed square (rect_window: the smallest one that
    holds every frame's picture), the grid is set only when the window changes, and the model's square grid is back afterwards.
    sliced: a yolo_nano_amd.SlicedInference - every batch of frames goes through its records() (yn_slice_infer: overlapping tiles at native
    resolution plus the whole frame, merged per frame on the device); the model's grid must be the tile (model.set_grid(tile))."""
    ev = None                                                   # made on the first chunk, on the handle its route has settled on

    def consume(h, rec, off, geoms, lo, hi):
        nonlocal ev
        if ev is None:
            ev = VOCEval(model.num_classes, ovthresh, handle=h)
        ev.add(rec, off, geoms, annotations[lo:hi], handle=h)

    _run_batches("evaluate", model, images, batch, test_aug, rect, sliced, consume)
    if ev is None:
        raise ValueError("evaluate: no images")
    aps, mAP = ev.compute(use_07_metric, handle=model.handle(1))
    ev.close()
    return aps, mAP
