"""COCO box AP on the device: what COCOAPIEvaluator.evaluate (evaluator/cocoapi_evaluator.py) obtains from pycocotools'
COCOeval(cocoGt, cocoDt, 'bbox') with its default parameters, through yn_coco_*.

    gts, image_ids, cat_ids = coco_gt_arrays(json.load(open('instances_val2017.json')))
    ev = COCOEval(80)                                # one evaluator, any number of batches
    ev.add(rec, offsets, geoms, ids, gts)            # yn_pack_detections output (device) + letterbox geometry + ground truth
    stats = ev.compute()                             # COCOeval.stats [12]; ev.precision [10,101,C,4,3], ev.recall [10,C,4,3]

    ap50, ap50_95 = evaluate_coco(model, images, image_ids, annotations)

computeIoU, evaluateImg and accumulate run on the device (float64 IoU as the C routine bbIou, integer counts, COCOeval's stable
orders: by score descending, equal scores in results-list order inside an image and in ascending image id between images);
summarize is numpy on the host, from the two arrays the device returns.  The parameters are numpy's own doubles, handed down.
pycocotools is not a dependency and is never imported; parity with pycocotools is unpinned wherever it cannot be installed - the
device is tested bit for bit against the host restatement tests/coco_oracle.py, and tests/golden/gen_coco_eval.py asserts that
restatement against pycocotools when it is importable.
"""
import ctypes

import numpy as np
import torch

from . import capi
from .voc import voc_geometry


def default_params():
    """pycocotools' Params.setDetParams"""
    return {"iouThrs": np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
            "recThrs": np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
            "maxDets": [1, 10, 100],
            "areaRng": [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]}


def summarize(precision, recall, params=None):
    """COCOeval.summarize for iouType 'bbox': the 12 stats from precision [T,R,K,A,M] and recall [T,K,A,M]."""
    p = params or default_params()

    def one(ap, iou_thr=None, area=0, max_det=100):
        mind = [i for i, v in enumerate(p["maxDets"]) if v == max_det]
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == p["iouThrs"])[0]]
        s = s[:, :, :, [area], mind] if ap else s[:, :, [area], mind]
        s = s[s > -1]
        return -1.0 if len(s) == 0 else float(np.mean(s))

    last = p["maxDets"][-1]
    return np.array([one(1, max_det=last), one(1, .5, max_det=last), one(1, .75, max_det=last),
                     one(1, area=1, max_det=last), one(1, area=2, max_det=last), one(1, area=3, max_det=last),
                     one(0, max_det=p["maxDets"][0]), one(0, max_det=p["maxDets"][1]), one(0, max_det=last),
                     one(0, area=1, max_det=last), one(0, area=2, max_det=last), one(0, area=3, max_det=last)], dtype=np.float64)


def coco_gt_arrays(dataset):
    """An already loaded COCO annotation dict ('images', 'annotations', 'categories') -> (gts, image_ids, cat_ids): gts[i] is the
    float64 array [G][7] = x, y, w, h, area, category index, iscrowd of image image_ids[i] in file order; image_ids follows
    dataset['images']; cat_ids[k] is the category id of index k (ascending ids, as COCO's getCatIds; the reference's class_ids)."""
    cat_ids = sorted(int(c["id"]) for c in dataset["categories"])
    index = {c: k for k, c in enumerate(cat_ids)}
    image_ids = [int(im["id"]) for im in dataset["images"]]
    rows = {i: [] for i in image_ids}
    for a in dataset["annotations"]:
        x, y, w, h = [float(v) for v in a["bbox"]]
        rows[int(a["image_id"])].append([x, y, w, h, float(a["area"]), index[int(a["category_id"])], int(a.get("iscrowd", 0))])
    gts = [np.array(rows[i], dtype=np.float64).reshape(-1, 7) for i in image_ids]
    return gts, image_ids, cat_ids


class COCOEval:
    """Device state of one COCO box evaluation (yn_coco).  Every method may take the capi.Handle to launch on (its stream); by default
    the evaluator's own bare handle on `device`."""

    def __init__(self, num_classes, params=None, device=None, handle=None):
        self.lib = capi.load_library()
        self.num_classes = int(num_classes)
        self.params = params or default_params()
        self._handle = handle
        self._device = device
        e = ctypes.c_void_p()
        h = self._h()
        h._ck(self.lib.yn_coco_create(h.h, self.num_classes, int(self.params["maxDets"][-1]), ctypes.byref(e)), "yn_coco_create")
        self.e = e
        self.precision = self.recall = self.stats = None

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
            self.lib.yn_coco_destroy(self.e)
            self.e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, handle=None):
        h = self._h(handle)
        h._ck(self.lib.yn_coco_reset(h.h, self.e), "yn_coco_reset")
        self.precision = self.recall = self.stats = None

    def size(self):
        """(detections kept, images) added so far"""
        n, m = ctypes.c_int64(), ctypes.c_int64()
        self.lib.yn_coco_size(self.e, ctypes.byref(n), ctypes.byref(m))
        return n.value, m.value

    def add(self, rec, offsets, geoms, image_ids, gts, handle=None):
        """rec [>=total, 6] float32 / offsets [B+1] int32 on the device as yn_pack_detections wrote them, geoms B rows
        (w0, h0, rw, rh, left, top, side) (voc_geometry), image_ids B ints, gts B float arrays [G_b][7] = x, y, w, h, area, category
        index, iscrowd (coco_gt_arrays; None or empty for none).  Raises capi.YnRangeError, adding nothing, when offsets[B] carries
        the split-f16 range mark."""
        h = self._h(handle)
        B = int(offsets.shape[0]) - 1
        assert rec.is_cuda and offsets.is_cuda and rec.dtype == torch.float32 and offsets.dtype == torch.int32
        geom = np.ascontiguousarray(np.asarray(geoms, dtype=np.int32).reshape(B, 7))
        ids = np.ascontiguousarray(np.asarray(image_ids, dtype=np.int64).reshape(-1))
        parts = [np.zeros((0, 7)) if g is None else np.asarray(g, dtype=np.float64).reshape(-1, 7) for g in gts]
        assert len(parts) == B and len(ids) == B, "one ground-truth array and one image id per image"
        gt = np.concatenate(parts) if parts else np.zeros((0, 7))
        box = np.ascontiguousarray(gt[:, :5])
        meta = np.ascontiguousarray(gt[:, 5:7].astype(np.int32))
        if len(gt) and not np.array_equal(meta, gt[:, 5:7]):
            raise ValueError("COCOEval.add: category index and iscrowd must be integers")
        gt_off = np.zeros(B + 1, dtype=np.int32)
        gt_off[1:] = np.cumsum([len(p) for p in parts])
        rec, offsets = h._in(rec), h._in(offsets, torch.int32)
        h._ck(self.lib.yn_coco_add(h.h, self.e, B, rec.data_ptr(), offsets.data_ptr(), geom.ctypes.data, ids.ctypes.data,
                                   box.ctypes.data if len(gt) else None, meta.ctypes.data if len(gt) else None, gt_off.ctypes.data),
              "yn_coco_add")
        self.precision = self.recall = self.stats = None

    def add_host(self, dets, geoms, image_ids, gts, handle=None):
        """`dets`: B (bboxes [K,4] float32 in the letterboxed square's [0,1] frame, scores [K] float32, cls_inds [K]) triples, as
        YOLONano.forward / forward_batch return them; uploaded as one record list, then add()."""
        h = self._h(handle)
        off = np.zeros(len(dets) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(d[1]) for d in dets])
        rows = np.zeros((max(int(off[-1]), 1), 6), dtype=np.float32)
        for b, (bb, sc, cl) in enumerate(dets):
            r = rows[off[b]:off[b + 1]]
            r[:, :4] = np.asarray(bb, dtype=np.float32).reshape(-1, 4)
            r[:, 4] = np.asarray(sc, dtype=np.float32)
            r[:, 5] = np.asarray(cl).astype(np.float32)
        self.add(torch.from_numpy(rows).to(h.device), torch.from_numpy(off).to(h.device), geoms, image_ids, gts, handle=h)

    def _param_arrays(self):
        p = self.params
        return (np.ascontiguousarray(p["iouThrs"], dtype=np.float64), np.ascontiguousarray(p["recThrs"], dtype=np.float64),
                np.ascontiguousarray(np.asarray(p["areaRng"], dtype=np.float64).reshape(-1, 2)),
                np.ascontiguousarray(p["maxDets"], dtype=np.int32))

    def compute(self, handle=None):
        """-> stats float64 [12] (COCOeval.stats); also sets .precision [T,R,C,A,M] and .recall [T,C,A,M]."""
        h = self._h(handle)
        iou, rec, area, md = self._param_arrays()
        C = self.num_classes
        precision = np.zeros((len(iou), len(rec), C, len(area), len(md)), dtype=np.float64)
        recall = np.zeros((len(iou), C, len(area), len(md)), dtype=np.float64)
        h._ck(self.lib.yn_coco_finish(h.h, self.e, iou.ctypes.data, len(iou), rec.ctypes.data, len(rec), area.ctypes.data, len(area),
                                      md.ctypes.data, len(md), precision.ctypes.data, recall.ctypes.data), "yn_coco_finish")
        self.precision, self.recall = precision, recall
        self.stats = summarize(precision, recall, self.params)
        return self.stats

    def matches(self, handle=None):
        """Testing aid, after compute(): (det float32 [n][5] = x1, y1, x2, y2, score; seg int64 [images * C + 1]; matched bool
        [A][T][n]; ignored bool [A][T][n]).  det[seg[i * C + k]:seg[i * C + k + 1]] are the detections kept for image i (add order)
        and category k, in rank order."""
        assert self.precision is not None, "compute() first"
        h = self._h(handle)
        n, n_img = self.size()
        A, T = len(self.params["areaRng"]), len(self.params["iouThrs"])
        det = np.zeros((n, 5), dtype=np.float32)
        seg = np.zeros(n_img * self.num_classes + 1, dtype=np.int64)
        flags = np.zeros((A, n), dtype=np.uint32)
        h._ck(self.lib.yn_coco_matches(h.h, self.e, det.ctypes.data, seg.ctypes.data, flags.ctypes.data, A), "yn_coco_matches")
        t = np.arange(T, dtype=np.uint32).reshape(1, T, 1)
        matched = ((flags[:, None, :] >> t) & 1).astype(bool)
        ignored = ((flags[:, None, :] >> (t + np.uint32(16))) & 1).astype(bool)
        return det, seg, matched, ignored


def evaluate_coco(model, images, image_ids, annotations, batch=32, test_aug=None, rect=False, sliced=None):
    """COCOAPIEvaluator.evaluate for `model` (an eval-mode yolo_nano_amd.YOLONano): `images` are decoded uint8 HxWx3 BGR arrays,
    `image_ids` their COCO ids, `annotations` one float array [G][7] per image (coco_gt_arrays).  Per batch: ValTransforms.batch ->
    yn_infer -> yn_pack_detections -> yn_coco_add; nothing comes back to the host but two 4-byte counts per batch.
    -> (ap50, ap50_95) as the reference returns them; (0, 0) without any detection (cocoapi_evaluator.py:131-132).
    test_aug: a yolo_nano_amd.TestTimeAugmentation - every batch goes through its records() (yn_tta_infer) instead of the single
    forward.
    rect=True: rectangular inference, as voc.evaluate - each batch on its own window of the letterboxed square.
    sliced: a yolo_nano_amd.SlicedInference, as voc.evaluate - every batch of frames goes through its records() (yn_slice_infer)."""
    from .voc import _run_batches
    ev = None                                                   # made on the first chunk, on the handle its route has settled on

    def consume(h, rec, off, geoms, lo, hi):
        nonlocal ev
        if ev is None:
            ev = COCOEval(model.num_classes, handle=h)
        ev.add(rec, off, geoms, image_ids[lo:hi], annotations[lo:hi], handle=h)

    _run_batches("evaluate_coco", model, images, batch, test_aug, rect, sliced, consume)
    if ev is None:
        raise ValueError("evaluate_coco: no images")
    if ev.size()[0] == 0:
        ev.close()
        return 0, 0
    stats = ev.compute(handle=model.handle(1))
    ev.close()
    return stats[1], stats[0]
