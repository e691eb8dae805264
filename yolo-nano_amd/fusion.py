"""Weighted box fusion on the device (yn_wbf_merge, yn_fuse_*; csrc/kernels_wbf.hip).

The rule is this package's own - tests/wbf_oracle.py restates it in float32 numpy and the kernel agrees with it bit for bit.  Parity
with the ensemble_boxes package is UNPINNED: the call shapes below follow it, the numbers need not.

    boxes, scores, labels = weighted_boxes_fusion(boxes_list, scores_list, labels_list, iou_thr=0.55)
    ens = Ensemble([model_a, model_b]); rec, offsets = ens.records(x); per_image = ens.batch(x)

Soft-NMS (yn_soft_nms_merge; csrc/kernels_soft.hip) keeps the neighbours of a kept box and marks their scores down; the rule
is the package's own as well (tests/soft_nms_oracle.py), parity with third-party implementations UNPINNED.

    boxes, scores, labels = soft_nms(boxes, scores, labels, method="gaussian", sigma=0.5)
    ens = Ensemble([model_a, model_b], merge="nms", soft="linear")
"""
import numpy as np

from .capi import MERGE_WBF, YnError, check_soft_with_merge, merge_rule_id, records_to_host, soft_method_id

_handles = {}


def _bare_handle(num_classes, device):
    """A handle that only lends its stream, scratch and class count (no weights are loaded)."""
    import torch
    from . import arch
    from .capi import Handle
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(num_classes), str(dev))
    h = _handles.get(key)
    if h is None:
        if len(_handles) >= 8:
            _handles.pop(next(iter(_handles))).close()
        h = _handles[key] = Handle(32, int(num_classes), arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=1, device=dev)
    h.follow_current_stream()
    return h


def weighted_boxes_fusion(boxes_list, scores_list, labels_list, iou_thr=0.55, expected=None, weights=None, num_classes=None, device=None):
    """One image: per model (or forward) boxes [n_i, 4], scores [n_i], labels [n_i] (integers) -> (boxes [K, 4] f32, scores [K] f32,
    labels [K] i64), the clusters in ascending order of their founder's row in the concatenation.  weights: one factor per list, applied
    to the scores with one float32 multiply; expected: the expected votes, None = the number of lists; num_classes: None = the largest
    label + 1.  Runs yn_wbf_merge on the GPU (there is no CPU fallback)."""
    import torch
    if not (len(boxes_list) == len(scores_list) == len(labels_list)):
        raise ValueError("weighted_boxes_fusion: %d box lists, %d score lists, %d label lists" % (len(boxes_list), len(scores_list), len(labels_list)))
    if weights is not None and len(weights) != len(boxes_list):
        raise ValueError("weighted_boxes_fusion: %d weights for %d lists" % (len(weights), len(boxes_list)))
    bs, ss, ls = [], [], []
    for i in range(len(boxes_list)):
        b = np.asarray(boxes_list[i], np.float32).reshape(-1, 4)
        s = np.asarray(scores_list[i], np.float32).reshape(-1)
        lab = np.asarray(labels_list[i]).reshape(-1)
        if not (len(b) == len(s) == len(lab)):
            raise ValueError("weighted_boxes_fusion: list %d has %d boxes, %d scores, %d labels" % (i, len(b), len(s), len(lab)))
        if len(lab) and not np.array_equal(lab, np.floor(lab)):
            raise ValueError("weighted_boxes_fusion: list %d has a label that is not an integer" % i)
        if weights is not None:
            s = (s * np.float32(weights[i])).astype(np.float32)
        bs.append(b); ss.append(s); ls.append(lab.astype(np.int64))
    boxes = np.concatenate(bs) if bs else np.zeros((0, 4), np.float32)
    scores = np.concatenate(ss) if ss else np.zeros((0,), np.float32)
    labels = np.concatenate(ls) if ls else np.zeros((0,), np.int64)
    if len(labels) and labels.min() < 0:
        raise ValueError("weighted_boxes_fusion: negative label")
    C = int(num_classes) if num_classes is not None else (int(labels.max()) + 1 if len(labels) else 1)
    if len(labels) and labels.max() >= C:
        raise ValueError("weighted_boxes_fusion: label %d with num_classes %d" % (int(labels.max()), C))
    E = max(len(boxes_list), 1) if expected is None else int(expected)
    if len(boxes) == 0:
        return boxes, scores, labels
    h = _bare_handle(C, device)
    ob, osc, oc, _, _ = h.wbf_merge(torch.from_numpy(boxes).to(h.device), torch.from_numpy(scores).to(h.device),
                                    torch.from_numpy(labels.astype(np.int32)).to(h.device), C, iou_thr, E)
    return ob.cpu().numpy().copy(), osc.cpu().numpy().copy(), oc.cpu().numpy().astype(np.int64)


def soft_nms(boxes, scores, labels, method="gaussian", iou_thr=0.5, sigma=0.5, score_floor=0.001, num_classes=None, device=None):
    """One image: boxes [n, 4], scores [n], labels [n] (integers) -> (boxes [K, 4] f32, scores [K] f32 decayed, labels [K] i64), the kept rows
    in ascending row order.  method "hard" / "linear" / "gaussian" (DESIGN.md 31); rows whose score is or falls to score_floor or below are
    dropped.  Runs yn_soft_nms_merge on the GPU (there is no CPU fallback)."""
    import torch
    if method is None:
        raise ValueError("soft_nms: method must be 'hard', 'linear' or 'gaussian', got None")
    m = soft_method_id(method)
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    s = np.asarray(scores, np.float32).reshape(-1)
    lab = np.asarray(labels).reshape(-1)
    if not (len(b) == len(s) == len(lab)):
        raise ValueError("soft_nms: %d boxes, %d scores, %d labels" % (len(b), len(s), len(lab)))
    if len(lab) and not np.array_equal(lab, np.floor(lab)):
        raise ValueError("soft_nms: a label is not an integer")
    lab = lab.astype(np.int64)
    if len(lab) and lab.min() < 0:
        raise ValueError("soft_nms: negative label")
    C = int(num_classes) if num_classes is not None else (int(lab.max()) + 1 if len(lab) else 1)
    if len(lab) and lab.max() >= C:
        raise ValueError("soft_nms: label %d with num_classes %d" % (int(lab.max()), C))
    if len(b) == 0:
        return b, s, lab
    h = _bare_handle(C, device)
    ob, osc, oc, _ = h.soft_nms_merge(torch.from_numpy(b).to(h.device), torch.from_numpy(s).to(h.device),
                                      torch.from_numpy(lab.astype(np.int32)).to(h.device), C, m, iou_thr, sigma, score_floor)
    return ob.cpu().numpy().copy(), osc.cpu().numpy().copy(), oc.cpu().numpy().astype(np.int64)


class Ensemble(object):
    """Several YOLONano models of one class count on one batch: each model's yn_infer + yn_pack_detections is appended to the B merge
    lists of a yn_fuse and the lists are merged once (merge "wbf": weighted box fusion, "nms": per-class NMS) at iou_thr.  weights: one
    score factor per model.  soft ("hard" / "linear" / "gaussian", with merge="nms" only): the NMS merge suppresses by Soft-NMS.  records() gives the device record lists VOCEval.add / COCOEval.add / Visualizer / Tracker take."""
    list_capacity = 8192                                       # rows of one image's merge list (all models together)

    def __init__(self, models, iou_thr=0.55, merge="wbf", weights=None, expected=None, soft=None, sigma=0.5, score_floor=0.001):
        check_soft_with_merge("Ensemble", merge, soft)
        self.soft, self.sigma, self.score_floor = soft, float(sigma), float(score_floor)
        self.models = list(models)
        if not self.models:
            raise ValueError("Ensemble: no models")
        if weights is not None and len(weights) != len(self.models):
            raise ValueError("Ensemble: %d weights for %d models" % (len(weights), len(self.models)))
        self.iou_thr, self.merge, self._rule = float(iou_thr), merge, merge_rule_id(merge)
        self.weights = [1.0] * len(self.models) if weights is None else [float(w) for w in weights]
        self.expected = None if expected is None else int(expected)
        self._obj = None

    def _fuse(self, h, B):
        from . import capi
        obj = self._obj
        if obj is None or obj.handle is not h or obj.max_units < B or obj.list_capacity != int(self.list_capacity):
            if obj is not None:
                obj.close()
            self._obj = None
            obj = self._obj = capi.Fuse(h, max_units=max(int(B), 1), list_capacity=int(self.list_capacity))
        return obj

    def records(self, x):
        """x [B,3,S,S] on the models' device -> (rec [>= total, 6] float32, offsets [B+1] int32) ON THE DEVICE, in yn_pack_detections'
        layout: views of the yn_fuse object's buffers, valid until the next records() / batch()."""
        B = int(x.shape[0])
        xf = x.float()
        handles = []
        for m in self.models:
            h = m.handle(B)
            h.follow_current_stream()
            handles.append(h)
        h0 = handles[0]
        for h in handles[1:]:
            if h.C != h0.C or h.device != h0.device:
                raise YnError("Ensemble: the models have %d and %d classes on %s and %s; one class count on one device is needed"
                              % (h0.C, h.C, h0.device, h.device))
        obj = self._fuse(h0, B)
        obj.open(B)
        for m, h, w in zip(self.models, handles, self.weights):
            rec, off = m._retry_exact(h, lambda: self._packed(h, xf))
            obj.append(rec, off, w, handle=h0)
        obj.merge_soft(self.soft, self.sigma, self.score_floor, handle=h0)
        obj.merge(B, self._rule, self.iou_thr, 0 if self.expected is None else self.expected)
        return obj.result()

    @staticmethod
    def _packed(h, xf):
        from .capi import YnRangeError
        out = h.infer(xf)
        rec, off = h.pack_detections(out)
        if int(off[-1].item()) < 0:                            # the range mark: the model's own fallback takes over (_retry_exact)
            raise YnRangeError("yn_infer: an activation exceeded the split-f16 range (|x| >= 65504); results invalid, re-run under exact_f32")
        return rec, off

    def batch(self, x):
        """One (bboxes [K,4] f32, scores [K] f32, cls_inds [K] i64) numpy triple per image of x."""
        return records_to_host(*self.records(x))


__all__ = ["weighted_boxes_fusion", "soft_nms", "Ensemble", "MERGE_WBF"]
