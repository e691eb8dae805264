"""Detections tracked across video frames on the device (yn_track_*, csrc/kernels_track.hip).

    tracker = Tracker(streams=32)                               # one slot table and one id counter per camera stream
    rec_out, ids, offsets_out = tracker.update(rec, offsets)    # frame b of the batch belongs to stream b

`rec` / `offsets` are the device pair of yn_pack_detections, yn_tta_result or yn_slice_result; `rec_out` / `offsets_out` have the same
layout (x1, y1, x2, y2, score, class per confirmed track seen in this step) and go as they are into Visualizer.batch, evaluate and
JPEGEncoder; `ids` is the parallel int32 array of identities.  All three are device tensors owned by the tracker and valid until its next
update.  Nothing is read back and nothing synchronises in update().  The reference has no tracker: the rules are this package's own, of
the ByteTrack / BoT-SORT family with a greedy assignment, and tests/track_oracle.py pins them bit for bit.
"""
import ctypes
import math

import numpy as np

DEFAULTS = dict(track_high=0.5, track_low=0.1, new_thresh=0.6, iou_high=0.2, iou_low=0.5, iou_new=0.3, w_pos=1.0 / 20.0, w_vel=1.0 / 160.0,
                max_lost=30, min_hits=2, class_aware=1)
FLOAT_PARAMS = ("track_high", "track_low", "new_thresh", "iou_high", "iou_low", "iou_new", "w_pos", "w_vel")
INT_PARAMS = ("max_lost", "min_hits", "class_aware")
COUNTERS = ("steps", "births", "dropped_births", "overflow", "ignored", "range_marks")
MAX_STREAMS, MAX_SLOTS = 4096, 128


class TrackParams(ctypes.Structure):
    """yn_track_params"""
    _fields_ = [(k, ctypes.c_float) for k in FLOAT_PARAMS] + [(k, ctypes.c_int32) for k in INT_PARAMS]


def make_params(**kw):
    """The defaults overridden by `kw`, as the float32 / int32 values the library will see."""
    unknown = sorted(set(kw) - set(DEFAULTS))
    if unknown:
        raise TypeError("Tracker: unknown parameter %s" % ", ".join(unknown))
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: (np.float32(p[k]) if k in FLOAT_PARAMS else int(p[k])) for k in DEFAULTS}


def refusal(streams, max_tracks, max_dets, p):
    """The reason yn_track_create refuses these arguments with, or None: the same checks in the same order, so that a bad configuration
    is reported without a device."""
    if not 1 <= streams <= MAX_STREAMS:
        return "yn_track_create: streams %d outside 1..%d" % (streams, MAX_STREAMS)
    if not 1 <= max_tracks <= MAX_SLOTS:
        return "yn_track_create: max_tracks %d outside 1..%d" % (max_tracks, MAX_SLOTS)
    if not 1 <= max_dets <= MAX_SLOTS:
        return "yn_track_create: max_dets %d outside 1..%d" % (max_dets, MAX_SLOTS)
    for k in FLOAT_PARAMS:
        if not math.isfinite(float(p[k])):
            return "yn_track_create: %s is not finite" % k
    if p["track_low"] > p["track_high"]:
        return "yn_track_create: track_low is above track_high"
    for k in ("iou_high", "iou_low", "iou_new"):
        if not 0.0 < float(p[k]) <= 1.0:
            return "yn_track_create: %s outside (0, 1]" % k
    if p["max_lost"] < 0:
        return "yn_track_create: max_lost is negative"
    if p["min_hits"] < 1:
        return "yn_track_create: min_hits is below 1"
    return None


class Tracker:
    """One yn_track: `streams` independent trackers stepped together, `max_tracks` slots and at most `max_dets` detections per frame
    each (1..128).  `params`: track_high, track_low, new_thresh, iou_high, iou_low, iou_new, w_pos, w_vel, max_lost, min_hits,
    class_aware (DEFAULTS)."""

    def __init__(self, streams, max_tracks=128, max_dets=128, handle=None, device=None, **params):
        from . import capi
        self.streams, self.max_tracks, self.max_dets = int(streams), int(max_tracks), int(max_dets)
        self.params = make_params(**params)
        why = refusal(self.streams, self.max_tracks, self.max_dets, self.params)
        if why:
            raise capi.YnError(why)
        self.lib = capi.load_library()
        self._handle, self._device = handle, device
        h = self._h()
        import torch
        cp = TrackParams(**{k: (float(v) if k in FLOAT_PARAMS else v) for k, v in self.params.items()})
        t = ctypes.c_void_p()
        h._ck(self.lib.yn_track_create(h.h, self.streams, self.max_tracks, self.max_dets, ctypes.addressof(cp), ctypes.byref(t)), "yn_track_create")
        self.t = t
        rows = self.streams * self.max_tracks
        self._rec = torch.zeros((rows, 6), dtype=torch.float32, device=h.device)
        self._ids = torch.zeros((rows,), dtype=torch.int32, device=h.device)
        self._off = torch.zeros((self.streams + 1,), dtype=torch.int32, device=h.device)

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
        if getattr(self, "t", None):
            self.lib.yn_track_destroy(self.t)
            self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, rec, offsets, streams=None, handle=None, out=None):
        """One step of the B = len(offsets) - 1 streams named by `streams` (None: 0..B-1) from rec [>= total, 6] float32 / offsets [B+1]
        int32 on the device -> (rec_out [B * max_tracks, 6], ids [B * max_tracks], offsets_out [B+1]); rows offsets_out[b] ..
        offsets_out[b+1] are frame b's tracks in slot order.  offsets_out[B] < 0: the input carried the range mark and nothing was
        stepped.  `out`: three caller-owned device tensors of those shapes to write instead of the tracker's own."""
        import torch
        h = self._h(handle)
        assert rec.is_cuda and offsets.is_cuda and rec.dtype == torch.float32 and offsets.dtype == torch.int32
        assert rec.dim() == 2 and rec.shape[1] == 6 and offsets.dim() == 1 and int(offsets.shape[0]) >= 1, (tuple(rec.shape), tuple(offsets.shape))
        B = int(offsets.shape[0]) - 1
        table = None
        if streams is not None:
            table = np.ascontiguousarray(np.asarray(streams, dtype=np.int64).reshape(-1).astype(np.int32))
            assert len(table) == B, "%d stream indices for %d frames" % (len(table), B)
        if out is None:
            rows = min(B, self.streams) * self.max_tracks       # B > streams is the library's to refuse
            o_rec, o_ids, o_off = self._rec[:rows], self._ids[:rows], self._off[:min(B, self.streams) + 1]
        else:
            o_rec, o_ids, o_off = out
            assert o_rec.is_cuda and o_rec.dtype == torch.float32 and o_rec.is_contiguous() and o_rec.numel() >= B * self.max_tracks * 6
            assert o_ids.is_cuda and o_ids.dtype == torch.int32 and o_ids.is_contiguous() and o_ids.numel() >= B * self.max_tracks
            assert o_off.is_cuda and o_off.dtype == torch.int32 and o_off.is_contiguous() and o_off.numel() >= B + 1
        rec, offsets = h._in(rec), h._in(offsets, torch.int32)
        h._ck(self.lib.yn_track_update(h.h, self.t, B, table.ctypes.data if table is not None else None, rec.data_ptr(), offsets.data_ptr(),
                                       int(rec.shape[0]), o_rec.data_ptr(), o_ids.data_ptr(), o_off.data_ptr()), "yn_track_update")
        return o_rec, o_ids, o_off

    def reset(self, stream=None, handle=None):
        """Frees every slot of `stream` and restarts its ids at 1; None: every stream, and the counters.  Asynchronous."""
        h = self._h(handle)
        h._ck(self.lib.yn_track_reset(h.h, self.t, -1 if stream is None else int(stream)), "yn_track_reset")

    def state(self, stream, handle=None):
        """Testing aid (yn_track_state; synchronises): {'meta': int32 [max_tracks][5] state, id, hits, lost_age, detection matched or born
        from in the last step or -1; 'filt': float32 [max_tracks][22] class, score, then p, v, P00, P01, P11 for cx, cy, w, h; 'next_id'}."""
        h = self._h(handle)
        meta = np.zeros((self.max_tracks, 5), dtype=np.int32)
        filt = np.zeros((self.max_tracks, 22), dtype=np.float32)
        nid = ctypes.c_int32()
        h._ck(self.lib.yn_track_state(h.h, self.t, int(stream), meta.ctypes.data, filt.ctypes.data, ctypes.byref(nid)), "yn_track_state")
        return {"meta": meta, "filt": filt, "next_id": int(nid.value)}

    def status(self, handle=None):
        """The counters since creation / reset(): steps (frames stepped), births, dropped_births, overflow, ignored, range_marks
        (yn_track_status; synchronises)."""
        h = self._h(handle)
        c = np.zeros(6, dtype=np.int64)
        h._ck(self.lib.yn_track_status(h.h, self.t, c.ctypes.data), "yn_track_status")
        return dict(zip(COUNTERS, (int(v) for v in c)))
