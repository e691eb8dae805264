"""The tracker's rules (yn_track_*) restated in float32 numpy, one operation at a time: the specification the kernel
(csrc/kernels_track.hip) has to meet bit for bit.  Every array expression below is elementwise float32, written in the order the kernel
evaluates it; nothing is fused and nothing is reassociated.  State lives in plain arrays of the yn_track_state layout:

    meta int32   [max_tracks][5]   state, id, hits, lost_age, detection matched (or born from) in the last step or -1
    filt float32 [max_tracks][22]  class, score, then p, v, P00, P01, P11 for cx, cy, w, h
"""
import numpy as np

FREE, TENTATIVE, CONFIRMED, LOST = 0, 1, 2, 3
F32 = np.float32

DEFAULTS = dict(track_high=0.5, track_low=0.1, new_thresh=0.6, iou_high=0.2, iou_low=0.5, iou_new=0.3, w_pos=1.0 / 20.0, w_vel=1.0 / 160.0,
                max_lost=30, min_hits=2, class_aware=1)
FLOAT_PARAMS = ("track_high", "track_low", "new_thresh", "iou_high", "iou_low", "iou_new", "w_pos", "w_vel")
COUNTERS = ("steps", "births", "dropped_births", "overflow", "ignored", "range_marks")


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    for k in FLOAT_PARAMS:
        p[k] = F32(p[k])
    return p


def _base(k):
    return 2 + 5 * k                                            # the filter of coordinate k (cx, cy, w, h) starts here in a filt row


def _scales(filt, idx):
    """The noise scale of each coordinate, read before the step: the track's w for cx and w, its h for cy and h."""
    w, h = filt[idx, _base(2)].copy(), filt[idx, _base(3)].copy()
    return (w, h, w, h)


def kf_initiate(filt, idx, z, p):
    """z [n][4] = cx, cy, w, h of the measurements the tracks idx start from."""
    s4 = (z[:, 2], z[:, 3], z[:, 2], z[:, 3])
    for k in range(4):
        b, s = _base(k), s4[k]
        t0 = F32(2.0) * p["w_pos"] * s
        t1 = F32(10.0) * p["w_vel"] * s
        filt[idx, b + 0] = z[:, k]
        filt[idx, b + 1] = F32(0)
        filt[idx, b + 2] = t0 * t0
        filt[idx, b + 3] = F32(0)
        filt[idx, b + 4] = t1 * t1


def kf_predict(filt, idx, p):
    s4 = _scales(filt, idx)
    for k in range(4):
        b, s = _base(k), s4[k]
        q = p["w_pos"] * s
        qv = p["w_vel"] * s
        P00, P01, P11 = filt[idx, b + 2], filt[idx, b + 3], filt[idx, b + 4]
        filt[idx, b + 0] = filt[idx, b + 0] + filt[idx, b + 1]
        filt[idx, b + 2] = ((P00 + F32(2.0) * P01) + P11) + q * q
        filt[idx, b + 3] = P01 + P11
        filt[idx, b + 4] = P11 + qv * qv


def kf_update(filt, idx, z, p):
    s4 = _scales(filt, idx)
    for k in range(4):
        b, s = _base(k), s4[k]
        q = p["w_pos"] * s
        P00, P01, P11 = filt[idx, b + 2], filt[idx, b + 3], filt[idx, b + 4]
        S = P00 + q * q
        K0 = P00 / S
        K1 = P01 / S
        r = z[:, k] - filt[idx, b + 0]
        filt[idx, b + 0] = filt[idx, b + 0] + K0 * r
        filt[idx, b + 1] = filt[idx, b + 1] + K1 * r
        filt[idx, b + 2] = P00 - (K0 * K0) * S
        filt[idx, b + 3] = P01 - (K0 * K1) * S
        filt[idx, b + 4] = P11 - (K1 * K1) * S


def measurement(rec):
    """rec [n][>=4] float32 -> z [n][4] = cx, cy, w, h."""
    x1, y1, x2, y2 = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    return np.stack([F32(0.5) * (x1 + x2), F32(0.5) * (y1 + y2), x2 - x1, y2 - y1], axis=1).astype(F32)


def corners(cx, cy, w, h):
    return cx - F32(0.5) * w, cy - F32(0.5) * h, cx + F32(0.5) * w, cy + F32(0.5) * h


def _min(a, b):
    return np.where(a < b, a, b)                                # the kernel's a < b ? a : b, not fminf


def _max(a, b):
    return np.where(a > b, a, b)


def iou_matrix(tb, db):
    """tb: the tracks' (x1, y1, x2, y2) as [T] arrays, db: the detections' as [D] arrays -> float32 [T][D]."""
    ax1, ay1, ax2, ay2 = (v[:, None] for v in tb)
    bx1, by1, bx2, by2 = (v[None, :] for v in db)
    iw = _min(ax2, bx2) - _max(ax1, bx1)
    ih = _min(ay2, by2) - _max(ay1, by1)
    iw = np.where(iw > 0, iw, F32(0))
    ih = np.where(ih > 0, ih, F32(0))
    inter = iw * ih
    area_a = (ax2 - ax1) * (ay2 - ay1)
    area_b = (bx2 - bx1) * (by2 - by1)
    union = (area_a + area_b) - inter
    pos = union > 0
    return np.where(pos, inter / np.where(pos, union, F32(1)), F32(0)).astype(F32)


def greedy_sequential(iou, rows, cols, thr):
    """Repeatedly the eligible pair of the highest IoU among the open rows and columns; ties to the lowest row, then the lowest column.
    iou [T][D] (an ineligible pair holds a negative value), rows / cols boolean masks of the open ones -> list of (row, column)."""
    m = np.where(rows[:, None] & cols[None, :] & (iou >= thr), iou, F32(-1))
    out = []
    if m.size == 0:
        return out
    while True:
        k = int(np.argmax(m))                                   # first occurrence in row-major order: lowest row, then lowest column
        r, c = divmod(k, m.shape[1])
        if not m[r, c] >= 0:
            return out
        out.append((r, c))
        m[r, :] = -1
        m[:, c] = -1


def greedy_rounds(iou, rows, cols, thr):
    """What the kernel does: in rounds, every pair that is the best of its row (ties: lowest column) and the best of its column (ties:
    lowest row) among the pairs still open.  -> (pairs, rounds)"""
    m = np.where(rows[:, None] & cols[None, :] & (iou >= thr), iou, F32(-1))
    out, rounds = [], 0
    if m.size == 0:
        return out, rounds
    while True:
        rb = np.argmax(m, axis=1)                               # first maximum: lowest column
        cb = np.argmax(m, axis=0)                               # first maximum: lowest row
        took = [(r, int(rb[r])) for r in range(m.shape[0]) if m[r, rb[r]] >= 0 and cb[rb[r]] == r]
        if not took:
            return out, rounds
        rounds += 1
        for r, c in took:
            out.append((r, c))
            m[r, :] = -1
            m[:, c] = -1


class Stream:
    def __init__(self, max_tracks):
        self.meta = np.zeros((max_tracks, 5), np.int32)
        self.meta[:, 4] = -1
        self.filt = np.zeros((max_tracks, 22), F32)
        self.next_id = 1


class Tracker:
    def __init__(self, streams, max_tracks=128, max_dets=128, **kw):
        self.p = params(**kw)
        self.max_tracks, self.max_dets = int(max_tracks), int(max_dets)
        self.streams = [Stream(self.max_tracks) for _ in range(streams)]
        self.counters = dict.fromkeys(COUNTERS, 0)

    def reset(self, stream=None):
        if stream is None:
            self.streams = [Stream(self.max_tracks) for _ in self.streams]
            self.counters = dict.fromkeys(COUNTERS, 0)
        else:
            self.streams[stream] = Stream(self.max_tracks)

    def update(self, frames, streams=None, mark=False):
        """frames: one float32 [n][6] record array per frame, frame b for stream streams[b] (None: b).  mark: the call carried the range
        mark.  -> (rec [total][6], ids [total], offsets [B+1])"""
        B = len(frames)
        off = np.zeros(B + 1, np.int32)
        if mark:
            self.counters["range_marks"] += 1
            off[B] = -1
            return np.zeros((0, 6), F32), np.zeros(0, np.int32), off
        recs, ids = [], []
        for b, fr in enumerate(frames):
            r, i = self.step(self.streams[b if streams is None else streams[b]], np.asarray(fr, F32).reshape(-1, 6))
            recs.append(r)
            ids.append(i)
            off[b + 1] = off[b] + len(i)
        return (np.concatenate(recs) if recs else np.zeros((0, 6), F32)), (np.concatenate(ids) if ids else np.zeros(0, np.int32)), off

    def step(self, st, rec):
        p, meta, filt = self.p, st.meta, st.filt
        with np.errstate(all="ignore"):
            # 1. detections
            usable = np.isfinite(rec[:, :4]).all(axis=1) & (rec[:, 2] > rec[:, 0]) & (rec[:, 3] > rec[:, 1]) & (rec[:, 4] >= p["track_low"])
            n_usable = int(usable.sum())
            det = rec[usable][:self.max_dets]
            D = len(det)
            self.counters["steps"] += 1
            self.counters["ignored"] += len(rec) - n_usable
            self.counters["overflow"] += n_usable - D
            high = det[:, 4] >= p["track_high"]
            z = measurement(det)
            # 2. predict
            state0 = meta[:, 0].copy()
            lost = np.nonzero(state0 == LOST)[0]
            filt[lost, _base(2) + 1] = 0
            filt[lost, _base(3) + 1] = 0
            live = np.nonzero(state0 != FREE)[0]
            kf_predict(filt, live, p)
            w, h = filt[:, _base(2)], filt[:, _base(3)]
            valid = (state0 != FREE) & np.isfinite(w) & np.isfinite(h) & (w > 0) & (h > 0)
            # 3. IoU
            iou = iou_matrix(corners(filt[:, _base(0)], filt[:, _base(1)], w, h), (det[:, 0], det[:, 1], det[:, 2], det[:, 3]))
            ok = valid[:, None] & np.ones(D, bool)[None, :]
            if p["class_aware"]:
                ok &= filt[:, 0][:, None] == det[:, 5][None, :]
            iou = np.where(ok, iou, F32(-1))
            # 4. matching
            tmatch = np.full(self.max_tracks, -1, np.int64)
            dmatch = np.full(D, -1, np.int64)
            for rows, cols, thr in (((state0 == CONFIRMED) | (state0 == LOST), high, p["iou_high"]),
                                    (state0 == CONFIRMED, ~high, p["iou_low"]),
                                    (state0 == TENTATIVE, high, p["iou_new"])):
                for r, c in greedy_sequential(iou, rows & valid & (tmatch < 0), cols & (dmatch < 0), thr):
                    tmatch[r], dmatch[c] = c, r
            # 5. matched tracks
            m = np.nonzero(tmatch >= 0)[0]
            kf_update(filt, m, z[tmatch[m]], p)
            filt[m, 0] = det[tmatch[m], 5]
            filt[m, 1] = det[tmatch[m], 4]
            meta[m, 2] += 1
            meta[m, 3] = 0
            meta[m, 4] = tmatch[m]
            promote = m[(state0[m] == LOST) | ((state0[m] == TENTATIVE) & (meta[m, 2] >= p["min_hits"]))]
            meta[promote, 0] = CONFIRMED
            # 6. unmatched tracks
            u = (tmatch < 0) & (state0 != FREE)
            meta[u, 4] = -1
            c = np.nonzero(u & (state0 == CONFIRMED))[0]
            meta[c, 0], meta[c, 3] = LOST, 1
            lo = np.nonzero(u & (state0 == LOST))[0]
            meta[lo, 3] += 1
            gone = np.concatenate([np.nonzero(u & (state0 == TENTATIVE))[0], lo[meta[lo, 3] > p["max_lost"]]])
            meta[gone] = (FREE, 0, 0, 0, -1)
            filt[gone] = 0
            # 7. births
            cand = np.nonzero(high & (dmatch < 0) & (det[:, 4] >= p["new_thresh"]))[0]
            free = np.nonzero(meta[:, 0] == FREE)[0]
            n = min(len(cand), len(free))
            self.counters["births"] += n
            self.counters["dropped_births"] += len(cand) - n
            cand, free = cand[:n], free[:n]
            kf_initiate(filt, free, z[cand], p)
            filt[free, 0] = det[cand, 5]
            filt[free, 1] = det[cand, 4]
            meta[free, 0] = CONFIRMED if p["min_hits"] <= 1 else TENTATIVE
            meta[free, 1] = st.next_id + np.arange(n)
            meta[free, 2] = 1
            meta[free, 3] = 0
            meta[free, 4] = cand
            st.next_id += n
            # 8. output
            e = np.nonzero((meta[:, 0] == CONFIRMED) & (meta[:, 4] >= 0))[0]
            x1, y1, x2, y2 = corners(filt[e, _base(0)], filt[e, _base(1)], filt[e, _base(2)], filt[e, _base(3)])
            out = np.stack([x1, y1, x2, y2, filt[e, 1], filt[e, 0]], axis=1).astype(F32).reshape(-1, 6)
            return out, meta[e, 1].astype(np.int32)
