"""Scenario builders for the tracker tests (tests/test_track_cpu.py, tests/test_gpu_track.py): every builder returns a list of frames,
a frame being a float32 [n][6] record array x1, y1, x2, y2, score, class, plus whatever the case needs.  numpy only."""
import numpy as np

F32 = np.float32
# the exact cases use dyadic thresholds, so that a score or an IoU can sit exactly on one
EXACT = dict(track_high=0.5, track_low=0.25, new_thresh=0.75, iou_high=0.25, iou_low=0.5, iou_new=0.25)


def box(cx, cy, w, h, score=0.9, cls=0):
    return [cx - w / 2.0, cy - h / 2.0, cx + w / 2.0, cy + h / 2.0, score, cls]


def frame(*rows):
    return np.asarray(rows, dtype=F32).reshape(-1, 6)


def below(v):
    """One float32 ulp below v."""
    return np.nextafter(F32(v), F32(-np.inf))


def scripted_scene():
    """One stream, 30 frames, six objects, max_lost = 4, min_hits = 2 (EXACT thresholds):
      A, B  cross each other around frame 12 on rows half a box apart
      C     is hidden in frames 8..10 (an occlusion shorter than max_lost) and comes back
      D     leaves after frame 9 and dies; its slot is the lowest free one when F is born in frame 20
      E     is seen at a low score from frame 15 on: it stays alive through stage B
      F     is born late, G appears in a single frame and never shows"""
    frames = []
    for t in range(30):
        rows = [box(40 + 6 * t, 100, 40, 40, 0.9, 0),            # A, left to right
                box(220 - 6 * t, 120, 40, 40, 0.85, 0)]          # B, right to left
        if not 8 <= t <= 10:
            rows.append(box(300 + 2 * t, 300 + t, 50, 30, 0.8, 1))                 # C
        if t <= 9:
            rows.append(box(500, 80 + 3 * t, 30, 60, 0.95, 2))                     # D
        rows.append(box(100 + t, 400, 60, 60, 0.9 if t < 15 else 0.3, 1))          # E
        if t >= 20:
            rows.append(box(600 - 4 * t, 250, 40, 40, 0.8, 0))                     # F
        if t == 5:
            rows.append(box(700, 700, 20, 20, 0.99, 2))                            # G
        frames.append(frame(*rows))
    return frames, dict(EXACT, max_lost=4, min_hits=2)


def crossing(steps=30):
    """Two objects of one class that pass each other on rows half a box apart -> frames; object 0 is always record 0."""
    return [frame(box(40 + 6 * t, 100, 40, 40, 0.9, 0), box(220 - 6 * t, 120, 40, 40, 0.9, 0)) for t in range(steps)]


def gap(before, empty, after, score=0.9):
    """One still object for `before` frames, `empty` empty frames, the object again for `after` frames."""
    f = frame(box(100, 100, 40, 40, score, 0))
    return [f] * before + [frame()] * empty + [f] * after


def grid(n, score=0.9, cls=0, pitch=60.0, size=40.0, dx=0.0):
    """n separated boxes on a 16-column grid."""
    return frame(*[box(50 + pitch * (i % 16) + dx, 50 + pitch * (i // 16), size, size, score, cls) for i in range(n)])


def sizes(max_tracks, max_dets):
    """Frame 0: max_dets + 5 separated boxes (5 overflow; births fill the table, the rest are dropped).  Frame 1: the same, one pixel on.
    Frame 2: three new boxes first, then frame 0's boxes without its first three."""
    f0 = grid(max_dets + 5)
    new = frame(*[box(50 + 60 * i, 1500, 40, 40, 0.9, 0) for i in range(3)])
    return [f0, grid(max_dets + 5, dx=1.0), np.concatenate([new, f0[3:]])]


def soak(seed, streams=4, steps=40, objects=(128, 90, 40, 128)):
    """Random-walk boxes with dropouts, clutter, exact duplicates (ties), unusable records and shuffled order -> frames[step][stream]."""
    rng = np.random.RandomState(seed)
    pos = [rng.uniform(0, 1000, size=(n, 2)) for n in objects]
    vel = [rng.uniform(-3, 3, size=(n, 2)) for n in objects]
    size = [rng.uniform(20, 80, size=(n, 2)) for n in objects]
    cls = [rng.randint(0, 3, size=n) for n in objects]
    out = []
    for _ in range(steps):
        row = []
        for s in range(streams):
            n = objects[s]
            pos[s] = pos[s] + vel[s] + rng.normal(0, 0.5, size=(n, 2))
            keep = rng.uniform(size=n) > 0.1
            sc = rng.uniform(0.15, 1.0, size=n)
            rows = [box(pos[s][i, 0], pos[s][i, 1], size[s][i, 0], size[s][i, 1], sc[i], cls[s][i]) for i in range(n) if keep[i]]
            for _ in range(rng.randint(0, 10)):                                    # clutter
                rows.append(box(rng.uniform(0, 1000), rng.uniform(0, 1000), rng.uniform(10, 60), rng.uniform(10, 60), rng.uniform(0.05, 0.7), rng.randint(0, 3)))
            for i in rng.randint(0, max(len(rows), 1), size=len(rows) // 20):      # duplicates: equal IoU to the same track
                rows.append(list(rows[i]))
            if rng.uniform() < 0.3:
                rows.append([np.nan, 0, 10, 10, 0.9, 0])
                rows.append([10, 10, 5, 20, 0.9, 0])
            order = rng.permutation(len(rows))
            row.append(frame(*[rows[i] for i in order]))
        out.append(row)
    return out


def shrinking():
    """A box whose width halves towards nothing (min_hits = 1): the filter's width velocity builds up to about -5.5 while the width falls
    to 4, so in frame 6 the predicted width is negative.  The track matches nothing in that step although a detection lies on it: it goes
    lost, keeps the non-positive width (a lost track's width velocity is zeroed) and a second track is born from the detection."""
    return [frame(box(100, 100, w, 40, 0.9, 0)) for w in (40, 32, 24, 16, 8, 4, 2, 1, 1, 1)]
