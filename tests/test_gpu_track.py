"""Detections tracked across frames on the device (yn_track_*, yolo_nano_amd.track) against the float32 restatement
(tests/track_oracle.py).  After EVERY step of every case the output rows, the ids, the output offsets, the full state of every stream
(yn_track_state) and the counters are compared with the oracle's, all bits equal.  The three output arrays are windows inside larger
device buffers filled with 0xA5; the bytes around the windows, and the rows of the windows past the step's output, must be unchanged.
The exact cases use dyadic thresholds (0.25, 0.5, 0.75), so that a score or an IoU can sit exactly on one."""
import numpy as np
import pytest
import torch

import track_cases as cases
import track_oracle as orc

pytestmark = pytest.mark.gpu

GUARD = 64                                                      # guard elements (4 bytes each) on both sides of a window


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


class Pair:
    """A device tracker and the oracle, stepped together and compared after every step."""

    def __init__(self, streams, max_tracks=128, max_dets=128, handle=None, **kw):
        from yolo_nano_amd import track
        self.dev = track.Tracker(streams, max_tracks, max_dets, handle=handle, **kw)
        self.orc = orc.Tracker(streams, max_tracks, max_dets, **kw)
        for k in orc.FLOAT_PARAMS:                              # both sides hold the same float32 parameters
            assert bits(np.float32(self.dev.params[k])) == bits(np.float32(self.orc.p[k])), k
        self.streams, self.max_tracks = streams, max_tracks

    def step(self, frames, streams=None, mark=False, capacity=None, handle=None):
        """frames: one record array per frame.  capacity: rec_capacity (rows at and past it exist in memory and must not be read)."""
        B = len(frames)
        frames = [np.asarray(f, np.float32).reshape(-1, 6) for f in frames]
        off = np.zeros(B + 1, np.int32)
        off[1:] = np.cumsum([len(f) for f in frames])
        total = int(off[B])
        rows = np.concatenate(frames + [np.zeros((1, 6), np.float32)])
        if mark:
            off[B] = -1
        cap = total + 1 if capacity is None else capacity
        # the oracle sees what lies below the capacity
        seen = [rows[min(off[b], cap):min(max(off[b + 1], off[b]), cap)] for b in range(B)] if not mark else frames
        mt = self.max_tracks
        bufs = [torch.full((4 * (GUARD + n + GUARD),), 0xA5, dtype=torch.uint8, device="cuda").view(dt)
                for n, dt in ((B * mt * 6, torch.float32), (B * mt, torch.int32), (B + 1, torch.int32))]
        before = [b.cpu().numpy().copy() for b in bufs]
        out = (bufs[0][GUARD:GUARD + B * mt * 6].view(B * mt, 6), bufs[1][GUARD:GUARD + B * mt], bufs[2][GUARD:GUARD + B + 1])
        rec_dev = torch.from_numpy(rows).cuda()
        got = self.dev.update(rec_dev[:cap], torch.from_numpy(off).cuda(), streams, handle=handle, out=out)
        assert got[0].data_ptr() == out[0].data_ptr()
        e_rec, e_ids, e_off = self.orc.update(seen, streams, mark=mark)
        host = [b.cpu().numpy() for b in bufs]
        n = len(e_ids)
        g_off = host[2][GUARD:GUARD + B + 1]
        assert np.array_equal(g_off, e_off), (g_off, e_off)
        g_ids = host[1][GUARD:GUARD + n]
        assert np.array_equal(g_ids, e_ids), (g_ids, e_ids)
        g_rec = host[0][GUARD:GUARD + n * 6].reshape(n, 6)
        assert np.array_equal(bits(g_rec), bits(e_rec)), np.nonzero(bits(g_rec) != bits(e_rec))
        # nothing else was written: the guards, and the windows past the output
        for h, b0, used in zip(host, before, (n * 6, n, B + 1)):
            mask = np.ones(len(h), bool)
            mask[GUARD:GUARD + used] = False
            assert np.array_equal(bits(h)[mask], bits(b0)[mask]), "bytes outside the step's output were written"
        self.compare_state(handle)
        return e_rec, e_ids, e_off

    def compare_state(self, handle=None):
        for s in range(self.streams):
            st, ref = self.dev.state(s, handle=handle), self.orc.streams[s]
            assert np.array_equal(st["meta"], ref.meta), (s, np.nonzero(st["meta"] != ref.meta))
            assert np.array_equal(bits(st["filt"]), bits(ref.filt)), (s, np.nonzero(bits(st["filt"]) != bits(ref.filt)))
            assert st["next_id"] == ref.next_id, s
        assert self.dev.status(handle=handle) == self.orc.counters


def test_scripted_scene():
    frames, kw = cases.scripted_scene()
    p = Pair(1, **kw)
    seen = set()
    for f in frames:
        seen.update(p.step([f])[1].tolist())
    assert seen == {1, 2, 3, 4, 5, 7}
    assert p.orc.counters["births"] == 7 and p.orc.streams[0].meta[3, 1] == 7      # F in D's slot, the lowest free one


def test_score_boundaries():
    kw = dict(cases.EXACT, min_hits=1)
    lo, hi, new = 0.25, 0.5, 0.75
    p = Pair(1, 16, 16, **kw)
    scores = [new, cases.below(new), hi, cases.below(hi), lo, cases.below(lo)]
    f = cases.frame(*[cases.box(50 + 100 * i, 50, 40, 40, s, 0) for i, s in enumerate(scores)])
    rec, ids, off = p.step([f])
    assert list(ids) == [1] and p.orc.counters["ignored"] == 1                      # only score == new_thresh is born; below track_low is ignored
    # six confirmed tracks, then the same six scores: >= track_high matches in stage A, >= track_low in stage B, below is not there
    p = Pair(1, 16, 16, **kw)
    p.step([cases.frame(*[cases.box(50 + 100 * i, 50, 40, 40, 0.9, 0) for i in range(6)])])
    rec, ids, off = p.step([f])
    assert list(ids) == [1, 2, 3, 4, 5]
    assert p.orc.streams[0].meta[:6, 0].tolist() == [orc.CONFIRMED] * 5 + [orc.LOST]


def test_iou_boundaries_and_ties():
    kw = dict(cases.EXACT, min_hits=1, iou_high=0.5)
    # a track born from [0,0,4,4] with zero velocity predicts to itself; [0,0,4,2] has IoU 8/16 = 0.5 exactly: matched
    p = Pair(1, 8, 8, **kw)
    p.step([cases.frame([0, 0, 4, 4, 0.9, 0])])
    assert list(p.step([cases.frame([0, 0, 4, 2, 0.9, 0])])[1]) == [1]
    # one ulp less of height: IoU below 0.5, no match, a second track
    p = Pair(1, 8, 8, **kw)
    p.step([cases.frame([0, 0, 4, 4, 0.9, 0])])
    assert list(p.step([cases.frame([0, 0, 4, cases.below(2.0), 0.9, 0])])[1]) == [2]
    # two detections with the same IoU to one track: the lower detection index wins, the other is born
    p = Pair(1, 8, 8, **kw)
    p.step([cases.frame([0, 0, 4, 4, 0.9, 0])])
    p.step([cases.frame([0, 0, 4, 2, 0.9, 0], [0, 2, 4, 4, 0.9, 0])])
    assert p.orc.streams[0].meta[:2, 4].tolist() == [0, 1] and p.orc.streams[0].meta[:2, 1].tolist() == [1, 2]
    # two tracks with the same IoU (8 / 24) to one detection: the lower slot wins
    p = Pair(1, 8, 8, **dict(kw, iou_high=0.25))
    p.step([cases.frame([0, 0, 4, 4, 0.9, 0], [4, 0, 8, 4, 0.9, 0])])
    p.step([cases.frame([2, 0, 6, 4, 0.9, 0])])
    assert p.orc.streams[0].meta[:2, 4].tolist() == [0, -1]
    # best in its row but not in its column: track 0 prefers detection 0 (32 / 96) to detection 1 (28 / 100), detection 0 prefers track 1
    # (48 / 80); the first round takes (1, 0) alone, the second gives track 0 detection 1
    p = Pair(1, 8, 8, **dict(kw, iou_high=0.25))
    p.step([cases.frame([0, 0, 8, 8, 0.9, 0], [6, 0, 14, 8, 0.9, 0])])
    p.step([cases.frame([4, 0, 12, 8, 0.9, 0], [-4.5, 0, 3.5, 8, 0.9, 0])])
    assert p.orc.streams[0].meta[:2, 4].tolist() == [1, 0]


SIZES = [(1, 1), (1, 4), (63, 63), (64, 64), (65, 65), (63, 66), (64, 67), (65, 68), (127, 127), (125, 128), (128, 128), (128, 1), (1, 128)]


@pytest.mark.parametrize("max_tracks, max_dets", SIZES)
def test_sizes(max_tracks, max_dets):
    p = Pair(1, max_tracks, max_dets, min_hits=1)
    f = cases.sizes(max_tracks, max_dets)
    p.step([f[0]])
    c = p.orc.counters
    assert c["overflow"] == 5 and c["births"] == min(max_tracks, max_dets) and c["dropped_births"] == max(0, max_dets - max_tracks)
    p.step([f[1]])
    assert p.orc.counters["overflow"] == 10
    p.step([f[2]])
    if max_dets >= max_tracks + 3 or (max_tracks, max_dets) == (128, 128):
        assert p.orc.counters["dropped_births"] >= 3


@pytest.mark.parametrize("class_aware", [1, 0])
def test_class_aware(class_aware):
    p = Pair(1, 8, 8, min_hits=1, class_aware=class_aware)
    a, b = cases.box(100, 100, 40, 40, 0.9, 0), cases.box(104, 100, 40, 40, 0.8, 1)
    p.step([cases.frame(a, b)])
    # the two swap classes: with classes each track takes the detection of its class, without them the nearer one
    a2, b2 = cases.box(101, 100, 40, 40, 0.9, 1), cases.box(103, 100, 40, 40, 0.8, 0)
    p.step([cases.frame(a2, b2)])
    assert p.orc.streams[0].meta[:2, 4].tolist() == ([1, 0] if class_aware else [0, 1])


def test_degenerate_input():
    kw = dict(min_hits=1, max_lost=3)
    p = Pair(1, 8, 8, **kw)
    nan, inf = np.nan, np.inf
    bad = [[nan, 0, 10, 10, 0.9, 0], [0, -inf, 10, 10, 0.9, 0], [0, 0, inf, 10, 0.9, 0], [0, 0, 10, nan, 0.9, 0], [10, 0, 10, 10, 0.9, 0], [12, 0, 10, 10, 0.9, 0],
           [0, 10, 10, 10, 0.9, 0], [0, 0, 10, 10, nan, 0]]
    p.step([cases.frame(*(bad + [cases.box(100, 100, 40, 40)]))])
    assert p.orc.counters["ignored"] == len(bad) and p.orc.counters["births"] == 1
    p.step([cases.frame()])                                     # an empty frame
    for _ in range(kw["max_lost"]):                             # all frames empty until every slot is free again
        p.step([cases.frame()])
    assert (p.orc.streams[0].meta[:, 0] == orc.FREE).all()
    p.step([])                                                  # B == 0
    assert p.orc.counters["steps"] == 2 + kw["max_lost"]


def test_rec_capacity_below_the_offsets():
    p = Pair(2, 8, 8, min_hits=1)
    f0 = cases.frame(*[cases.box(50 + 100 * i, 50, 40, 40) for i in range(3)])
    f1 = cases.frame(*[cases.box(50 + 100 * i, 300, 40, 40) for i in range(4)])
    p.step([f0, f1], capacity=5)                                # frame 1 is cut after two records
    assert p.orc.counters["births"] == 5
    p.step([f0, f1], capacity=2)                                # frame 0 is cut, frame 1 is empty
    p.step([f0, f1], capacity=0)
    assert p.orc.counters["steps"] == 6


def test_predicted_width_goes_non_positive():
    p = Pair(1, 4, 4, min_hits=1)
    frames = cases.shrinking()
    for k, f in enumerate(frames):
        p.step([f])
        if k == 6:
            m, fl = p.orc.streams[0].meta, p.orc.streams[0].filt
            assert m[0].tolist()[:1] == [orc.LOST] and fl[0, 12] <= 0 and m[1, 1] == 2, "the case did not drive the width through zero"
    assert p.orc.streams[0].filt[0, 12] <= 0 and p.orc.streams[0].meta[0, 0] == orc.LOST


def test_streams():
    scenes = [cases.scripted_scene()[0], cases.crossing(), cases.gap(3, 4, 23)]
    kw = cases.scripted_scene()[1]
    together = Pair(3, 16, 16, **kw)
    alone = [orc.Tracker(1, 16, 16, **kw) for _ in scenes]
    for k in range(30):
        rec, ids, off = together.step([s[k] for s in scenes])
        for b, (a, s) in enumerate(zip(alone, scenes)):
            r1, i1, _ = a.update([s[k]])
            assert np.array_equal(bits(rec[off[b]:off[b + 1]]), bits(r1)) and np.array_equal(ids[off[b]:off[b + 1]], i1)
    for b, a in enumerate(alone):
        assert np.array_equal(together.orc.streams[b].meta, a.streams[0].meta)
    # a call for streams (2, 0): stream 1 keeps every bit (compare_state checks it against the oracle, which did not touch it)
    s1 = together.dev.state(1)
    together.step([scenes[2][5], scenes[0][5]], streams=[2, 0])
    s1b = together.dev.state(1)
    assert np.array_equal(s1["meta"], s1b["meta"]) and np.array_equal(bits(s1["filt"]), bits(s1b["filt"])) and s1["next_id"] == s1b["next_id"]
    # refused before any launch: the state and the counters stay as they are
    from yolo_nano_amd import capi
    rec, off = torch.zeros((4, 6), device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    for table, why in (([1, 1], "yn_track_update: stream 1 is named twice"), ([0, 3], "yn_track_update: frame 1 names stream 3, outside 0..2"),
                       ([-1, 0], "yn_track_update: frame 0 names stream -1, outside 0..2")):
        with pytest.raises(capi.YnError) as e:
            together.dev.update(rec, off, table)
        assert str(e.value) == "yn_track_update: " + why
    with pytest.raises(capi.YnError) as e:
        together.dev.update(rec, torch.zeros(5, dtype=torch.int32, device="cuda"))
    assert str(e.value) == "yn_track_update: yn_track_update: 4 frames for 3 streams"
    together.compare_state()
    # reset(1) restarts stream 1 alone
    together.dev.reset(1)
    together.orc.reset(1)
    together.compare_state()
    assert together.dev.state(1)["next_id"] == 1 and together.dev.state(0)["next_id"] > 1
    rec, ids, off = together.step([scenes[1][0], scenes[1][0]], streams=[1, 2])
    rec, ids, off = together.step([scenes[1][1], scenes[1][1]], streams=[1, 2])
    assert ids[off[0]:off[1]].tolist() == [1, 2]
    together.dev.reset()
    together.orc.reset()
    together.compare_state()
    assert together.dev.status() == dict.fromkeys(orc.COUNTERS, 0)


def test_range_mark():
    p = Pair(2, 8, 8, min_hits=1)
    frames = cases.crossing(6)
    p.step([frames[0], frames[0]])
    p.step([frames[1], frames[1]])
    before = [p.dev.state(s) for s in range(2)]
    rec, ids, off = p.step([frames[2], frames[2]], mark=True)
    assert off.tolist() == [0, 0, -1] and p.orc.counters["range_marks"] == 1 and p.orc.counters["steps"] == 4
    for s in range(2):
        after = p.dev.state(s)
        assert np.array_equal(before[s]["meta"], after["meta"]) and np.array_equal(bits(before[s]["filt"]), bits(after["filt"]))
    # the next good frame continues as if the marked call had not happened
    q = orc.Tracker(2, 8, 8, min_hits=1)
    for k in (0, 1, 2):
        last = q.update([frames[k], frames[k]])
    rec, ids, off = p.step([frames[2], frames[2]])
    assert np.array_equal(bits(rec), bits(last[0])) and np.array_equal(ids, last[1])


def test_seeded_soak():
    steps = cases.soak(5)
    p = Pair(4, 128, 128)
    tracks = 0
    for row in steps:
        tracks += len(p.step(row)[1])
    c = p.orc.counters
    assert tracks > 4000 and c["overflow"] > 0 and c["ignored"] > 0 and c["births"] > 300, (tracks, c)


def test_parameter_refusals_of_the_library():
    """The library's own checks give the text the package gives without a device (tests/test_track_cpu.py)."""
    import ctypes
    from yolo_nano_amd import arch, capi, track
    h = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x")
    lib = capi.load_library()
    for args, kw in (((1, 128, 128), dict(track_high=float("nan"))), ((1, 128, 128), dict(track_low=0.6)), ((1, 128, 128), dict(iou_new=1.5)),
                     ((1, 128, 128), dict(max_lost=-1)), ((1, 128, 128), dict(min_hits=0)), ((0, 128, 128), {}), ((1, 129, 128), {}), ((1, 128, 0), {})):
        p = track.make_params(**kw)
        cp = track.TrackParams(**{k: (float(v) if k in track.FLOAT_PARAMS else v) for k, v in p.items()})
        t = ctypes.c_void_p()
        assert lib.yn_track_create(h.h, *args, ctypes.addressof(cp), ctypes.byref(t)) == 1 and not t.value
        assert lib.yn_last_error(h.h).decode() == track.refusal(*args, p)
    # NULL parameters are the defaults
    t = ctypes.c_void_p()
    assert lib.yn_track_create(h.h, 1, 4, 4, None, ctypes.byref(t)) == 0
    d = track.Tracker(1, 4, 4, handle=h)
    f = torch.from_numpy(cases.frame(cases.box(100, 100, 40, 40, 0.6, 0), cases.box(300, 100, 40, 40, 0.59, 0))).cuda()
    off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
    meta = [np.zeros((4, 5), np.int32), None]
    filt = [np.zeros((4, 22), np.float32), None]
    out = [torch.zeros((4, 6), device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")]
    for _ in range(2):
        assert lib.yn_track_update(h.h, t, 1, None, f.data_ptr(), off.data_ptr(), 2, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()) == 0
        d.update(f, off)
    assert lib.yn_track_state(h.h, t, 0, meta[0].ctypes.data, filt[0].ctypes.data, None) == 0
    s = d.state(0)
    assert np.array_equal(meta[0], s["meta"]) and np.array_equal(bits(filt[0]), bits(s["filt"])) and s["meta"][:, 0].tolist() == [orc.CONFIRMED, 0, 0, 0]
    lib.yn_track_destroy(t)
    d.close()
    h.close()


def test_lifetime():
    import ctypes
    import gc
    from yolo_nano_amd import arch, capi
    lib = capi.load_library()

    def live():
        blocks, nbytes = ctypes.c_int64(), ctypes.c_int64()
        lib.yn_live_device_memory(ctypes.byref(blocks), ctypes.byref(nbytes))
        return blocks.value, nbytes.value

    gc.collect()
    base = live()
    h1 = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x")
    with_h1 = live()
    p = Pair(2, 8, 8, handle=h1, min_hits=1)
    own = (live()[0] - with_h1[0], live()[1] - with_h1[1])
    assert own[0] >= 3 and own[1] >= 2 * 8 * (5 + 22 + 7) * 4, own          # the state and the staging rows are device memory of the object
    frames = cases.crossing(4)
    p.step([frames[0], frames[0]], handle=h1)
    p.step([frames[1], frames[1]], handle=h1)
    h2 = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x")
    h1.close()                                                  # the tracker outlives the handle it was made with
    p.dev._handle = h2
    rec, ids, off = p.step([frames[2], frames[2]], handle=h2)
    assert ids.tolist() == [1, 2, 1, 2]
    before = live()
    p.dev.close()
    assert (before[0] - live()[0], before[1] - live()[1]) == own
    h2.close()
    assert live() == base


def test_end_to_end_with_the_golden_net():
    """net_coco128_b2's network on its two-image batch, shifted two pixels per step for five steps: YOLONano -> yn_infer ->
    yn_pack_detections -> Tracker.update; the oracle is fed the read-back records; rec_out goes through Visualizer.batch."""
    import yolo_nano_amd
    from yolo_nano_amd import arch, voc_geometry, weights
    S, C = 128, 80
    sd = weights.make_state_dict("1.0x", C)
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, conf_thresh=0.001, nms_thresh=0.5, anchor_size=arch.MULTI_ANCHOR_SIZE_COCO)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to("cuda").eval()
    h = m.handle(2)
    x0 = torch.from_numpy(weights.make_input(2, S, seed=2)).cuda()
    out = h.infer(x0)
    scores = np.concatenate([d[1] for d in h.detections_to_host(out)])
    assert len(scores) >= 8
    hi, lo = float(np.median(scores)), float(np.quantile(scores, 0.25))
    p = Pair(2, 128, 128, handle=h, track_high=hi, new_thresh=hi, track_low=lo)
    vis = yolo_nano_amd.Visualizer(["c%d" % i for i in range(C)], yolo_nano_amd.class_colors(C), vis_thresh=0.0, handle=h)
    shown = 0
    for k in range(5):
        x = torch.roll(x0, shifts=(2 * k, 2 * k), dims=(2, 3)).contiguous()
        rec, off = h.pack_detections(h.infer(x))
        off_h = off.cpu().numpy()
        assert off_h[2] >= 0, "the range mark: the case needs the exact route"
        rec_h = rec.cpu().numpy()
        frames = [rec_h[off_h[b]:off_h[b + 1]] for b in range(2)]
        e_rec, e_ids, e_off = p.step(frames, handle=h)
        shown += len(e_ids)
    assert shown > 0, "no track was ever confirmed: the case shows nothing"
    # once more through the tracker's own buffers, which is what a caller hands to the painter
    q = yolo_nano_amd.Tracker(2, handle=h, track_high=hi, new_thresh=hi, track_low=lo, min_hits=1)
    rec_out, ids, off_out = q.update(rec, off, handle=h)
    frames_dev = [torch.zeros((S, S, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    vis.batch(frames_dev, rec_out, off_out, [voc_geometry(S, S, S)] * 2, handle=h)
    st = vis.status(h)
    assert not st["range_mark"] and st["drawn"] + st["skipped"] == int(off_out.cpu()[2]) > 0
    assert sum(int(f.any()) for f in frames_dev) >= 1
