"""Detections cut out of device frames as chips (yn_chip_*, yolo_nano_amd.chips) against the restatement (tests/chip_oracle.py) on the
shared case table (tests/chip_cases.py).  Every comparison is all bytes / bits equal.  Frames are windows of larger device buffers at
four alignments; every output buffer is pre-filled with 0xA5 and carries 64 guard bytes: slots past the count and the guards must
still hold 0xA5 afterwards."""
import ctypes

import numpy as np
import pytest
import torch

import chip_cases as cc
import chip_oracle as orc
from oracle.preprocess import letterbox_geometry

pytestmark = pytest.mark.gpu

GUARD = 64
FIT_NAMES, FORMAT_NAMES = {0: "letterbox", 1: "stretch"}, {0: "u8", 1: "f32"}


@pytest.fixture(scope="module")
def handle():
    from yolo_nano_amd import arch, capi
    return capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=torch.device("cuda", torch.cuda.current_device()))


def upload_frames(frames):
    """Host frames as windows of device buffers whose start is dword-aligned for one frame in four."""
    bufs, views = [], []
    for i, f in enumerate(frames):
        n, shift = f.size, i % 4
        buf = torch.full((GUARD + shift + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        buf[GUARD + shift:GUARD + shift + n] = torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).cuda()
        bufs.append(buf)
        views.append(buf[GUARD + shift:GUARD + shift + n].view(f.shape))
    return bufs, views


def extractor(case, handle, **kw):
    from yolo_nano_amd import chips
    p = case["params"]
    classes = None if case["keep"] is None else [c for c, k in enumerate(case["keep"]) if k]
    args = dict(size=(p["cw"], p["ch"]), fit=FIT_NAMES[p["fit"]], out=FORMAT_NAMES[p["format"]], margin=p["margin_permille"] / 1000.0,
                margin_px=p["margin_px"], min_score=float(p["min_score"]), min_side=p["min_side"], classes=classes, max_chips=case["max_chips"],
                num_classes=case["num_classes"], mean=cc.MEAN, std=cc.STD, fill=tuple(float(v) for v in p["fill"]), handle=handle)
    args.update(kw)
    cut = chips.ChipExtractor(**args)
    assert cut.params["margin_permille"] == p["margin_permille"]
    return cut


class Outputs:
    """The four output buffers of one extractor, each a window of a 0xA5 buffer with GUARD bytes behind it."""

    def __init__(self, cut, B):
        n = cut.max_chips
        item = 1 if cut.out == "u8" else 4
        self.sizes = [n * cut.ch * cut.cw * 3 * item, n * 4, (B + 1) * 4, n * 8 * 4]
        self.raw = [torch.full((s + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for s in self.sizes]
        chips = self.raw[0][:self.sizes[0]]
        chips = chips.view(n, cut.ch, cut.cw, 3) if cut.out == "u8" else chips.view(torch.float32).view(n, 3, cut.ch, cut.cw)
        self.tensors = (chips, self.raw[1][:self.sizes[1]].view(torch.int32), self.raw[2][:self.sizes[2]].view(torch.int32),
                        self.raw[3][:self.sizes[3]].view(torch.int32).view(n, 8))
        assert chips.data_ptr() % 16 == 0

    def host(self):
        return [r.cpu().numpy() for r in self.raw]

    def untouched(self):
        return all((h == 0xA5).all() for h in self.host())


def check(outs, cut, want, B):
    """All bytes of the four buffers against the oracle's result: the used slots equal, everything else still 0xA5."""
    chips_h, index_h, off_h, rect_h = outs.host()
    n = len(want["chips"])
    off = off_h[:(B + 1) * 4].view(np.int32)
    assert off.tolist() == want["offsets"], (off.tolist(), want["offsets"])
    assert (off_h[(B + 1) * 4:] == 0xA5).all(), "guard bytes behind chip_offsets were written"
    assert index_h[:n * 4].view(np.int32).tolist() == want["index"]
    assert (index_h[n * 4:] == 0xA5).all(), "index was written past the count"
    assert rect_h[:n * 32].view(np.int32).reshape(n, 8).tolist() == want["rects"]
    assert (rect_h[n * 32:] == 0xA5).all(), "rects were written past the count"
    per = cut.ch * cut.cw * 3 * (1 if cut.out == "u8" else 4)
    assert (chips_h[n * per:] == 0xA5).all(), "chips were written past the count"
    for k in range(n):
        got = chips_h[k * per:(k + 1) * per]
        exp = np.ascontiguousarray(want["chips"][k]).view(np.uint8).reshape(-1)
        if not np.array_equal(got, exp):
            bad = np.nonzero(got != exp)[0]
            raise AssertionError("slot %d (record %d, rect %s): %d of %d bytes differ, first at %d: got %d, expected %d" % (
                k, want["index"][k], want["rects"][k], len(bad), per, bad[0], got[bad[0]], exp[bad[0]]))


def run_case(case, handle, cut=None, repeat=2):
    frames, geoms, rows, off, cap = cc.materialise(case)
    want = orc.extract(frames, geoms, case["space"], rows, off, cap, case["params"], case["num_classes"], case["keep"], case["max_chips"])
    bufs, views = upload_frames(frames)
    clean = [b.clone() for b in bufs]
    cut = cut or extractor(case, handle)
    B = len(frames)
    rec, offsets = torch.from_numpy(rows[:max(cap, 1)]).cuda(), torch.from_numpy(off).cuda()      # no row at or past rec_capacity exists
    for _ in range(repeat):                                     # the same object, the same result
        outs = Outputs(cut, B)
        got = cut.batch(views, rec, offsets, geoms if case["space"] == orc.LETTERBOX else None, pixels=case["space"] == orc.PIXELS, out=outs.tensors)
        assert got[2].shape[0] == B + 1
        check(outs, cut, want, B)
        st = cut.status()
        assert (st["chips"], st["skipped"], st["overflow"], int(st["range_mark"])) == want["counters"], (st, want["counters"])
        assert cut.count() == want["offsets"][-1]
    assert all(torch.equal(a, b) for a, b in zip(bufs, clean)), "a frame was written"      # the frames are read only
    return cut, want, views, rec, offsets


@pytest.mark.parametrize("name", cc.NAMES)
def test_case_against_the_oracle(name, handle):
    case = cc.CASES[cc.NAMES.index(name)]
    cut, want, *_ = run_case(case, handle)
    cut.close()


def test_lifetime_second_handle_and_live_memory(handle):
    from yolo_nano_amd import arch, capi
    lib = capi.load_library()

    def live():
        blocks, nbytes = ctypes.c_int64(), ctypes.c_int64()
        lib.yn_live_device_memory(ctypes.byref(blocks), ctypes.byref(nbytes))
        return blocks.value, nbytes.value

    other = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=handle.device)
    torch.cuda.synchronize()
    before = live()
    case = cc.CASES[cc.NAMES.index("chunks_257_513")]
    cut, want, views, rec, offsets = run_case(case, handle)
    assert live()[1] > before[1], "the object's buffers do not show in yn_live_device_memory"
    outs = Outputs(cut, 2)
    cut.batch(views, rec, offsets, None, pixels=True, out=outs.tensors, handle=other)      # a second handle of the same device
    check(outs, cut, want, 2)
    assert cut.status(handle=other)["chips"] == want["counters"][0]
    small = cc.CASES[cc.NAMES.index("modes_u8_stretch_8x8")]    # fewer records and frames after more: the work buffers stay
    frames, geoms, rows, off, cap = cc.materialise(small)
    _, v2 = upload_frames(frames)
    grown = live()
    o2 = Outputs(cut, 1)
    cut.batch(v2, torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda(), None, pixels=True, out=o2.tensors)
    torch.cuda.synchronize()
    assert live() == grown
    cut.close()
    assert live() == before
    del other


def test_f32_letterbox_chips_are_preprocess_batch_of_the_crops(handle):
    """No oracle: the device's own yn_preprocess_batch on torch-cropped contiguous sub-images."""
    from yolo_nano_amd import chips
    side = 32
    frames = [cc.frame_pixels(50, 130, 37), cc.frame_pixels(51, 64, 64)]
    _, views = upload_frames(frames)
    boxes = [[(3, 2, 3 + side - 1, 2 + side - 1), (0, 0, 63, 35), (10, 1, 73, 36), (100, 5, 129, 36), (40, 0, 40, 36), (7, 9, 70, 9)],
             [(0, 0, 63, 63), (5, 5, 5 + side - 1, 5 + side - 1), (13, 3, 27, 44), (1, 20, 59, 29), (30, 30, 60, 46)]]      # the exact 2:1, a copy, linear
    rows = np.asarray([b + (0.9, 1) for per in boxes for b in per], dtype=np.float32)
    off = np.asarray([0, len(boxes[0]), len(rows)], dtype=np.int32)
    cut = chips.ChipExtractor(size=(side, side), fit="letterbox", out="f32", min_score=0.3, min_side=1, max_chips=16, handle=handle)
    got, index, chip_off, rects = cut.batch(views, torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda(), None, pixels=True)
    crops, geoms = [], []
    for b, per in enumerate(boxes):
        for x1, y1, x2, y2 in per:
            sw, sh = x2 - x1 + 1, y2 - y1 + 1
            rw, rh, left, top = letterbox_geometry(sh, sw, side)[:4]
            if rw == 0 or rh == 0:
                continue
            crops.append(views[b][y1:y2 + 1, x1:x2 + 1].contiguous())
            geoms.append((rw, rh, left, top))
    want = handle.preprocess_batch(crops, geoms, side, cc.MEAN, cc.STD)
    n = cut.count()
    assert n == len(crops) and 9 <= n < len(rows), "the 64x1 box must letterbox to nothing, the rest must survive"
    assert torch.equal(got[:n].view(torch.int32), want.view(torch.int32))
    assert cut.status() == {"chips": n, "skipped": len(rows) - n, "overflow": 0, "range_mark": False}
    cut.close()


def test_jpeg_encoder_takes_the_chips(handle):
    from yolo_nano_amd import jpeg
    case = cc.CASES[cc.NAMES.index("aspects_u8_letterbox_32x32")]
    cut, want, views, rec, offsets = run_case(case, handle, repeat=1)
    chips, _, _, _ = cut.batch(views, rec, offsets, None, pixels=True)
    n = cut.count()
    assert n == len(want["chips"]) >= 8
    enc = jpeg.JPEGEncoder(max_batch=16, handle=handle)
    mine = enc.batch(list(chips[:n]))
    theirs = enc.batch([torch.from_numpy(c).cuda() for c in want["chips"]])
    assert len(mine) == n and all(a == b and a[:2] == b"\xff\xd8" for a, b in zip(mine, theirs))
    cut.close()


def test_tracker_output_is_accepted(handle):
    from yolo_nano_amd import chips, track
    frames = [cc.frame_pixels(60, 130, 37), cc.frame_pixels(61, 64, 64)]
    _, views = upload_frames(frames)
    rows = np.asarray([[5, 3, 40, 30, 0.9, 1], [60, 2, 120, 35, 0.8, 2], [4, 4, 30, 50, 0.95, 3], [20, 10, 60, 60, 0.7, 0], [35, 5, 50, 20, 0.85, 5]], np.float32)
    rec, off = torch.from_numpy(rows).cuda(), torch.tensor([0, 2, 5], dtype=torch.int32).cuda()
    tracker = track.Tracker(2, max_tracks=8, max_dets=8, handle=handle, min_hits=1)
    for _ in range(2):
        t_rec, t_ids, t_off = tracker.update(rec, off)
    cut = chips.ChipExtractor(size=(16, 8), fit="stretch", out="u8", min_score=0.3, max_chips=8, handle=handle)
    outs = Outputs(cut, 2)
    _, index, chip_off, _ = cut.batch(views, t_rec, t_off, None, pixels=True, out=outs.tensors)
    n = cut.count()
    host_rec, host_off = t_rec.cpu().numpy(), t_off.cpu().numpy()
    assert host_off[2] >= 3, "the tracker confirmed nothing: the test checks nothing"
    want = orc.extract(frames, [(130, 37, 0, 0, 0, 0, 0), (64, 64, 0, 0, 0, 0, 0)], orc.PIXELS, host_rec, host_off, len(host_rec),
                       cc.params((16, 8), orc.FIT_STRETCH, orc.U8, fill=(0, 0, 0)), 20, None, 8)
    check(outs, cut, want, 2)
    assert n == len(want["chips"]) >= 3
    ids = t_ids[index[:n].long()].cpu().numpy()                 # one gather: the identity of every chip
    first = int(chip_off[1].item())                             # a stream counts its own ids from 1: unique within a frame
    assert (ids >= 1).all() and len(set(ids[:first].tolist())) == first and len(set(ids[first:].tolist())) == n - first
    cut.close()
    tracker.close()


def test_create_refusals_on_the_library(handle):
    """yn_chip_create itself (ChipExtractor refuses the same configurations before it gets there): 1, the documented message, no object."""
    from yolo_nano_amd import capi, chips
    lib = capi.load_library()
    for kw, reason in cc.REFUSALS:
        kw = dict(kw)
        kw.setdefault("out", "f32")
        nc, mc = kw.pop("num_classes", 20), kw.pop("max_chips", 1024)
        p = chips.make_params(**kw)
        cp = chips.ChipParams(**{k: p[k] for k in chips.INT_PARAMS})
        cp.min_score = float(p["min_score"])
        for k in ("fill", "mean", "std"):
            for i in range(3):
                getattr(cp, k)[i] = float(p[k][i])
        c = ctypes.c_void_p()
        assert lib.yn_chip_create(handle.h, nc, None, mc, ctypes.addressof(cp), ctypes.byref(c)) == 1, kw
        assert lib.yn_last_error(handle.h).decode() == reason and not c.value
    c = ctypes.c_void_p()
    assert lib.yn_chip_create(handle.h, 20, None, 8, None, ctypes.byref(c)) == 1 and "null argument" in lib.yn_last_error(handle.h).decode()


def test_batch_refusals_launch_nothing(handle):
    from yolo_nano_amd import capi, chips
    lib = capi.load_library()
    cut = chips.ChipExtractor(size=(16, 8), fit="stretch", out="u8", max_chips=8, handle=handle)
    frames = [cc.frame_pixels(70, 61, 47), cc.frame_pixels(71, 64, 64)]
    _, views = upload_frames(frames)
    rows = np.asarray([cc.box(3, 3, 30, 30), cc.box(5, 5, 50, 40), cc.box(1, 1, 9, 9)], np.float32)
    rec, off = torch.from_numpy(rows).cuda(), torch.tensor([0, 1, 2], dtype=torch.int32).cuda()
    outs = Outputs(cut, 2)
    chips_t, index_t, off_t, rect_t = outs.tensors
    ptrs = (ctypes.c_void_p * 2)(views[0].data_ptr(), views[1].data_ptr())
    good_geom = np.asarray([cc.geometry(61, 47, 96), cc.geometry(64, 64, 96)], dtype=np.int32)

    def call(B=2, frames_p=ptrs, geom=good_geom, space=0, rec_p=rec.data_ptr(), off_p=off.data_ptr(), cap=3, chips_p=chips_t.data_ptr(),
             index_p=index_t.data_ptr(), rect_p=rect_t.data_ptr(), co_p=off_t.data_ptr()):
        g = None if geom is None else np.ascontiguousarray(geom, dtype=np.int32)
        rc = lib.yn_chip_batch(handle.h, cut.c, B, None if frames_p is None else ctypes.cast(frames_p, ctypes.c_void_p), None if g is None else g.ctypes.data,
                               space, rec_p, off_p, cap, chips_p, index_p, rect_p, co_p)
        return rc, lib.yn_last_error(handle.h).decode()

    def geom_with(b, k, v):
        g = good_geom.copy()
        g[b, k] = v
        return g

    one_null = (ctypes.c_void_p * 2)(views[0].data_ptr(), None)
    refused = [
        (dict(B=-1), "yn_chip_batch: B -1 outside 0..1024"),
        (dict(B=1025), "yn_chip_batch: B 1025 outside 0..1024"),
        (dict(cap=-1), "yn_chip_batch: rec_capacity outside 0..2^31 - 1"),
        (dict(chips_p=chips_t.data_ptr() + 4), "yn_chip_batch: chips_dev is not 16-byte aligned"),
        (dict(co_p=None), "yn_chip_batch: null pointer chip_offsets_dev"),
        (dict(frames_p=None), "yn_chip_batch: null pointer frames_host"),
        (dict(geom=None), "yn_chip_batch: null pointer geom_host"),
        (dict(rec_p=None), "yn_chip_batch: null pointer rec_dev"),
        (dict(off_p=None), "yn_chip_batch: null pointer offsets_dev"),
        (dict(chips_p=None), "yn_chip_batch: null pointer chips_dev"),
        (dict(index_p=None), "yn_chip_batch: null pointer index_dev"),
        (dict(rect_p=None), "yn_chip_batch: null pointer rect_dev"),
        (dict(frames_p=one_null), "yn_chip_batch: null frame pointer for frame 1"),
        (dict(geom=geom_with(1, 0, 0)), "yn_chip_batch: frame 1 is 0x64, sides must be 1..16384"),
        (dict(geom=geom_with(0, 1, 16385)), "yn_chip_batch: frame 0 is 61x16385, sides must be 1..16384"),
        (dict(geom=geom_with(1, 6, 0)), "yn_chip_batch: bad letterbox geometry for frame 1"),
        (dict(geom=geom_with(0, 4, 90)), "yn_chip_batch: bad letterbox geometry for frame 0"),
        (dict(space=2), "yn_chip_batch: space 2 is neither YN_DRAW_LETTERBOX nor YN_DRAW_PIXELS"),
        # the order: a limit before a null pointer, a null pointer before the geometry, the geometry before the space
        (dict(B=-1, frames_p=None), "yn_chip_batch: B -1 outside 0..1024"),
        (dict(rec_p=None, geom=geom_with(1, 6, 0)), "yn_chip_batch: null pointer rec_dev"),
        (dict(space=0, geom=geom_with(1, 6, 0)), "yn_chip_batch: bad letterbox geometry for frame 1"),
        (dict(space=2, geom=geom_with(1, 0, 0)), "yn_chip_batch: frame 1 is 0x64, sides must be 1..16384"),
    ]
    for kw, reason in refused:
        rc, msg = call(**kw)
        assert (rc, msg) == (1, reason), (kw, rc, msg)
    rc, msg = lib.yn_chip_batch(handle.h, None, 2, None, None, 0, None, None, 0, None, None, None, None), lib.yn_last_error(handle.h).decode()
    assert rc == 1 and "null object" in msg
    if torch.cuda.device_count() > 1:                           # a handle on another device than the object's
        from yolo_nano_amd import arch
        far = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=torch.device("cuda", (handle.device.index + 1) % torch.cuda.device_count()))
        rc = lib.yn_chip_batch(far.h, cut.c, 2, ctypes.cast(ptrs, ctypes.c_void_p), good_geom.ctypes.data, 0, rec.data_ptr(), off.data_ptr(), 3,
                               chips_t.data_ptr(), index_t.data_ptr(), rect_t.data_ptr(), off_t.data_ptr())
        assert rc == 1 and "the handle is on device" in lib.yn_last_error(far.h).decode()
    torch.cuda.synchronize()
    assert outs.untouched(), "a refused call wrote to an output"
    with pytest.raises(capi.YnError, match="no yn_chip_batch has run"):
        cut.status()
    rc, msg = call(B=0, frames_p=None, geom=None, rec_p=None, off_p=None, cap=0, chips_p=None, index_p=None, rect_p=None)      # B == 0 is no error
    assert rc == 0, msg
    torch.cuda.synchronize()
    chips_h, index_h, off_h, rect_h = outs.host()
    assert off_h[:4].view(np.int32)[0] == 0 and (off_h[4:] == 0xA5).all() and (chips_h == 0xA5).all() and (index_h == 0xA5).all() and (rect_h == 0xA5).all()
    assert cut.status() == {"chips": 0, "skipped": 0, "overflow": 0, "range_mark": False}
    rc, msg = call(space=1)                                     # and the object still works
    assert rc == 0, msg
    assert cut.status()["chips"] == 2
    cut.close()
