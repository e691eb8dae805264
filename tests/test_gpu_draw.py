"""Detections painted onto frames on the device (yn_draw_*, yolo_nano_amd.draw) against the scalar oracle (tests/draw_oracle.py).
Every comparison is all bytes equal.  Each frame is a window inside a larger device buffer with 64 guard bytes of 0xA5 on both sides
(and a start that is not dword-aligned for three frames in four); the guard bytes must be unchanged.  The tile is 64 x 16 pixels, a
launch carries 32 frames and the on-chip primitive list holds 256 entries: the shapes below cross each of these."""
import json
import os

import numpy as np
import pytest
import torch

import draw_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64
NAMES = json.load(open(os.path.join(HERE, "golden", "class_names.json")))["voc"]


def colors_for(n, seed=1):
    return [tuple(int(v) for v in c) for c in np.random.RandomState(seed).randint(0, 256, size=(n, 3))]


def make_vis(labels, n_classes, thickness=2, font=None, vis_thresh=0.3):
    from yolo_nano_amd import draw
    if labels is None:                                          # a list of length <= 1: colour (255, 0, 0), no label
        return draw.Visualizer([], num_classes=n_classes, vis_thresh=vis_thresh, thickness=thickness)
    return draw.Visualizer(labels, class_colors=colors_for(len(labels)), vis_thresh=vis_thresh, thickness=thickness, font=font)


class Windows:
    """Host frames uploaded as windows of guarded device buffers."""

    def __init__(self, frames):
        self.bufs, self.views, self.shifts = [], [], []
        for i, f in enumerate(frames):
            n, shift = f.size, i % 4
            buf = torch.full((GUARD + shift + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            buf[GUARD + shift:GUARD + shift + n] = torch.from_numpy(np.ascontiguousarray(f).reshape(-1)).cuda()
            self.bufs.append(buf)
            self.views.append(buf[GUARD + shift:GUARD + shift + n].view(f.shape))
            self.shifts.append(shift)

    def check(self, expected):
        for i, (buf, exp) in enumerate(zip(self.bufs, expected)):
            host = buf.cpu().numpy()
            lo = GUARD + self.shifts[i]
            assert (host[:lo] == 0xA5).all() and (host[lo + exp.size:] == 0xA5).all(), "guard bytes of frame %d were written" % i
            got = host[lo:lo + exp.size].reshape(exp.shape)
            if not np.array_equal(got, exp):
                ys, xs = np.nonzero((got != exp).any(axis=2))
                raise AssertionError("frame %d (%dx%d): %d pixels differ, first at x=%d y=%d: got %s, expected %s" % (
                    i, exp.shape[1], exp.shape[0], len(ys), xs[0], ys[0], got[ys[0], xs[0]], exp[ys[0], xs[0]]))


def pixel_geoms(frames):
    return [(f.shape[1], f.shape[0], 0, 0, 0, 0, 0) for f in frames]


def run(vis, frames, recs, geoms, space, vis_thresh=0.3, check_status=True):
    """Paints `frames` (host arrays) with the per-frame record arrays `recs` on the device and through the oracle; compares."""
    recs = [np.asarray(r, dtype=np.float32).reshape(-1, 6) for r in recs]
    off = np.zeros(len(frames) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in recs])
    rows = np.concatenate(recs + [np.zeros((1, 6), np.float32)])
    win = Windows(frames)
    vis.batch(win.views, torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda(), geoms, pixels=space == orc.PIXELS, vis_thresh=vis_thresh)
    expected, prims, skipped = [], [], 0
    for b, (f, r, g) in enumerate(zip(frames, recs, geoms)):
        img, p, s = orc.draw(f, r, g, space, vis_thresh, vis.colors, vis.labels, vis.font, vis.thickness)
        expected.append(img)
        prims += [(b,) + q for q in p]
        skipped += s
    win.check(expected)
    if check_status:
        st = vis.status()
        assert (st["drawn"], st["skipped"], st["range_mark"]) == (len(prims), skipped, False), (st, len(prims), skipped)
    return expected, prims


def background(rng, w0, h0):
    return rng.randint(0, 256, size=(h0, w0, 3)).astype(np.uint8)


def random_boxes(rng, n, w0, h0, n_classes, low_scores=True):
    x = np.sort(rng.uniform(-12, w0 + 8, size=(n, 2)), axis=1)
    y = np.sort(rng.uniform(-12, h0 + 8, size=(n, 2)), axis=1)
    score = rng.uniform(0.2 if low_scores else 0.31, 1.0, size=n)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1], score, rng.randint(0, n_classes, size=n)], axis=1).astype(np.float32)


@pytest.mark.parametrize("labelled", [False, True])
@pytest.mark.parametrize("thickness", [1, 2, 3, 8])
def test_one_box(thickness, labelled):
    rng = np.random.RandomState(thickness)
    vis = make_vis(NAMES if labelled else None, 20, thickness)
    frames = [background(rng, 40, 30), background(rng, 5, 4)]   # 5x4 is thinner than the band: the hole is empty
    recs = [[[8, 14, 30, 25, 0.87, 1]], [[1, 1, 3, 2, 0.5, 7]]]
    expected, prims = run(vis, frames, recs, pixel_geoms(frames), orc.PIXELS)
    assert len(prims) == 2
    assert not np.array_equal(expected[0], frames[0]) and not np.array_equal(expected[1], frames[1])


def test_order():
    rng = np.random.RandomState(2)
    vis = make_vis(NAMES, 20)
    frame = background(rng, 110, 80)
    # B's bar (rows 24..35 from x = 40) lies over A's right edge (x = 60); C's left edge (x = 50) crosses B's bar: in list order a later
    # bar covers an earlier outline and a later outline covers an earlier bar, in the reversed order the other way round
    recs = np.array([[10, 20, 60, 50, 0.9, 0], [40, 35, 90, 60, 0.8, 1], [50, 28, 80, 70, 0.7, 2]], np.float32)
    fwd = orc.draw(frame, recs, None, orc.PIXELS, 0.3, vis.colors, vis.labels, vis.font, 2)[0]
    rev = orc.draw(frame, recs[::-1], None, orc.PIXELS, 0.3, vis.colors, vis.labels, vis.font, 2)[0]
    assert not np.array_equal(fwd, rev), "the case cannot tell the order apart"
    run(vis, [frame, frame], [recs, recs[::-1]], pixel_geoms([frame, frame]), orc.PIXELS)


def test_clipping():
    rng = np.random.RandomState(3)
    vis = make_vis(NAMES, 20, thickness=3)
    frame, dot = background(rng, 48, 40), background(rng, 1, 1)
    boxes = [(-10, 5, 20, 30), (30, 5, 60, 30), (5, -8, 30, 20), (5, 25, 30, 55),            # partly outside, each side
             (-50, 5, -20, 30), (60, 5, 90, 30), (5, -60, 30, -30), (5, 70, 30, 100),        # wholly outside, each side
             (20, 3, 47, 12), (20, 10, 48, 20),                                               # a bar above row 0; x2 >= w0
             (0, 0, 47, 39), (-5, -5, 60, 60),                                                # the whole frame, and more
             (-0.5, -0.5, 10.7, 10.2), (-3.9, 12.5, -0.2, 20.0), (-2000000.0, -2000000.0, 2000000.0, 2000000.0)]
    recs = np.array([b + (0.5 + 0.03 * i, i % 20) for i, b in enumerate(boxes)], np.float32)
    frames = [frame] + [frame.copy() for _ in boxes] + [dot, dot]
    per_frame = [recs] + [recs[i:i + 1] for i in range(len(boxes))] + [[[0, 0, 0, 0, 0.9, 3]], [[-3, -3, 5, 5, 0.9, 4]]]
    run(vis, frames, per_frame, pixel_geoms(frames), orc.PIXELS)


def test_tile_edges_and_alignment():
    rng = np.random.RandomState(4)
    vis = make_vis(NAMES, 20)
    shapes = [(w0, h0) for w0 in (1, 2, 3, 63, 64, 65, 66, 67, 129) for h0 in (1, 15, 16, 17, 33)]
    assert {w0 * 3 % 4 for w0, _ in shapes} == {0, 1, 2, 3}
    frames = [background(rng, w0, h0) for w0, h0 in shapes]    # 45 frames: two launches of the 32-frame descriptor block
    recs = [random_boxes(rng, 50, w0, h0, 20) for w0, h0 in shapes]
    run(vis, frames, recs, pixel_geoms(frames), orc.PIXELS)


def test_hole_is_left_alone():
    rng = np.random.RandomState(5)
    vis = make_vis(None, 3)
    frame = background(rng, 257, 130)
    expected, _ = run(vis, [frame], [[[0, 0, 256, 129, 0.9, 2]]], pixel_geoms([frame]), orc.PIXELS)
    assert np.array_equal(expected[0][1:129, 1:256], frame[1:129, 1:256])
    assert (expected[0][0] == vis.colors[2]).all() and (expected[0][:, 256] == vis.colors[2]).all()


def test_batch_and_status():
    from yolo_nano_amd import voc_geometry
    rng = np.random.RandomState(6)
    vis = make_vis(NAMES, 20)
    shapes = [(70, 50), (33, 20), (64, 16), (100, 37), (20, 90)]
    frames = [background(rng, w0, h0) for w0, h0 in shapes]
    geoms = [voc_geometry(h0, w0, 128) for w0, h0 in shapes]
    thr = np.float32(0.3)
    norm = lambda n: np.sort(rng.uniform(0.05, 0.95, size=(n, 2, 2)), axis=1).reshape(n, 4)     # x1, y1, x2, y2 in the letterboxed square
    ok = np.concatenate([norm(4), rng.uniform(0.4, 1.0, size=(4, 1)), rng.randint(0, 20, size=(4, 1))], axis=1)
    low = np.concatenate([norm(3), rng.uniform(0.0, 0.29, size=(3, 1)), rng.randint(0, 20, size=(3, 1))], axis=1)
    edge = np.concatenate([norm(3), [[thr], [np.nextafter(thr, np.float32(1))], [0.8]], [[1], [2], [3]]], axis=1)
    b = norm(9)
    bad = np.concatenate([b, np.full((9, 1), 0.9), np.full((9, 1), 5.0)], axis=1).astype(np.float32)
    bad[0, 5], bad[1, 5], bad[2, 5], bad[3, 5] = 20, 1.5, -1, np.nan       # class: past the end, no integer, negative, NaN
    bad[4, 0], bad[5, 2], bad[6, 1] = np.nan, np.inf, 1e12                 # coordinates: NaN, infinite, |v| >= 2^30
    bad[7, 4] = 1.2                                                        # digits: k = 120
    bad[8, 4] = np.nan                                                     # a NaN score is not drawn and not counted
    recs = [ok, np.zeros((0, 6)), low, edge, np.concatenate([bad, ok[:1]])]
    _, prims = run(vis, frames, recs, geoms, orc.LETTERBOX, vis_thresh=float(thr))
    assert [p[0] for p in prims] == [0, 0, 0, 0, 3, 3, 4]
    assert vis.status() == {"drawn": 7, "skipped": 8, "range_mark": False}


def test_primitives_and_score_digits():
    from yolo_nano_amd import voc_geometry
    rng = np.random.RandomState(7)
    vis = make_vis(None, 20)
    scores = np.concatenate([(np.arange(201) / 200.0), rng.uniform(0, 1, size=1799)]).astype(np.float32)
    rng.shuffle(scores)
    shapes = [(100, 75), (60, 90), (64, 64)]
    frames = [background(rng, w0, h0) for w0, h0 in shapes]
    geoms = [voc_geometry(h0, w0, 128) for w0, h0 in shapes]
    counts = [334, 333, 333]
    recs, at = [], 0
    for n in counts:
        box = rng.uniform(-0.2, 1.2, size=(n, 4))
        recs.append(np.concatenate([box, scores[at:at + n, None], rng.randint(0, 20, size=(n, 1))], axis=1).astype(np.float32))
        at += n
    win = Windows(frames)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    vis.batch(win.views, torch.from_numpy(np.concatenate(recs)).cuda(), torch.from_numpy(off).cuda(), geoms, vis_thresh=-1.0)
    want = [(b,) + p for b in range(3) for p in orc.select(recs[b], geoms[b], orc.LETTERBOX, -1.0, 20)[0]]
    got = vis.prims()
    assert len(want) == 1000 and got.tolist() == [list(p) for p in want]
    ks = set(got[:, 6].tolist())
    # pixel mode: negative and fractional coordinates
    frame = background(rng, 90, 70)
    box = np.round(rng.uniform(-40, 130, size=(1000, 4)) * 4) / 4
    box[::7] = rng.uniform(-0.99, 0.99, size=box[::7].shape)   # int() takes these to 0 from either side
    rec = np.concatenate([box, scores[1000:, None], rng.randint(0, 20, size=(1000, 1))], axis=1).astype(np.float32)
    win = Windows([frame])
    vis.batch(win.views, torch.from_numpy(rec).cuda(), torch.tensor([0, 1000], dtype=torch.int32).cuda(), None, pixels=True, vis_thresh=-1.0)
    want = [(0,) + p for p in orc.select(rec, None, orc.PIXELS, -1.0, 20)[0]]
    got = vis.prims()
    assert len(want) == 1000 and got.tolist() == [list(p) for p in want]
    assert sorted(ks | set(got[:, 6].tolist())) == list(range(101))
    assert (got[:, 2:6] < 0).any()


def test_long_list_is_chunked_in_order():
    rng = np.random.RandomState(8)
    font = rng.randint(0, 256, size=(95, 5, 4)).astype(np.uint8)
    vis = make_vis(["a", "b", "c"], 3, thickness=1, font=font)
    frame = background(rng, 128, 96)
    n = 3000                                                    # twelve chunks of the 256-entry list
    x1, y1 = rng.randint(-4, 126, size=n), rng.randint(-4, 94, size=n)
    rec = np.stack([x1, y1, x1 + rng.randint(0, 12, size=n), y1 + rng.randint(0, 9, size=n), rng.uniform(0.31, 1.0, size=n), rng.randint(0, 3, size=n)], axis=1)
    _, prims = run(vis, [frame], [rec], pixel_geoms([frame]), orc.PIXELS)
    assert len(prims) == n


def test_blending():
    rng = np.random.RandomState(9)
    font = rng.randint(0, 256, size=(95, 9, 7)).astype(np.uint8)
    font[:, 0, 0], font[:, 0, 1] = 0, 255
    vis = make_vis(NAMES, 20, font=font)
    frame = background(rng, 150, 60)
    rec = random_boxes(rng, 8, 150, 60, 20, low_scores=False)
    rec[:, 1] = np.abs(rec[:, 1]) + 12                          # the bars are inside the frame
    rec[:, 3] = np.maximum(rec[:, 3], rec[:, 1] + 3)
    expected, prims = run(vis, [frame], [rec], pixel_geoms([frame]), orc.PIXELS)
    assert len(prims) == 8
    shades = {tuple(p) for p in expected[0].reshape(-1, 3)} - {tuple(p) for p in frame.reshape(-1, 3)} - {tuple(c) for c in vis.colors}
    assert len(shades) > 50, "no blended pixel in the picture"


def test_range_mark_draws_nothing():
    rng = np.random.RandomState(10)
    vis = make_vis(NAMES, 20)
    frames = [background(rng, 70, 40), background(rng, 30, 50)]
    rec = np.concatenate([random_boxes(rng, 5, 70, 40, 20, False), random_boxes(rng, 5, 30, 50, 20, False)])
    win = Windows(frames)
    vis.batch(win.views, torch.from_numpy(rec).cuda(), torch.tensor([0, 5, -1], dtype=torch.int32).cuda(), None, pixels=True)
    win.check(frames)
    assert vis.status() == {"drawn": 0, "skipped": 0, "range_mark": True}
    vis.batch(win.views, torch.from_numpy(rec).cuda(), torch.tensor([0, 5, 10], dtype=torch.int32).cuda(), None, pixels=True)
    st = vis.status()
    assert st["drawn"] == 10 and not st["range_mark"]


def test_refusals_name_the_frame_or_class():
    from yolo_nano_amd import capi, draw
    with pytest.raises(capi.YnError, match="class 1"):
        draw.Visualizer(["ok", "x" * 33], class_colors=colors_for(2))
    with pytest.raises(capi.YnError, match="thickness"):
        draw.Visualizer(NAMES, thickness=9)
    with pytest.raises(capi.YnError, match="glyph cell"):
        draw.Visualizer(NAMES, font=np.zeros((95, 3, 6), np.uint8))
    vis = make_vis(NAMES, 20)
    buf = torch.zeros((40, 30, 3), dtype=torch.uint8, device="cuda")
    rec, off = torch.zeros((4, 6), device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.YnError, match="frames 0 and 1"):
        vis.batch([buf, buf], rec, off, None, pixels=True)
    with pytest.raises(capi.YnError, match="frame 1"):
        vis.batch([buf, torch.zeros((20, 30, 3), dtype=torch.uint8, device="cuda")], rec, off, [(30, 40, 30, 40, 0, 0, 40), (30, 20, 0, 20, 0, 0, 40)])
    vis.batch([], rec, off[:1], None, pixels=True)              # B == 0 is not an error
    assert vis.status() == {"drawn": 0, "skipped": 0, "range_mark": False}
    assert (buf == 0).all()


def test_end_to_end():
    import yolo_nano_amd
    from yolo_nano_amd import arch, weights, ValTransforms, rescale_boxes, voc_geometry
    S, C = 128, 20
    sd = weights.make_state_dict("1.0x", C)
    for hd in (1, 2, 3):                                        # YOLONano.init_bias (models/yolo_nano.py:77-83)
        sd["head_det_%d.4.bias" % hd][:3] = -4.595
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, conf_thresh=0.001, nms_thresh=0.5, anchor_size=arch.MULTI_ANCHOR_SIZE)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to("cuda").eval()
    rng = np.random.RandomState(11)
    images = [background(rng, 90, 60), background(rng, 50, 80)]
    h = m.handle(2)
    x, scales, offsets = ValTransforms(S, handle=h).batch(images)
    out = h.infer(x)
    rec, off = h.pack_detections(out)
    dets = h.detections_to_host(out)
    all_scores = np.concatenate([d[1] for d in dets])
    assert len(all_scores) >= 2
    thr = float(np.median(all_scores))
    vis = yolo_nano_amd.Visualizer(NAMES, yolo_nano_amd.class_colors(C), vis_thresh=thr, handle=h)
    win = Windows(images)
    vis.batch(win.views, rec, off, [voc_geometry(im.shape[0], im.shape[1], S) for im in images])
    expected, drawn, rows_of = [], 0, []
    for im, (bb, sc, cl), scale, offset in zip(images, dets, scales, offsets):
        px = rescale_boxes(bb, scale, offset, np.array([[im.shape[1], im.shape[0], im.shape[1], im.shape[0]]]))
        rows = np.concatenate([px, sc[:, None], cl[:, None].astype(np.float32)], axis=1).astype(np.float32)
        img, p, s = orc.draw(im, rows, None, orc.PIXELS, thr, vis.colors, vis.labels, vis.font, vis.thickness)
        assert s == 0
        expected.append(img)
        rows_of.append(rows)
        drawn += len(p)
    assert 1 <= drawn < len(all_scores)
    win.check(expected)
    assert vis.status() == {"drawn": drawn, "skipped": 0, "range_mark": False}
    # the reference's visualize() signature: one host frame, boxes in its pixels
    keep = images[0].copy()
    painted = vis(images[0], rows_of[0][:, :4], rows_of[0][:, 4], rows_of[0][:, 5])
    assert np.array_equal(painted, expected[0]) and np.array_equal(images[0], keep)
