"""Lifetime of the library's device memory (csrc/yn_devbuf.h) on the GPU: a handle that regrows its buffers computes what a fresh one
does, the evaluators' stores keep their records across a growth, and destroying every kind of object gives every block back
(yn_live_device_memory: the library's own count - a card's free memory is shared with other processes and cannot show that).

Shapes: 0.5x backbone, 64 x 64 input (as tests/golden/net_05x_coco64_b2.npz), 5 classes, random weights.  No allocation is made to
fail here: the failure paths are driven on the host (tests/test_devbuf_cpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu
C = 5
BACKBONE = "0.5x"


def _live():
    from yolo_nano_amd import capi
    blocks, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert capi.load_library().yn_live_device_memory(ctypes.byref(blocks), ctypes.byref(nbytes)) == 0
    return blocks.value, nbytes.value


@pytest.fixture(autouse=True)
def own_stream():
    """every handle here is made on (and every tensor read on) a stream of the test's own: the default stream cannot be captured"""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        yield
    st.synchronize()


@pytest.fixture(scope="module")
def state_dict():
    return weights.make_state_dict(BACKBONE, C)


def _net(sd, S, max_batch):
    from yolo_nano_amd import capi
    h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, BACKBONE, max_batch=max_batch)
    h.load_state_dict(sd)
    h.fold_bn()
    h.use_graph(True)
    return h


def _kept(out):
    """the kept rows of every image of one yn_infer, as host arrays"""
    boxes, scores, cls, index, count = [t.cpu().numpy() for t in out]
    assert (count >= 0).all()
    return [(int(n), boxes[b, :n].copy(), scores[b, :n].copy(), cls[b, :n].copy(), index[b, :n].copy()) for b, n in enumerate(count)]


def _same_rows(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(x[1:], y[1:]))
                                    for x, y in zip(a, b))


SHAPES = [(64, 1), (64, 3), (96, 2), (64, 1)]


def _infer_shapes(h):
    """yn_infer at every shape of SHAPES on one handle, twice each (the second run replays the graph the first one captured)"""
    res = []
    for S, B in SHAPES:
        h.set_grid(S)
        x = torch.from_numpy(weights.make_input(B, S, seed=3)).cuda()
        first = _kept(h.infer(x))
        assert _same_rows(_kept(h.infer(x)), first)
        res.append(first)
    return res


def test_regrown_handle_computes_what_a_fresh_one_does(state_dict):
    h = _net(state_dict, 64, 3)
    grown = _infer_shapes(h)                                # every growth: arena, heads, candidates, NMS scratch; graphs dropped each time
    h.close()
    assert sum(r[0] for r in grown[1]) > 0                  # random weights at conf 0.001: there are detections to compare
    for (S, B), got in zip(SHAPES, grown):
        f = _net(state_dict, S, B)
        want = _kept(f.infer(torch.from_numpy(weights.make_input(B, S, seed=3)).cuda()))
        f.close()
        assert _same_rows(got, want), (S, B)


def _bare():
    from yolo_nano_amd import capi
    return capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x")          # only its stream and error plumbing are used


SQUARE = (512, 512, 512, 512, 0, 0, 512)                    # w0, h0, rw, rh, left, top, side: normalised = pixel / 512, exact


def _dets(rng, n, classes):
    p0 = rng.integers(0, 100, (n, 2)) * 4
    pix = np.concatenate([p0, p0 + rng.integers(1, 25, (n, 2)) * 4], 1)
    return (pix / 512.0).astype(np.float32), (rng.integers(1, 1001, n) / 1000.0).astype(np.float32), classes


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_voc_store_across_its_first_capacity():
    """three images of 2 000 records: 6 000 cross the 4 096-record store.  One add per image grows it with 4 000 records inside (the
    re-striding copy of the seven planes); one add of all three sizes it at once."""
    from yolo_nano_amd import VOCEval
    rng = np.random.default_rng(5)
    dets = [_dets(rng, 2000, rng.integers(0, C, 2000)) for _ in range(3)]
    # ground truth: the first eight detections of each image themselves (so that there are matches), none difficult
    gts = [np.concatenate([np.rint(d[0][:8] * 512), d[2][:8, None], np.zeros((8, 1))], 1).astype(np.int32) for d in dets]
    h = _bare()
    res = []
    for bs in (1, 3):
        ev = VOCEval(C, handle=h)
        for s in range(0, 3, bs):
            ev.add_host(dets[s:s + bs], [SQUARE] * bs, gts[s:s + bs])
        assert ev.size() == (6000, 3)
        rec = ev.records()
        ap = [ev.compute(u)[0] for u in (True, False)]
        res.append((rec, ap[0], ap[1], ev.npos.copy(), ev.ndet.copy()))
        ev.close()
    h.close()
    assert res[0][0].shape == (6000, 7) and int(res[0][4].sum()) == 6000 and res[0][1].max() > 0
    assert all(_bits(a) == _bits(b) for a, b in zip(res[0], res[1]))


def test_coco_store_across_its_first_capacity():
    """three images x 5 categories with 120 records each: 100 are kept per list, 1 500 in all, past the 819-detection first store.  One
    add per image grows it with detections inside; one add of all three sizes it at once."""
    from yolo_nano_amd import COCOEval
    rng = np.random.default_rng(6)
    dets = [_dets(rng, 5 * 120, rng.permutation(np.repeat(np.arange(C), 120))) for _ in range(3)]
    gts = []                                                # the first eight detections of each image themselves (so that there are matches), no crowds
    for d in dets:
        p = np.rint(d[0][:8].astype(np.float64) * 512)
        w, hh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
        gts.append(np.stack([p[:, 0], p[:, 1], w, hh, w * hh, d[2][:8].astype(np.float64), np.zeros(8)], 1))
    ids = [30, 10, 20]
    h = _bare()
    res = []
    for bs in (1, 3):
        ev = COCOEval(C, handle=h)
        for s in range(0, 3, bs):
            ev.add_host(dets[s:s + bs], [SQUARE] * bs, ids[s:s + bs], gts[s:s + bs])
        assert ev.size() == (1500, 3)
        ev.compute()
        det, seg, matched, ignored = ev.matches()
        res.append((det, seg, matched, ignored, ev.precision.copy(), ev.recall.copy()))
        ev.close()
    h.close()
    assert res[0][0].shape == (1500, 5) and res[0][2].any() and res[0][4].max() > 0
    assert all(_bits(a) == _bits(b) for a, b in zip(res[0], res[1]))


def _one_of_everything(sd):
    """every kind of long-lived object, used once, then destroyed"""
    from yolo_nano_amd import capi, VOCEval, COCOEval, AnchorKMeans, draw
    rng = np.random.default_rng(7)
    h = _net(sd, 64, 3)
    _infer_shapes(h)
    h.set_grid(64)
    B, N = 2, h.N
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()      # noqa: E731
    target = np.zeros((B, N, 11), np.float32)
    target[:, :4, 0] = 1.0
    target[:, :4, 6] = 1.5
    target[:, :4, 7:9], target[:, :4, 9:11] = 0.25, 0.75
    losses, _ = h.loss(dev(rng.standard_normal((B, N))), dev(rng.standard_normal((B, N, C))), dev(rng.standard_normal((B, N, 4))), dev(target))
    assert np.isfinite(losses.cpu().numpy()).all()
    h.train_bind()
    x = torch.from_numpy(weights.make_input(B, 64, seed=8)).cuda()
    for dt in ("f32", "f16"):
        h.train_precision(dt)
        assert np.isfinite(h.train_step(x, dev(target), lr=1e-4, update=True).cpu().numpy()).all()
    d = _dets(rng, 50, rng.integers(0, C, 50))
    ev = VOCEval(C, handle=h)
    ev.add_host([d], [SQUARE], [None])
    ev.compute()
    co = COCOEval(C, handle=h)
    co.add_host([d], [SQUARE], [1], [None])
    co.compute()
    km = AnchorKMeans(rng.uniform(4, 200, (300, 2)), handle=h)
    km.seed_from([0, 100, 200])
    km.run(1e-6, 10)
    vis = draw.Visualizer([], num_classes=C, vis_thresh=0.0, handle=h)
    frame = torch.zeros((512, 512, 3), dtype=torch.uint8, device="cuda")
    rows = np.concatenate([d[0], d[1][:, None], d[2][:, None].astype(np.float32)], 1).astype(np.float32)
    vis.batch([frame], torch.from_numpy(rows).cuda(), torch.tensor([0, 50], dtype=torch.int32).cuda(), [SQUARE])
    assert vis.status()["drawn"] > 0
    h.fold_bn()
    tta = capi.Tta(h, [64], True, max_batch=1, list_capacity=1024)
    tta.infer(x[:1], 0.5)
    assert tta.result(total=True)[2] >= 0
    held = _live()
    for o in (tta, vis, km, co, ev, h):
        o.close()
    return held


def test_everything_is_given_back(state_dict):
    for cycle in range(2):
        before = _live()
        held = _one_of_everything(state_dict)
        assert held[0] > before[0] + 100 and held[1] > before[1]        # the count sees the objects while they live
        assert _live() == before, cycle
