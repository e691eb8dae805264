"""Batched test-time augmentation on the device (yn_tta_*, yn_resize_batch; kernels_tta.hip) against the host restatement
tests/tta_oracle.py and oracle.tta_merge, bit for bit.

Shapes: the model of test_tta_shim_loop (1.0x, C = 20, 160 x 160, conf 0.05), scales 128 / 160 / 192 (down, copy, up), three images
with different content.  Every forward is compared with yn_infer on the IDENTICAL six-image batch (the oracle's resized and mirrored
inputs, uploaded), so nothing is assumed about results across batch sizes."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from yolo_nano_amd import arch, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_oracle as to  # noqa: E402

pytestmark = pytest.mark.gpu

S, C, B = 160, 20, 3
SCALES = [128, 160, 192]
CAP = 2 * sum(3 * ((s // 8) ** 2 + (s // 16) ** 2 + (s // 32) ** 2) for s in SCALES)      # every candidate of every forward kept: 9702 rows
NMS = 0.4


def _model(conf):
    import yolo_nano_amd
    model = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, trainable=False, conf_thresh=conf, nms_thresh=0.5,
                                   anchor_size=arch.MULTI_ANCHOR_SIZE, backbone="1.0x")
    model.load_state_dict({k: torch.as_tensor(v) for k, v in weights.make_state_dict("1.0x", C).items()}, strict=False)
    return model.to("cuda").eval()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the resize kernel on its own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S0", [160, 96, 64])
def test_resize_batch_equals_the_oracle_bit_for_bit(S0):
    """Every (s, B, flip) of the issue's grid plus widths that are no multiple of 4 (50, 97: the scalar store path and its tail) and
    a 4-byte-offset output (the vector path must not be taken on it)."""
    from yolo_nano_amd import capi
    h = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=1)
    x = np.random.default_rng(S0).standard_normal((3, 3, S0, S0)).astype(np.float32)
    x[0, 0, 0, :2] = [-0.0, 0.0]
    xd = torch.from_numpy(x).cuda()
    special = x[:1].copy()                                       # s == S0 copies the bits: 1 * a + 0 * b would not keep these
    special[0, 1, 2, :4] = [-0.0, np.inf, -np.inf, np.nan]
    for flip in (False, True):
        got = h.resize_batch(torch.from_numpy(special).cuda(), S0, flip_pairs=flip).cpu().numpy()
        assert np.array_equal(_bits(got[0]), _bits(special[0])) and (not flip or np.array_equal(_bits(got[1]), _bits(special[0][..., ::-1])))
    for s in (32, 64, 100, 128, 160, 192, 224, 50, 97):
        want = to.resize(x, s)
        pairs = to.flip_pairs(want)
        for nb in (1, 3):
            got = h.resize_batch(xd[:nb], s).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want[:nb])), (S0, s, nb, "plain")
            got = h.resize_batch(xd[:nb], s, flip_pairs=True).cpu().numpy()
            assert got.shape == (2 * nb, 3, s, s)
            assert np.array_equal(_bits(got), _bits(pairs[:2 * nb])), (S0, s, nb, "pairs")
        odd = torch.zeros(6 * 3 * s * s + 1, dtype=torch.float32, device="cuda")[1:].view(6, 3, s, s)
        h.resize_batch(xd, s, flip_pairs=True, out=odd)
        assert np.array_equal(_bits(odd.cpu().numpy()), _bits(pairs)), (S0, s, "offset output")
    assert h.resize_batch(xd[:0], 64).shape == (0, 3, 64, 64)   # B == 0 is not an error
    h.close()


def test_resize_batch_torch_level_helper():
    import yolo_nano_amd
    x = np.random.default_rng(5).standard_normal((2, 3, 96, 96)).astype(np.float32)
    got = yolo_nano_amd.resize_batch(torch.from_numpy(x).cuda(), 128)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(to.resize(x, 128)))
    with pytest.raises(yolo_nano_amd.YnError):
        yolo_nano_amd.resize_batch(torch.from_numpy(x), 128)    # no CPU fallback


# ---- 2-4. forwards, merge, capacity: one model, one reference, shared ----------------------------------------------------------------
class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    """The device run (yn_tta_infer at B = 3) and its reference: per scale yn_infer over the oracle's six-image batch."""
    from yolo_nano_amd import capi
    c = Ctx()
    c.model = _model(0.05)
    c.x = weights.make_input(B, S, seed=4)
    assert not np.array_equal(c.x[0], c.x[1]) and not np.array_equal(c.x[1], c.x[2])
    c.xd = torch.from_numpy(c.x).cuda()
    c.h = c.model.handle(2 * B)
    c.tta = capi.Tta(c.h, SCALES, True, max_batch=B, list_capacity=CAP)
    c.tta.infer(c.xd, NMS)
    assert c.h.S == S                                            # the grid that was set before the call is back
    c.rec, c.off, c.total = [t.cpu().numpy().copy() if isinstance(t, torch.Tensor) else t for t in c.tta.result(total=True)]
    c.lists = c.tta.forwards_to_host(B)
    # reference: per image the six forwards in call order, from yn_infer on the identical batches
    c.per = [[] for _ in range(B)]
    for s in SCALES:
        batch = torch.from_numpy(to.flip_pairs(to.resize(c.x, s))).cuda()
        c.h.set_grid(s)
        boxes, scores, cls, _, count = [t.cpu().numpy() for t in c.h.infer(batch)]
        assert (count >= 0).all()
        for b in range(B):
            for img in (2 * b, 2 * b + 1):
                k = int(count[img])
                c.per[b].append((boxes[img, :k].copy(), scores[img, :k].copy(), cls[img, :k].astype(np.int64)))
    c.h.set_grid(S)
    yield c
    c.tta.close()


def test_forwards_equal_yn_infer_on_the_same_batch(ctx):
    boxes, scores, cls, count, start = ctx.lists
    assert start.shape == (2 * len(SCALES), B)
    for b in range(B):
        lb, ls, ll, lstart = to.build_list(ctx.per[b])           # un-mirrors the odd forwards
        n = len(ls)
        assert n > 0 and int(count[b]) == n <= CAP
        assert np.array_equal(start[:, b], lstart)
        for f in range(2 * len(SCALES)):                         # forward by forward, so that a failure names it
            lo = int(start[f, b])
            hi = int(start[f + 1, b]) if f + 1 < len(start) else n
            assert hi - lo == len(ctx.per[b][f][1]), (b, f)
            assert np.array_equal(_bits(boxes[b, lo:hi]), _bits(lb[lo:hi])), (b, f)
            assert np.array_equal(_bits(scores[b, lo:hi]), _bits(ls[lo:hi])), (b, f)
            assert np.array_equal(cls[b, lo:hi], ll[lo:hi]), (b, f)
        assert (cls[b, n:] == -1).all()                          # the rest of the list is no candidate
    assert len({int(v) for v in count}) > 1                      # different content: different lists


def _check_result(rec, off, total, per):
    assert off.shape == (B + 1,) and off[0] == 0 and int(off[-1]) == total and (np.diff(off) >= 0).all()
    for b in range(B):
        eb, es, el, _ = orc.tta_merge(per[b], C, NMS)
        r = rec[off[b]:off[b + 1]]
        assert len(r) == len(es) > 0, b
        assert np.array_equal(_bits(r[:, :4]), _bits(eb)), b
        assert np.array_equal(_bits(r[:, 4]), _bits(es)), b
        assert np.array_equal(r[:, 5].astype(np.int64), el), b


def test_merge_equals_the_oracle_merge_per_image(ctx):
    _check_result(ctx.rec, ctx.off, ctx.total, ctx.per)


def test_no_candidates_gives_empty_lists():
    """conf_thresh 0.999: nothing passes, every list is empty and every offset is 0."""
    from yolo_nano_amd import capi
    model = _model(0.999)
    h = model.handle(2 * B)
    tta = capi.Tta(h, SCALES, True, max_batch=B, list_capacity=256)
    tta.infer(torch.from_numpy(weights.make_input(B, S, seed=4)).cuda(), NMS)
    rec, off, total = tta.result(total=True)
    assert total == 0 and off.cpu().numpy().tolist() == [0] * (B + 1)
    _, _, cls, count, start = tta.forwards_to_host(B)
    assert (count == 0).all() and (start == 0).all() and (cls == -1).all()
    tta.infer(torch.zeros((0, 3, S, S), device="cuda"), NMS)    # B == 0 is not an error
    assert tta.result(total=True)[2] == 0
    tta.close()


def test_list_capacity_is_enforced_and_named(ctx):
    from yolo_nano_amd import capi
    count = ctx.lists[3]
    cap = int(count.max()) - 1                                   # below the fullest image's real total, enough for a shorter one
    first = int(np.argmax(count > cap))
    small = capi.Tta(ctx.h, SCALES, True, max_batch=B, list_capacity=cap)
    with pytest.raises(capi.YnError) as e:
        small.infer(ctx.xd, NMS)
    assert "image %d needs %d rows" % (first, int(count[first])) in str(e.value) and "list_capacity is %d" % cap in str(e.value)
    with pytest.raises(capi.YnError):
        small.result()                                           # nothing is delivered
    assert ctx.h.S == S                                          # the grid is restored on failure too
    got = small.forwards_to_host(B)[3]
    assert np.array_equal(got, count)                            # the sizes the lists needed
    small.close()
    enough = capi.Tta(ctx.h, SCALES, True, max_batch=B, list_capacity=int(count.max()))
    enough.infer(ctx.xd, NMS)
    rec, off, total = enough.result(total=True)
    _check_result(rec.cpu().numpy(), off.cpu().numpy(), total, ctx.per)
    enough.close()


def test_handle_too_small_is_refused_by_name():
    from yolo_nano_amd import capi
    model = _model(0.05)
    h = model.handle(2)                                          # room for one image and its mirror
    tta = capi.Tta(h, SCALES, True, max_batch=B, list_capacity=64)
    with pytest.raises(capi.YnError, match="max_batch >= 6"):
        tta.infer(torch.from_numpy(weights.make_input(B, S, seed=4)).cuda(), NMS)
    tta.close()


# ---- 5. the shim -----------------------------------------------------------------------------------------------------------------
def test_shim_batch_records_and_evaluate(ctx):
    import yolo_nano_amd
    from yolo_nano_amd import ValTransforms, VOCEval, evaluate, voc_geometry
    model = ctx.model
    tta = yolo_nano_amd.TestTimeAugmentation(num_classes=C, nms_thresh=NMS, scale_range=[128, 192, 32])
    tta.list_capacity = CAP
    x1 = ctx.xd[:1]
    (bb, sc, lb), = tta.batch(x1, model)
    assert model.input_size == S and model.handle().S == S
    rec, off = tta.records(x1, model)
    off = off.cpu().numpy()
    r = rec[: int(off[-1])].cpu().numpy()
    assert off.tolist() == [0, len(sc)] and len(sc) > 0
    assert np.array_equal(_bits(r[:, :4]), _bits(bb)) and np.array_equal(_bits(r[:, 4]), _bits(sc)) and np.array_equal(r[:, 5].astype(np.int64), lb)
    assert bb.dtype == np.float32 and sc.dtype == np.float32 and lb.dtype == np.int64
    # the whole batch through the shim equals the C-ABI run of the fixture
    trip = tta.batch(ctx.xd, model)
    for b in range(B):
        q = ctx.rec[ctx.off[b]:ctx.off[b + 1]]
        assert np.array_equal(_bits(trip[b][0]), _bits(q[:, :4])) and np.array_equal(_bits(trip[b][1]), _bits(q[:, 4]))
    # evaluate(..., test_aug=tta) on three tiny synthetic frames == VOCEval.add_host fed with batch()'s triples
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, shp + (3,), dtype=np.uint8) for shp in ((120, 160), (160, 120), (100, 100))]
    annots = []
    for im in frames:
        h0, w0 = im.shape[:2]
        k = 3
        x1_, y1_ = rng.integers(0, w0 - 50, k), rng.integers(0, h0 - 50, k)
        annots.append(np.stack([x1_, y1_, x1_ + rng.integers(5, 50, k), y1_ + rng.integers(5, 50, k), rng.integers(0, C, k),
                                np.zeros(k, dtype=np.int64)], 1).astype(np.int32).reshape(-1, 6))
    aps, mAP = evaluate(model, frames, annots, batch=32, use_07_metric=True, test_aug=tta)
    assert model.input_size == S
    h = model.handle(2 * len(frames))
    x = ValTransforms(S, handle=h).batch(frames)[0]
    dets = tta.batch(x, model)
    assert sum(len(d[1]) for d in dets) > 0
    ev = VOCEval(C, 0.5, handle=h)
    ev.add_host(dets, [voc_geometry(im.shape[0], im.shape[1], S) for im in frames], annots, handle=h)
    raps, rmAP = ev.compute(True, handle=h)
    ev.close()
    assert np.array_equal(aps, raps) and (mAP == rmAP or (np.isnan(mAP) and np.isnan(rmAP)))
