"""The YOLONano shim's split-f16 range fallback on the routes that deliver records: TestTimeAugmentation.records, SlicedInference.records and the
plain route of voc.evaluate.  (forward_raw / forward / forward_batch: test_gpu_parity.py::test_range_guard_whole_network_and_shim.)

The overflowing model is that test's part (b): 1.0x, S = 128, C = 20, the stem's BatchNorm gain x 3e5 - the stem's output reaches about 2.4e6 on
weights.make_input data AND on preprocessed uint8 frames (both are O(1) inputs), far past 65504, so stage 2 splits an out-of-range activation on
every route.  test_the_routes_overflow shows that through capi alone; then per route: exactly one warning, the model exact afterwards, no warning on
a second call, and results bit-equal to those of a model that was exact before its first forward."""
import warnings

import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu

S, C, GAIN = 128, 20, 3.0e5
MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)


@pytest.fixture(scope="module")
def capi():
    from yolo_nano_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return c


@pytest.fixture(scope="module")
def hot():
    sd = weights.make_state_dict("1.0x", C)
    sd["backbone.conv1.1.weight"] = sd["backbone.conv1.1.weight"] * np.float32(GAIN)
    return sd


def _x():
    return torch.from_numpy(weights.make_input(1, S, seed=4)).cuda()


def _frame():
    return np.random.default_rng(11).integers(0, 256, (160, 128, 3), dtype=np.uint8)


def _eval_frames():
    rng = np.random.default_rng(12)
    return [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((96, 128), (128, 80))]


def _model(hot, exact):
    import yolo_nano_amd
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, anchor_size=arch.MULTI_ANCHOR_SIZE)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in hot.items()})
    m = m.to("cuda").eval()
    m._exact_f32 = exact                                       # the handle is made on the first forward: exact from its first launch
    return m


def _range_warnings(run):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = run()
    return out, sum("split-f16 range" in str(w.message) for w in rec)


def _bits(rec, off):
    off = off.cpu().numpy().copy()
    assert int(off[-1]) > 0, "the overflowing model delivers no rows: the bit comparison would be empty"
    return off, rec[: int(off[-1])].cpu().numpy().view(np.uint32).copy()


def _check_route(hot, run):
    """run(model) -> arrays; the fallback's four statements"""
    m = _model(hot, False)
    first, n1 = _range_warnings(lambda: run(m))
    assert n1 == 1 and m._exact_f32 is True
    second, n2 = _range_warnings(lambda: run(m))
    assert n2 == 0
    e = _model(hot, True)
    want, n3 = _range_warnings(lambda: run(e))
    assert n3 == 0
    for got in (first, second):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_the_routes_overflow(capi, hot):
    """capi alone, split-f16 family: each route's input raises YnRangeError (yn_tta_infer, yn_slice_infer) or marks the counts (yn_infer)."""
    from yolo_nano_amd import ValTransforms, slicing
    h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=2)
    h.load_state_dict(hot); h.fold_bn()
    assert h.range_status() == (False, False)
    t = capi.Tta(h, [S], True, max_batch=1)
    with pytest.raises(capi.YnRangeError):
        t.infer(_x())
    t.close()
    assert h.range_status() == (False, True) and h.range_status() == (False, False)
    frame = torch.from_numpy(_frame()).cuda()
    s = capi.Slice(h, max_frames=1)
    with pytest.raises(capi.YnRangeError):
        s.infer([frame], slicing.tile_table([(160, 128)], S), MEAN, STD)
    s.close()
    assert h.range_status() == (False, True) and h.range_status() == (False, False)
    frames = _eval_frames()
    out = h.infer(ValTransforms(S, handle=h).batch(frames)[0])
    assert int(out[4].min()) < 0                                # (this read synchronises)
    with pytest.raises(capi.YnRangeError):
        h.pack_detections(out)
    assert h.range_status() == (False, True) and h.range_status() == (False, False)
    h.close()


def test_tta_records_fall_back(capi, hot):
    from yolo_nano_amd import TestTimeAugmentation
    x = _x()

    def run(m):
        tta = TestTimeAugmentation(num_classes=C, scale_range=[S, S, 32])
        return _bits(*tta.records(x, m))

    _check_route(hot, run)


def test_sliced_records_fall_back(capi, hot):
    from yolo_nano_amd import SlicedInference
    frame = _frame()

    def run(m):
        rec, off, _ = SlicedInference(tile=S).records([frame], m)
        return _bits(rec, off)

    _check_route(hot, run)


def test_evaluate_falls_back(capi, hot):
    """The ground truth is the exact model's own five best boxes per frame, so that some class has AP > 0 and the comparison carries a metric."""
    from yolo_nano_amd import ValTransforms, evaluate, rescale_boxes
    frames = _eval_frames()
    e, tf, annots = _model(hot, True), ValTransforms(S), []
    for im in frames:
        x, _, _, scale, offset = tf(im)
        b, sc, cl = e(x.unsqueeze(0))
        h0, w0 = im.shape[:2]
        top = np.argsort(-sc, kind="stable")[:5]
        b = np.round(rescale_boxes(b[top].copy(), scale, offset, np.array([[w0, h0, w0, h0]])))
        annots.append(np.column_stack([b, cl[top], np.zeros(len(top))]).astype(np.int32).reshape(-1, 6))

    def run(m):
        aps, mAP = evaluate(m, frames, annots)
        assert np.nanmax(aps) > 0, aps
        return np.asarray(aps, np.float64).view(np.uint64), np.asarray([mAP], np.float64).view(np.uint64)

    _check_route(hot, run)
