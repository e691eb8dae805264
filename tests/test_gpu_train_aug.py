"""GPU: TrainTransforms / ColorTransforms on the device (yn_train_transform_batch, kernels_aug.hip) against the numpy pixel oracle
tests/train_aug_oracle.py, BIT FOR BIT.  The oracle's pointwise ops and the host sampler are pinned to the reference by
tests/test_train_aug_cpu.py; its cv2 float resize and HSV conversion are restated and unpinned (the oracle's header says why)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_aug_oracle as tao                               # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(375, 500), (500, 375), (4, 4), (4, 9), (9, 4), (37, 53), (53, 37), (7, 300), (300, 7), (33, 33), (129, 95), (61, 200)]
MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)


def _frame(rs, h0, w0):
    """uint8 BGR noise with rows of the HSV corner cases: grey (s == 0), ties v == r == g and v == g == b, pure red (h = 0, the
    hue wraps below 0) and a red-magenta (h just under 360, the wrap above 360), black and white."""
    f = rs.randint(0, 256, (h0, w0, 3)).astype(np.uint8)
    k = rs.randint(0, 256, (h0, w0)).astype(np.uint8)
    rows = np.arange(h0) % 8
    f[rows == 1] = k[rows == 1][:, :, None]                                      # grey
    f[rows == 2, :, 1] = f[rows == 2, :, 2] = np.maximum(f[rows == 2, :, 1], f[rows == 2, :, 2])     # r == g >= b
    f[rows == 3, :, 0] = f[rows == 3, :, 1] = np.maximum(f[rows == 3, :, 0], f[rows == 3, :, 1])     # b == g: v == g ties
    f[rows == 4] = (0, 0, 255)
    f[rows == 5] = (3, 0, 255)
    f[rows == 6, ::2] = 0
    f[rows == 6, 1::2] = 255
    return f


def _target(rs, n):
    if n == 0:
        return np.zeros([1, 5])
    xy = rs.rand(n, 2) * 0.7
    return np.hstack([xy, np.minimum(xy + 0.05 + rs.rand(n, 2) * 0.3, 1.0), rs.randint(0, 20, (n, 1)).astype(np.float64)])


def _run(tf, seeds, shapes, rs):
    """Sample every seed, run the device in batches of 32, compare each image with the oracle; -> the records (for coverage)."""
    frames, recs = [], []
    for k, seed in enumerate(seeds):
        h0, w0 = shapes[k % len(shapes)]
        f = _frame(rs, h0, w0)
        t = _target(rs, int(rs.randint(0, 4)))
        np.random.seed(seed)
        rec = tf.sample(f.shape, t[:, :4], t[:, 4])[0]
        frames.append(f)
        recs.append(rec)
    for i0 in range(0, len(frames), 32):
        x = tf.batch(frames[i0:i0 + 32], recs[i0:i0 + 32]).cpu().numpy()
        for j in range(x.shape[0]):
            r = recs[i0 + j]
            ref = tao.train_pixels(frames[i0 + j], r.geom, r.photo, tf.size, MEAN, STD)
            np.testing.assert_array_equal(x[j], ref, err_msg="seed %d geom %s photo %s" % (seeds[i0 + j], r.geom.tolist(), r.photo.tolist()))
    return recs


def _coverage(recs, size, crop):
    g = np.stack([r.geom for r in recs])
    p = np.stack([r.photo for r in recs])
    flags = g[:, 11]
    cropped = (g[:, 4] != g[:, 1]) | (g[:, 5] != g[:, 0])
    copy = (g[:, 4] == g[:, 7]) & (g[:, 5] == g[:, 8])
    area = (g[:, 4] == 2 * g[:, 7]) & (g[:, 5] == 2 * g[:, 8])
    assert set(g[:, 6]) == {0, 1}
    assert (flags & tao.CONTRAST_FIRST).any() and (~flags & tao.CONTRAST_FIRST).any()
    for bit in (tao.BRIGHTNESS, tao.CONTRAST, tao.SATURATION, tao.HUE):
        assert (flags & bit).any() and (~flags & bit).any()
    hue = p[(flags & tao.HUE) != 0, 3]
    assert (hue > 0).any() and (hue < 0).any()
    assert (~cropped).any() and (cropped.any() if crop else not cropped.any())
    return copy, area


@pytest.mark.parametrize("size,n", [(64, 384), (416, 128), (608, 96)])
def test_train_transforms_equal_oracle(size, n):
    from yolo_nano_amd import TrainTransforms
    tf = TrainTransforms(size)
    rs = np.random.RandomState(size)
    shapes = SHAPES + [(2 * size, 2 * size), (size, size), (2 * size, 2 * size - 2 * (size // 8))]
    recs = _run(tf, list(range(7000, 7000 + n)), shapes, rs)
    copy, area = _coverage(recs, size, crop=True)
    assert copy.any() and area.any()                         # a crop of side `size` (copied) and an exact 2:1 reduction


@pytest.mark.parametrize("size,n", [(64, 160), (416, 64)])
def test_color_transforms_equal_oracle(size, n):
    from yolo_nano_amd import ColorTransforms
    tf = ColorTransforms(size)
    rs = np.random.RandomState(size + 1)
    recs = _run(tf, list(range(9000, 9000 + n)), SHAPES + [(2 * size, 2 * size), (size, size)], rs)
    copy, area = _coverage(recs, size, crop=False)
    assert copy.any() and area.any()


def test_call_and_batch_of_37_and_out_slots():
    from yolo_nano_amd import TrainTransforms
    size = 96
    tf = TrainTransforms(size)
    rs = np.random.RandomState(3)
    frames = [_frame(rs, *SHAPES[k % len(SHAPES)]) for k in range(37)]
    targets = [_target(rs, 1 + k % 3) for k in range(37)]
    per, outs = [], []
    for k in range(37):
        t = targets[k].copy()
        np.random.seed(100 + k)
        x, boxes, labels, scale, offset = tf(frames[k], t[:, :4], t[:, 4])
        np.testing.assert_array_equal(t, targets[k])            # the caller's array is left alone
        assert x.shape == (3, size, size) and x.dtype == torch.float32 and x.is_cuda
        np.random.seed(100 + k)
        rec, b2, l2, s2, o2 = tf.sample(frames[k].shape, targets[k][:, :4], targets[k][:, 4])
        np.testing.assert_array_equal(boxes, b2)
        np.testing.assert_array_equal(labels, l2)
        per.append(x.cpu().numpy())
        outs.append(rec)
    xb = tf.batch(frames, outs)                                 # 37 images: two launches (32 + 5)
    assert xb.shape == (37, 3, size, size)
    np.testing.assert_array_equal(xb.cpu().numpy(), np.stack(per))
    batch = torch.full((4, 3, size, size), float("nan"), device="cuda")
    np.random.seed(100 + 2)
    t = targets[2].copy()
    x = tf(frames[2], t[:, :4], t[:, 4], out=batch[2])[0]
    assert x.data_ptr() == batch[2].data_ptr()
    got = batch.cpu().numpy()
    np.testing.assert_array_equal(got[2], per[2])
    assert np.isnan(got[[0, 1, 3]]).all()
    tf.batch(frames[5:7], outs[5:7], out=batch[:2])
    np.testing.assert_array_equal(batch[:2].cpu().numpy(), np.stack(per[5:7]))
    assert np.isnan(batch[3].cpu().numpy()).all()
    assert tf.batch([], []).shape == (0, 3, size, size)


def test_end_to_end_step_from_device_augmentation():
    from oracle import targets as otg
    from yolo_nano_amd import TrainTransforms, arch, capi, multi_gt_creator, weights
    S, C, B = 416, 20, 8
    tf = TrainTransforms(S)
    rs = np.random.RandomState(21)
    np.random.seed(2026)
    frames, recs, label_lists = [], [], []
    for k in range(B):
        f = _frame(rs, *[(375, 500), (500, 375), (333, 500), (480, 640)][k % 4])
        t = _target(rs, 1 + k % 4)
        rec, boxes, labels, _, _ = tf.sample(f.shape, t[:, :4], t[:, 4])
        frames.append(f)
        recs.append(rec)
        label_lists.append(np.hstack((boxes, np.expand_dims(labels, axis=1))).tolist())     # data/voc.py:233, train.py:211
    x = tf.batch(frames, recs)
    target = multi_gt_creator(S, [8, 16, 32], label_lists, anchor_size=arch.MULTI_ANCHOR_SIZE)
    ref = otg.multi_gt_creator(S, [8, 16, 32], label_lists, arch.MULTI_ANCHOR_SIZE)
    got = target.cpu().numpy()
    assert got.shape == ref.shape
    for fld in (0, 1, 2, 3, 6, 7, 8, 9, 10):
        np.testing.assert_array_equal(got[..., fld], ref[..., fld], err_msg="field %d" % fld)
    for fld in (4, 5):                                          # log(box / anchor): one float32 ulp (tests/test_gpu_targets.py)
        assert (np.abs(got[..., fld] - ref[..., fld]) <= np.spacing(np.abs(ref[..., fld]).astype(np.float32))).all()
    sd = weights.make_state_dict("1.0x", C)
    h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=B)
    h.load_state_dict(sd)
    h.train_bind()
    losses = h.train_step(x, target, lr=1e-3).cpu().numpy()
    assert losses.shape == (4,) and np.isfinite(losses).all()
    h.close()


def test_c_entry_errors():
    from yolo_nano_amd import TrainTransforms, capi
    tf = TrainTransforms(64)
    hd = tf._h()
    img = torch.zeros((20, 30, 3), dtype=torch.uint8, device="cuda")
    good = np.array([20, 30, 0, 0, 30, 20, 0, 64, 42, 0, 11, 0], np.int32)
    photo = np.zeros(7, np.float32)

    def err(geom, std=(1.0, 1.0, 1.0), side=64):
        with pytest.raises(capi.YnError) as e:
            hd.train_transform_batch([img], geom, photo, side, (0.0, 0.0, 0.0), std)
        return str(e.value)

    hd.train_transform_batch([img], good, photo, 64, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for k, v in ((2, 1), (3, 1), (4, 0), (5, 0), (2, -1)):
        g = good.copy(); g[k] = v
        assert "crop" in err(g) and "outside" in err(g)
    for k, v in ((7, 65), (8, 54), (9, 1), (10, 23), (7, 0)):
        g = good.copy(); g[k] = v
        assert "resized extent" in err(g)
    g = good.copy(); g[11] = 64
    assert "flags" in err(g)
    assert "std must be positive" in err(good, std=(1.0, 0.0, 1.0))
    assert "std must be positive" in err(good, std=(1.0, float("nan"), 1.0))
    lib = hd.lib
    m = (ctypes.c_float * 3)(0, 0, 0)
    s = (ctypes.c_float * 3)(1, 1, 1)
    out = torch.empty((1, 3, 64, 64), device="cuda")
    ptrs = (ctypes.c_void_p * 1)(img.data_ptr())
    gp = good.ctypes.data_as(ctypes.c_void_p)
    pp = photo.ctypes.data_as(ctypes.c_void_p)
    assert lib.yn_train_transform_batch(hd.h, 0, None, None, None, 64, None, None, None) == 0        # empty batch: not an error
    assert lib.yn_train_transform_batch(hd.h, 1, ptrs, gp, None, 64, m, s, out.data_ptr()) != 0
    assert b"null pointer" in lib.yn_last_error(hd.h)
    assert lib.yn_train_transform_batch(hd.h, 1, ptrs, gp, pp, 64, m, s, None) != 0
    assert b"null pointer" in lib.yn_last_error(hd.h)
    nul = (ctypes.c_void_p * 1)(None)
    assert lib.yn_train_transform_batch(hd.h, 1, nul, gp, pp, 64, m, s, out.data_ptr()) != 0
    assert b"null frame pointer" in lib.yn_last_error(hd.h)
    assert lib.yn_train_transform_batch(hd.h, -1, ptrs, gp, pp, 64, m, s, out.data_ptr()) != 0
    torch.cuda.synchronize()
