"""GPU: mosaic samples on the device (yn_mosaic_transform_batch, mosaic_aug_kernel in kernels_aug.hip) against the numpy pixel oracle
tests/mosaic_oracle.py, BIT FOR BIT.  The host sampler and the oracle's canvas composition are pinned to the reference's load_mosaic by
tests/test_mosaic_cpu.py; the cv2 pieces (8-bit frame resize, float canvas resize, HSV conversions) are the restatements of
oracle/preprocess.py and tests/train_aug_oracle.py and stay unpinned, as their headers say.

Every test in this module fails at the parent commit: `Mosaic` cannot be imported from the package and the library has no
yn_mosaic_transform_batch."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mosaic_oracle as mo                                   # noqa: E402
import train_aug_oracle as tao                               # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)


def _shapes(m):
    """Frame shapes (h0, w0) for mosaic size m that reach every branch of the 8-bit resize: up-scale and down-scale, r == 1 (long
    side == m: pasted unresized), exact 2:1 (long side 2m, both sides even: the area path), nearly 2:1, odd, and thin frames whose
    resized extent is 1 px (2 x (2m - 2) shrinks to m x 1, (m - 3) x 1 grows to m x 1)."""
    return [(375, 500), (500, 375), (37, 53), (53, 37), (129, 95), (61, 200), (9, 4), (4, 9), (m, m - m // 4), (m // 2 + 1, m), (m, m),
            (2 * m, 2 * m - 2 * (m // 8)), (2 * m, 2 * m), (2 * m + 1, 2 * m), (2, 2 * m - 2), (m - 3, 1), (2 * m - 2, 2)]


def _targets(rs, n):
    xy = rs.rand(n, 2) * 0.7
    return np.hstack([xy, np.minimum(xy + 0.05 + rs.rand(n, 2) * 0.3, 1.0), rs.randint(0, 20, (n, 1)).astype(np.float64)]).tolist()


def _make(m, side, n, seed):
    """n seeded mosaics: (Mosaic, frame quads, records).  Mosaics 0 and 1 sit at the two ends of the centre's range (S/2 and 3S/2, which
    random.uniform can return), mosaic 2 has no target in any frame; the others draw their centre."""
    from yolo_nano_amd import ColorTransforms, Mosaic
    mz = Mosaic(m, ColorTransforms(side))
    rs = np.random.RandomState(seed)
    shapes = _shapes(m)
    lo, hi = -((-m) // 2), 2 * m + (-m) // 2
    quads, recs = [], []
    for k in range(n):
        sh = [shapes[(4 * k + j + k // len(shapes)) % len(shapes)] for j in range(4)]
        frames = [mo.frame(int(rs.randint(1 << 30)), h0, w0) for h0, w0 in sh]
        tg = [[] if k == 2 else _targets(rs, int(rs.randint(0, 3))) for _ in range(4)]
        random.seed(seed * 1000 + k)
        np.random.seed(seed * 1000 + k)
        center = {0: (lo, lo), 1: (hi, hi)}.get(k)
        rec, boxes, labels, scale, offset = mz.sample(sh, tg, center=center)
        if k == 2:
            assert boxes.shape == (1, 4) and labels.tolist() == [0.0]          # zeros([1, 5]); RandomMirror turns x into 1.
        quads.append(frames)
        recs.append(rec)
    return mz, quads, recs


def _coverage(recs, m):
    g = np.stack([r.geom for r in recs])
    fr = g[:, :48].reshape(-1, 12)
    flags = g[:, 49]
    assert set(g[:, 48]) == {0, 1}                                                           # mirror on and off
    assert (flags & tao.CONTRAST_FIRST).any() and (~flags & tao.CONTRAST_FIRST).any()        # both photometric branches
    for bit in (tao.BRIGHTNESS, tao.CONTRAST, tao.SATURATION, tao.HUE):
        assert (flags & bit).any() and (~flags & bit).any()
    h0, w0, rw, rh = fr[:, 0], fr[:, 1], fr[:, 2], fr[:, 3]
    copy = (rw == w0) & (rh == h0)
    area = (w0 == 2 * rw) & (h0 == 2 * rh)
    assert copy.any() and area.any() and (rw > w0).any() and ((rw < w0) & ~area).any()
    assert (np.minimum(rw, rh) == 1).any()                                                   # a resized extent of 1 px
    assert ((fr[:, 10] - fr[:, 8] != rw) | (fr[:, 11] - fr[:, 9] != rh)).any()               # a frame only partly on the canvas
    lo, hi = -((-m) // 2), 2 * m + (-m) // 2
    assert tuple(fr[0, 6:8]) == (lo, lo) and tuple(fr[4, 6:8]) == (hi, hi)                   # centres at both ends of the range


def _compare(mz, quads, recs, x, label):
    x = x.cpu().numpy()
    assert x.shape == (len(recs), 3, mz.color_augment.size, mz.color_augment.size)
    for j, r in enumerate(recs):
        ref = mo.mosaic_pixels(quads[j], r.geom, r.photo, mz.img_size, mz.color_augment.size, MEAN, STD)
        np.testing.assert_array_equal(x[j], ref, err_msg="%s mosaic %d geom %s photo %s" % (label, j, r.geom.tolist(), r.photo.tolist()))


# (M, side): the exact-2:1 canvas resize at three sizes (dataset img_size == transform size), a generic pair, a copy pair (2M == side)
@pytest.mark.parametrize("m,side,n", [(64, 64, 48), (416, 416, 16), (608, 608, 16), (320, 416, 16), (32, 64, 32)])
def test_mosaic_equals_oracle(m, side, n):
    mz, quads, recs = _make(m, side, n, seed=m + side)
    _coverage(recs, m)
    x = mz.batch(quads, recs)
    assert x.dtype == torch.float32 and x.is_cuda
    _compare(mz, quads, recs, x, "M %d side %d" % (m, side))


def test_batch_of_37_and_out_slots():
    m = side = 48
    mz, quads, recs = _make(m, side, 37, seed=5)
    xb = mz.batch(quads, recs)                                   # 37 mosaics: three launches (14 + 14 + 9)
    _compare(mz, quads, recs, xb, "37")
    per = xb.cpu().numpy()
    one = mz.batch(quads[20:21], recs[20:21])                   # one at a time gives the same bits
    np.testing.assert_array_equal(one.cpu().numpy()[0], per[20])
    dev = [[torch.as_tensor(f).cuda() for f in q] for q in quads[3:6]]           # frames already on the device
    np.testing.assert_array_equal(mz.batch(dev, recs[3:6]).cpu().numpy(), per[3:6])
    batch = torch.full((5, 3, side, side), float("nan"), device="cuda")
    got = mz.batch(quads[7:9], recs[7:9], out=batch[1:3])
    assert got.data_ptr() == batch[1].data_ptr()
    b = batch.cpu().numpy()
    np.testing.assert_array_equal(b[1:3], per[7:9])
    assert np.isnan(b[[0, 3, 4]]).all()
    assert mz.batch([], []).shape == (0, 3, side, side)


def test_mixed_batch_equals_per_sample_results():
    from yolo_nano_amd import ColorTransforms, Mosaic, MosaicParams, TrainTransforms
    from yolo_nano_amd.augment import collate, sample_item
    s, n_ids = 64, 12
    tf = TrainTransforms(s)
    mz = Mosaic(s, ColorTransforms(s, handle=tf._h()))
    shapes = _shapes(s)[:n_ids]
    frames = [mo.frame(900 + j, *shapes[j]) for j in range(n_ids)]
    rs = np.random.RandomState(2)
    targets = [_targets(rs, j % 3) for j in range(n_ids)]
    random.seed(11)
    np.random.seed(11)
    items = [sample_item(j % n_ids, n_ids, lambda i: (frames[i], targets[i]), tf, mz)[:2] for j in range(40)]
    kinds = [isinstance(r, MosaicParams) for _, r in items]
    assert 8 < sum(kinds) < 32                                   # a real mixture, interleaved
    x = collate(tf, mz, items)
    assert x.shape == (40, 3, s, s)
    got = x.cpu().numpy()
    for k, (f, r) in enumerate(items):
        if kinds[k]:
            ref = mo.mosaic_pixels(f, r.geom, r.photo, s, s, MEAN, STD)
            one = mz.batch([f], [r])
        else:
            ref = tao.train_pixels(f, r.geom, r.photo, s, MEAN, STD)
            one = tf.batch([f], [r])
        np.testing.assert_array_equal(got[k], ref, err_msg="slot %d" % k)
        np.testing.assert_array_equal(one.cpu().numpy()[0], ref)
    out = torch.full((6, 3, s, s), float("nan"), device="cuda")                # neighbouring slots are written in place
    order = [k for k in range(40) if not kinds[k]][:3] + [k for k in range(40) if kinds[k]][:3]
    assert collate(tf, mz, [items[k] for k in order], out=out).data_ptr() == out.data_ptr()
    np.testing.assert_array_equal(out.cpu().numpy(), got[order])
    only = [items[k] for k in range(40) if kinds[k]][:5]
    np.testing.assert_array_equal(collate(tf, mz, only).cpu().numpy(), got[[k for k in range(40) if kinds[k]][:5]])


def test_c_entry_errors():
    from yolo_nano_amd import ColorTransforms, Mosaic, capi
    m, side = 32, 64
    mz = Mosaic(m, ColorTransforms(side))
    hd = mz.color_augment._h()
    imgs = [torch.zeros((24, 32, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
    rec = mz.sample([(24, 32)] * 4, [[], [], [], []], center=(30, 28))[0]
    good = rec.geom.copy()
    good[48] = 0
    photo = rec.photo

    def err(geom, std=(1.0, 1.0, 1.0), size=m):
        with pytest.raises(capi.YnError) as e:
            hd.mosaic_transform_batch(imgs, geom, photo, size, side, (0.0, 0.0, 0.0), std)
        return str(e.value)

    hd.mosaic_transform_batch(imgs, good, photo, m, side, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for k, v in ((12 + 2, 0), (24 + 3, -1)):                                     # rw, rh
        g = good.copy(); g[k] = v
        assert "non-positive extent" in err(g) and "frame %d" % (k // 12) in err(g)
    for k, v in ((4, -1), (12 + 6, 2 * m + 1), (24 + 7, 2 * m + 1), (36 + 5, -2)):
        g = good.copy(); g[k] = v
        assert "canvas rectangle" in err(g) and "mosaic 0 frame %d" % (k // 12) in err(g)
    for k, v in ((8, -1), (12 + 10, 33), (24 + 11, 25), (36 + 9, -1)):
        g = good.copy(); g[k] = v
        assert "source rectangle" in err(g) and "frame %d" % (k // 12) in err(g)
    g = good.copy(); g[36 + 6] -= 1                                              # x2a - x1a != x2b - x1b
    assert "sizes differ" in err(g) and "frame 3" in err(g)
    g = good.copy(); g[7] -= 1
    assert "sizes differ" in err(g) and "frame 0" in err(g)
    g = good.copy(); g[48] = 2
    assert "mirror" in err(g)
    g = good.copy(); g[49] = 64
    assert "flags" in err(g)
    assert "std must be positive" in err(good, std=(1.0, 0.0, 1.0))
    assert "std must be positive" in err(good, std=(float("nan"), 1.0, 1.0))
    assert "canvas rectangle" in err(good, size=m // 2)                            # the same rectangles on a smaller canvas
    two = np.stack([good, good])
    two[1, 12 + 2] = 0
    with pytest.raises(capi.YnError) as e:
        hd.mosaic_transform_batch(imgs + imgs, two, np.stack([photo, photo]), m, side, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert "mosaic 1 frame 1" in str(e.value)
    lib = hd.lib
    mm = (ctypes.c_float * 3)(0, 0, 0)
    ss = (ctypes.c_float * 3)(1, 1, 1)
    out = torch.empty((1, 3, side, side), device="cuda")
    ptrs = (ctypes.c_void_p * 4)(*[im.data_ptr() for im in imgs])
    gp = good.ctypes.data_as(ctypes.c_void_p)
    pp = photo.ctypes.data_as(ctypes.c_void_p)
    assert lib.yn_mosaic_transform_batch(hd.h, 0, None, None, None, m, side, None, None, None) == 0   # empty batch: not an error
    assert lib.yn_mosaic_transform_batch(hd.h, 1, ptrs, gp, pp, m, side, mm, ss, out.data_ptr()) == 0
    assert lib.yn_mosaic_transform_batch(hd.h, 1, ptrs, gp, None, m, side, mm, ss, out.data_ptr()) != 0
    assert b"null pointer" in lib.yn_last_error(hd.h)
    assert lib.yn_mosaic_transform_batch(hd.h, 1, ptrs, gp, pp, m, side, mm, ss, None) != 0
    assert b"null pointer" in lib.yn_last_error(hd.h)
    nul = (ctypes.c_void_p * 4)(imgs[0].data_ptr(), imgs[1].data_ptr(), None, imgs[3].data_ptr())
    assert lib.yn_mosaic_transform_batch(hd.h, 1, nul, gp, pp, m, side, mm, ss, out.data_ptr()) != 0
    assert b"null frame pointer for mosaic 0 frame 2" in lib.yn_last_error(hd.h)
    assert lib.yn_mosaic_transform_batch(hd.h, -1, ptrs, gp, pp, m, side, mm, ss, out.data_ptr()) != 0
    assert lib.yn_mosaic_transform_batch(hd.h, 1, ptrs, gp, pp, 0, side, mm, ss, out.data_ptr()) != 0
    assert lib.yn_mosaic_transform_batch(hd.h, 1, ptrs, gp, pp, m, 0, mm, ss, out.data_ptr()) != 0
    torch.cuda.synchronize()
