"""CPU: the host half of TrainTransforms / ColorTransforms (yolo_nano_amd.augment) against the reference's own classes
(tests/golden/train_transforms.npz, tests/golden/gen_train_transforms.py), and the numpy pixel oracle (tests/train_aug_oracle.py)
that the GPU tests hold the device to: its pointwise ops against the reference bit for bit, its cv2 restatements against
float64 interpolation and the HSV round trip."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_aug_oracle as tao                               # noqa: E402
from oracle import preprocess as pp                          # noqa: E402

FN = {0: "randint", 1: "uniform"}


class DrawLog(object):
    def __init__(self):
        self.rows = []

    def __enter__(self):
        self._orig = {k: getattr(np.random, k) for k in FN.values()}
        for code, k in FN.items():
            setattr(np.random, k, self._wrap(code, self._orig[k]))
        return self

    def __exit__(self, *exc):
        for k, f in self._orig.items():
            setattr(np.random, k, f)

    def _wrap(self, code, f):
        def g(*args):
            v = f(*args)
            a = list(args) + [np.nan] * (2 - len(args))
            self.rows.append((code, float(a[0]), float(a[1]), float(v)))
            return v
        return g


def _cases(g):
    for i in range(len(g["s_seed"])):
        t = g["s_target"][g["s_target_off"][i]:g["s_target_off"][i + 1]]
        yield (i, bool(g["s_crop"][i]), int(g["s_seed"][i]), tuple(int(v) for v in g["s_shape"][i]), t,
               g["s_draws"][g["s_draws_off"][i]:g["s_draws_off"][i + 1]],
               g["s_boxes"][g["s_out_off"][i]:g["s_out_off"][i + 1]], g["s_labels"][g["s_out_off"][i]:g["s_out_off"][i + 1]],
               tuple(int(v) for v in g["s_crop_shape"][i]))


@pytest.mark.parametrize("size", [64, 416, 608])
def test_sampler_consumes_the_reference_draws_and_returns_its_boxes(golden, size):
    from yolo_nano_amd import TrainTransforms, ColorTransforms
    g = golden("train_transforms.npz")
    tfs = {True: TrainTransforms(size), False: ColorTransforms(size)}
    for i, crop, seed, (h0, w0), target, draws, rboxes, rlabels, (ch, cw) in _cases(g):
        t = target.copy()
        np.random.seed(seed)
        with DrawLog() as log:
            rec, boxes, labels, scale, offset = tfs[crop].sample((h0, w0, 3), t[:, :4], t[:, 4])
        got = np.array(log.rows, np.float64).reshape(-1, 4)
        np.testing.assert_array_equal(got, draws, err_msg="case %d: draw sequence" % i)
        np.testing.assert_array_equal(t, target, err_msg="case %d: the caller's target changed" % i)
        geom = rec.geom
        assert tuple(geom[:2]) == (h0, w0) and (int(geom[5]), int(geom[4])) == (ch, cw), i
        rw, rh, left, top, side, rscale, roffset = pp.letterbox_geometry(ch, cw, size)      # Resize's own expressions
        assert side == size and tuple(int(v) for v in geom[7:11]) == (rw, rh, left, top), i
        np.testing.assert_array_equal(np.asarray(scale), np.asarray(rscale))
        np.testing.assert_array_equal(offset, roffset)
        np.testing.assert_array_equal(boxes, rboxes * rscale + roffset, err_msg="case %d: boxes" % i)
        np.testing.assert_array_equal(np.asarray(labels, np.float64), rlabels, err_msg="case %d: labels" % i)
        assert geom.dtype == np.int32 and rec.photo.dtype == np.float32 and rec.photo.shape == (7,)


def test_fixture_covers_every_branch(golden):
    g = golden("train_transforms.npz")
    modes, accepted_after_miss, mirrors, empty_uncropped = set(), 0, set(), 0
    for i, crop, seed, shape, target, draws, rboxes, rlabels, crop_shape in _cases(g):
        six = draws[(draws[:, 0] == 0) & (draws[:, 1] == 6)][:, 3]
        modes.update(int(v) for v in six)
        if crop and not target[:, :4].any():
            empty_uncropped += six[-1] == 0 and tuple(crop_shape) == shape
        mirrors.add(int(draws[-1, 3]))
        if crop and len(six) > 1:
            accepted_after_miss += 1
    assert modes == set(range(6)) and mirrors == {0, 1} and accepted_after_miss > 5
    assert empty_uncropped == sum(1 for c in _cases(g) if c[1] and not c[4][:, :4].any()) > 0


def test_letterbox_matches_val_transforms_geometry():
    from yolo_nano_amd import ValTransforms
    from yolo_nano_amd.augment import letterbox
    for size in (64, 416, 608):
        vt = ValTransforms(size)
        for h0, w0 in [(375, 500), (500, 375), (4, 4), (4, 9), (9, 4), (size, size), (2 * size, 2 * size), (123, 457)]:
            a, b = letterbox(h0, w0, size), vt.geometry(h0, w0)
            assert a[:4] == b[:4]
            np.testing.assert_array_equal(np.asarray(a[4]), np.asarray(b[4]))
            np.testing.assert_array_equal(a[5], b[5])


@pytest.mark.parametrize("name,fn", [("brightness", tao.brightness), ("contrast", tao.contrast), ("saturation", tao.saturation),
                                     ("hue", tao.hue)])
def test_oracle_pointwise_ops_equal_the_reference(golden, name, fn):
    g = golden("train_transforms.npz")
    ins, outs, draws = g["p_%s_in" % name], g["p_%s_out" % name], g["p_%s_draws" % name]
    fired = 0
    for k in range(len(ins)):
        d = draws[k]
        assert d[0, 0] == 0 and d[0, 1] == 2
        if d[0, 3]:
            fired += 1
            got = fn(ins[k], float(d[1, 3]))
        else:
            got = ins[k]
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, outs[k], err_msg="%s case %d" % (name, k))
    assert 0 < fired < len(ins)
    if name == "hue":                                        # both wraps occurred
        hv = [(ins[k][..., 0] + np.float32(draws[k][1, 3])) for k in range(len(ins)) if draws[k][0, 3]]
        assert any((h > 360).any() for h in hv) and any((h < 0).any() for h in hv)


def _bilinear64(img, dw, dh):
    """float64 bilinear interpolation with half-pixel centres and edge clamping; the source coordinates are rounded to float32
    as cv2 stores them (a coordinate error of an ulp times a gradient of hundreds per pixel is not the arithmetic under test)."""
    sh, sw = img.shape[:2]
    fx = np.clip(((np.arange(dw) + 0.5) * (sw / dw) - 0.5).astype(np.float32).astype(np.float64), 0, sw - 1)
    fy = np.clip(((np.arange(dh) + 0.5) * (sh / dh) - 0.5).astype(np.float32).astype(np.float64), 0, sh - 1)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    ax, ay = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    im = img.astype(np.float64)
    top = im[y0][:, x0] * (1 - ax) + im[y0][:, x1] * ax
    bot = im[y1][:, x0] * (1 - ax) + im[y1][:, x1] * ax
    return top * (1 - ay) + bot * ay


def test_oracle_float_resize_against_float64_bilinear():
    rs = np.random.RandomState(11)
    for (sh, sw), (dw, dh) in [((37, 53), (64, 45)), ((375, 500), (416, 312)), ((500, 375), (456, 608)), ((4, 9), (64, 28)),
                               ((9, 4), (28, 64)), ((300, 7), (9, 416)), ((97, 131), (41, 30))]:
        img = (rs.rand(sh, sw, 3) * 600 - 150).astype(np.float32)
        got = tao.cv2_resize_linear_f32(img, (dw, dh))
        ref = _bilinear64(img, dw, dh)
        assert got.shape == (dh, dw, 3) and got.dtype == np.float32
        assert np.abs(got - ref).max() <= 4 * np.spacing(np.float32(450)), (sh, sw, dw, dh)
    img = (rs.rand(20, 30, 3) * 255).astype(np.float32)
    np.testing.assert_array_equal(tao.cv2_resize_linear_f32(img, (30, 20)), img)                    # identity: a copy
    half = tao.cv2_resize_linear_f32(img, (15, 10))                                                   # exact 2:1: the area path
    np.testing.assert_array_equal(half, (((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]) * np.float32(0.25))
    for dsize in [(15, 10), (60, 40), (30, 40), (60, 20)]:                                           # constant input: exact
        c = np.full((20, 30, 3), 77.0, np.float32)
        np.testing.assert_array_equal(tao.cv2_resize_linear_f32(c, dsize), np.full(dsize[::-1] + (3,), 77.0, np.float32))


def test_oracle_hsv_round_trip():
    rs = np.random.RandomState(5)
    img = (rs.rand(64, 64, 3) * 255).astype(np.float32)
    img[:16] = np.round(img[:16])
    img[16:20, :, 1] = img[16:20, :, 0]                                                                # ties: v == r == g etc.
    img[20:24, :, 2] = img[20:24, :, 1]
    back = tao.hsv2bgr(tao.bgr2hsv(img))
    assert back.dtype == np.float32
    ulp = np.spacing(img.max(axis=-1, keepdims=True))
    assert (np.abs(back - img) <= 16 * ulp).all()
    grey = np.repeat(img[..., :1], 3, axis=-1)                                                          # s == 0: exact
    hsv = tao.bgr2hsv(grey)
    assert (hsv[..., 1] == 0).all()
    np.testing.assert_array_equal(tao.hsv2bgr(hsv), grey)
    assert not np.array_equal(back, img)                    # not an identity in float32: the pass always runs


def test_sampler_is_numpy_only():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; from yolo_nano_amd import TrainTransforms; np.random.seed(0); "
            "TrainTransforms(416).sample((375, 500, 3), np.array([[0.1, 0.1, 0.5, 0.5]]), np.array([3.])); "
            "assert 'torch' not in sys.modules, 'the sampler imported torch'")
    subprocess.check_call([sys.executable, "-c", code], cwd=root)
