"""Oracle (TEST INFRASTRUCTURE ONLY): numpy restatement of the pixel work of TrainTransforms / ColorTransforms
(data/transforms.py:402-442) for one image and its AugParams record: ConvertFromInts, the PhotometricDistort chain, the crop and
mirror of RandomSampleCrop / RandomMirror, Resize (float cv2.resize + letterbox), Normalize and ToTensor.

Pinned to the reference (tests/golden/train_transforms.npz, made by the reference's own classes): the pointwise ops `brightness`,
`contrast`, `saturation`, `hue` and the host sampler's draws and boxes.

PARITY UNPINNED: the two cv2 pieces.  cv2 is not installed where the fixture is made, so `cv2_resize_linear_f32`, `bgr2hsv` and
`hsv2bgr` restate OpenCV 4.5.x's published scalar code instead (modules/imgproc/src/resize.cpp: resize()'s dsize == ssize copy and
its switch to the 2x2 INTER_AREA fast path, `resizeGeneric_` coordinate set-up, `HResizeLinear<float>`, `VResizeLinear<float>`;
color_hsv.simd.hpp: `RGB2HSV_f`, `HSV2RGB_native`).  Whether cv2's SIMD builds of them fuse a multiply and an add is not settled
here; every step below rounds once per float32 operation, as the scalar code does.  The same holds for ValTransforms' 8-bit path
(oracle/preprocess.py).
"""
import numpy as np

F32 = np.float32
FLT_EPSILON = F32(np.finfo(np.float32).eps)
BRIGHTNESS, CONTRAST, CONTRAST_FIRST, SATURATION, HUE = 1, 2, 4, 8, 16


# ---- the reference's pointwise classes, applied with a drawn factor u (float64) as numpy does: float32(u) -----------------------
def brightness(img, u):
    """RandomBrightness (:221-223): image += delta."""
    out = img.copy()
    out += u
    return out


def contrast(img, u):
    """RandomContrast (:208-210): image *= alpha."""
    out = img.copy()
    out *= u
    return out


def saturation(img, u):
    """RandomSaturation (:146-147) on an HSV image: image[:, :, 1] *= u."""
    out = img.copy()
    out[:, :, 1] *= u
    return out


def hue(img, u):
    """RandomHue (:159-162) on an HSV image: += u, then the > 360 wrap, then the < 0 wrap."""
    out = img.copy()
    out[:, :, 0] += u
    out[:, :, 0][out[:, :, 0] > 360.0] -= 360.0
    out[:, :, 0][out[:, :, 0] < 0.0] += 360.0
    return out


# ---- cv2.cvtColor, float32 (UNPINNED restatement) ----------------------------------------------------------------------------
def bgr2hsv(img):
    """COLOR_BGR2HSV on float32: RGB2HSV_f::operator() with bidx 0, hrange 360 (hscale = 360 * (1.f/360.f) = 1.0f)."""
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = r.copy()
    v = np.where(v < g, g, v)
    v = np.where(v < b, b, v)
    vmin = r.copy()
    vmin = np.where(vmin > g, g, vmin)
    vmin = np.where(vmin > b, b, vmin)
    diff = v - vmin
    s = diff / (np.abs(v) + FLT_EPSILON)
    diff = (60.0 / (diff + FLT_EPSILON).astype(np.float64)).astype(F32)        # (float)(60./(diff + FLT_EPSILON)): double division
    h = np.where(v == r, (g - b) * diff, np.where(v == g, (b - r) * diff + F32(120.0), (r - g) * diff + F32(240.0)))
    h = np.where(h < 0, h + F32(360.0), h)
    return np.stack([h, s, v], axis=-1).astype(F32)


def hsv2bgr(img):
    """COLOR_HSV2BGR on float32: HSV2RGB_native with hscale = 6.f/360.f: s == 0 -> grey; fmod 6, cvFloor, the sector table."""
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    hh = np.fmod(h * (F32(6.0) / F32(360.0)), F32(6.0))
    sector = np.trunc(hh).astype(np.int64)
    sector = sector - (sector > hh)                                          # cvFloor: (int)x - ((int)x > x)
    hh = hh - sector.astype(F32)
    bad = (sector < 0) | (sector >= 6)                                       # (unsigned)sector >= 6u
    sector = np.where(bad, 0, sector)
    hh = np.where(bad, F32(0.0), hh)
    one = F32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * hh), v * (one - s * (one - hh))], axis=-1)
    table = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    idx = table[sector]                                                      # (b, g, r) index into tab
    out = np.take_along_axis(tab, idx, axis=-1)
    grey = (s == 0)[..., None]
    return np.where(grey, v[..., None], out).astype(F32)


def photometric(img, flags, u):
    """PhotometricDistort (:363-370) with the drawn flags and factors u = (brightness, contrast, saturation, hue)."""
    img = img.astype(F32)
    if flags & BRIGHTNESS:
        img = brightness(img, u[0])
    if flags & CONTRAST and flags & CONTRAST_FIRST:
        img = contrast(img, u[1])
    img = bgr2hsv(img)
    if flags & SATURATION:
        img = saturation(img, u[2])
    if flags & HUE:
        img = hue(img, u[3])
    img = hsv2bgr(img)
    if flags & CONTRAST and not flags & CONTRAST_FIRST:
        img = contrast(img, u[1])
    return img


# ---- cv2.resize, float32, INTER_LINEAR (UNPINNED restatement) ---------------------------------------------------------------
def _axis(src, dst):
    """resizeGeneric_ set-up for one axis: fx = (float)((dx+0.5)*scale - 0.5), sx = cvFloor(fx), fx -= sx."""
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    return s, f - s.astype(F32)


def cv2_resize_linear_f32(img, dsize):
    """cv2.resize(img, dsize) for a float32 HxWxC image; dsize = (width, height)."""
    img = np.ascontiguousarray(img, dtype=F32)
    sh, sw = img.shape[:2]
    dw, dh = int(dsize[0]), int(dsize[1])
    if (dw, dh) == (sw, sh):                                                 # resize(): dsize == ssize -> copy
        return img.copy()
    scale_x, scale_y = 1.0 / (dw / sw), 1.0 / (dh / sh)
    isx, isy = int(np.rint(scale_x)), int(np.rint(scale_y))
    eps = np.finfo(np.float64).eps
    if abs(scale_x - isx) < eps and abs(scale_y - isy) < eps and isx == 2 and isy == 2:
        # INTER_LINEAR with an exact 2:1 reduction -> resizeAreaFast_: sum = 0; sum += S0 + S1 + S2 + S3; D = sum * (1.f/4)
        v = img[:2 * dh, :2 * dw]
        s = F32(0.0) + (((v[0::2, 0::2] + v[0::2, 1::2]) + v[1::2, 0::2]) + v[1::2, 1::2])
        return (s * F32(0.25)).astype(F32)
    sx, fx = _axis(sw, dw)
    lo = sx < 0                                                              # xmin border: sx = 0, fx = 0 (alpha 1, 0)
    sx = np.where(lo, 0, sx)
    fx = np.where(lo, F32(0.0), fx)
    hi = sx + 1 >= sw                                                        # dx >= xmax: D = S[sw - 1] * ONE
    sx = np.where(hi, sw - 1, sx)
    fx = np.where(hi, F32(0.0), fx)
    a0, a1 = (F32(1.0) - fx)[None, :, None], fx[None, :, None]
    sx1 = np.minimum(sx + 1, sw - 1)
    hrow = np.where(hi[None, :, None], img[:, sx, :], img[:, sx, :] * a0 + img[:, sx1, :] * a1)    # HResizeLinear<float>
    sy, fy = _axis(sh, dh)
    b0, b1 = (F32(1.0) - fy)[:, None, None], fy[:, None, None]               # y weights kept, source rows clipped instead
    r0, r1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    return (hrow[r0] * b0 + hrow[r1] * b1).astype(F32)                       # VResizeLinear<float>


# ---- the whole pixel pipeline for one record ----------------------------------------------------------------------------------
def train_pixels(frame, geom, photo, size, mean=(0.406, 0.456, 0.485), std=(0.225, 0.224, 0.229)):
    """uint8 HxWx3 BGR frame + AugParams rows -> float32 [3,size,size] RGB, as the reference's TrainTransforms pipeline makes it."""
    h0, w0, x, y, cw, ch, mirror, rw, rh, left, top, flags = [int(v) for v in geom]
    assert frame.shape[:2] == (h0, w0)
    u = [float(v) for v in photo[:4]]                                        # float32(u) already: a Python float acts as float32
    img = photometric(frame[y:y + ch, x:x + cw].astype(F32), flags, u)       # pointwise: cropping first changes nothing
    if mirror:
        img = img[:, ::-1]
    pad = np.array([v * 255 for v in mean])                                  # Resize.mean: float64
    if ch == cw:
        canvas = img if ch == size else cv2_resize_linear_f32(img, (size, size))
    else:
        canvas = np.ones([size, size, 3]) * pad
        canvas[top:top + rh, left:left + rw, :] = cv2_resize_linear_f32(img, (rw, rh))
    out = canvas.astype(F32)                                                 # Normalize
    out /= 255.
    out -= np.array(mean, dtype=F32)
    out /= np.array(std, dtype=F32)
    out = out[..., (2, 1, 0)]                                                # ToTensor
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1)))
