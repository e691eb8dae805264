"""Oracle (TEST INFRASTRUCTURE ONLY): numpy restatement of the pixel work of a mosaic sample, load_mosaic (data/voc.py:140-211)
followed by ColorTransforms (data/transforms.py:424-442), for four uint8 frames and their MosaicParams record: the float64 canvas
filled with mean * 255, the four 8-bit cv2.resize calls and pastes, then ConvertFromInts, the PhotometricDistort chain on the whole
canvas, RandomMirror, Resize of the square canvas, Normalize and ToTensor.

Pinned to the reference (tests/golden/mosaic.npz, made by the reference's own load_mosaic): the canvas composition - fill, paste
rectangles, order - for the fixture's small sizes, with cv2.resize standing for oracle/preprocess.py's restatement on both sides.

PARITY UNPINNED: the cv2 pieces, exactly as in the two parents - `cv2_resize_linear_u8` (oracle/preprocess.py) for the frames and
`cv2_resize_linear_f32`, `bgr2hsv`, `hsv2bgr` (tests/train_aug_oracle.py) for the canvas.  cv2 is not installed where the fixture
is made; whether its SIMD builds fuse a multiply and an add is not settled here.  This file adds no unpinned arithmetic of its own.
"""
import numpy as np

import train_aug_oracle as tao
from oracle.preprocess import cv2_resize_linear_u8

F32 = np.float32


def frame(seed, h0, w0):
    """A seeded uint8 BGR test frame: noise with rows of the HSV corner cases (grey, channel ties, pure red, black / white)."""
    rs = np.random.RandomState(seed)
    f = rs.randint(0, 256, (h0, w0, 3)).astype(np.uint8)
    k = rs.randint(0, 256, (h0, w0)).astype(np.uint8)
    rows = np.arange(h0) % 8
    f[rows == 1] = k[rows == 1][:, :, None]
    f[rows == 2, :, 1] = f[rows == 2, :, 2] = np.maximum(f[rows == 2, :, 1], f[rows == 2, :, 2])
    f[rows == 3, :, 0] = f[rows == 3, :, 1] = np.maximum(f[rows == 3, :, 0], f[rows == 3, :, 1])
    f[rows == 4] = (0, 0, 255)
    f[rows == 5] = (3, 0, 255)
    f[rows == 6, ::2] = 0
    f[rows == 6, 1::2] = 255
    return f


def canvas(frames, geom, mosaic_size, mean=(0.406, 0.456, 0.485)):
    """load_mosaic's image (:155-187): float64 [2S,2S,3].  geom = MosaicParams.geom (only its 4 x 12 frame part is read)."""
    s = int(mosaic_size)
    fill = np.array([v * 255 for v in mean])
    img = np.ones([s * 2, s * 2, 3], dtype=np.uint8) * fill
    for i in range(4):
        h0, w0, rw, rh, x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b = [int(v) for v in geom[12 * i:12 * i + 12]]
        f = frames[i]
        assert f.dtype == np.uint8 and f.shape == (h0, w0, 3)
        if (rw, rh) != (w0, h0):                              # `if r != 1`; cv2.resize itself copies when dsize == ssize
            f = cv2_resize_linear_u8(f, (rw, rh))
        img[y1a:y2a, x1a:x2a] = f[y1b:y2b, x1b:x2b]
    return img


def mosaic_pixels(frames, geom, photo, mosaic_size, size, mean=(0.406, 0.456, 0.485), std=(0.225, 0.224, 0.229)):
    """Four uint8 frames + MosaicParams rows -> float32 [3,size,size] RGB, as load_mosaic + ColorTransforms make it."""
    mirror, flags = int(geom[48]), int(geom[49])
    u = [float(v) for v in photo[:4]]
    img = canvas(frames, geom, mosaic_size, mean).astype(F32)                 # ConvertFromInts
    img = tao.photometric(img, flags, u)
    if mirror:
        img = img[:, ::-1]
    if 2 * mosaic_size != size:                                              # Resize, square case: h0 == self.size -> image_ = image
        img = tao.cv2_resize_linear_f32(img, (size, size))
    out = img.astype(F32)                                                    # Normalize
    out /= 255.
    out -= np.array(mean, dtype=F32)
    out /= np.array(std, dtype=F32)
    out = out[..., (2, 1, 0)]                                                # ToTensor
    return np.ascontiguousarray(np.transpose(out, (2, 0, 1)))
