"""TrainTransforms / ColorTransforms (data/transforms.py:402-442) with the pixel work on the device.

    x, boxes, labels, scale, offset = TrainTransforms(size)(image, boxes, labels)

The reference runs the whole pipeline per image in DataLoader workers, in float32 numpy and cv2.  No random draw depends on a pixel
value, so the work splits in two:

- `sample(shape, boxes, labels)` (host, numpy only): every `np.random` draw of the reference in its order, and all box arithmetic in
  float64 numpy exactly as the reference does it.  It returns an `AugParams` record (the two rows yn_train_transform_batch takes) plus
  `boxes, labels, scale, offset`.  It touches neither torch nor the GPU, so it runs where the reference drew: in the workers.
- `batch(frames, records)` (device): uploads the uint8 frames and runs one launch per 32 images of kernels_aug.hip, which goes from
  the uint8 frame to the normalised RGB CHW network input in one pass (crop, mirror, photometric chain, cv2's float resize,
  letterbox, Normalize, ToTensor).  The chain is pointwise, so it is applied per resize tap without materialising the image.

Quirks of the reference kept on purpose (DESIGN.md "TrainTransforms on the device" lists them): the reversed interval of
`random.uniform(width - w)`, an IoU test that never rejects (max_iou is always inf), no crop ever accepted for the empty-image target
`zeros([1, 5])` (its box centre is (0, 0)), the crop's width in RandomMirror, no clipping anywhere, the HSV round trip even when no
HSV draw fired, and a letterbox pad of float32(float64(mean) * 255).
"""
from collections import namedtuple

import numpy as np
from numpy import random

# flag bits of the geometry row (include/yolonano_hip.h YN_AUG_*)
BRIGHTNESS, CONTRAST, CONTRAST_FIRST, SATURATION, HUE = 1, 2, 4, 8, 16

# RandomSampleCrop.sample_options (data/transforms.py:245-256)
SAMPLE_OPTIONS = (None, (0.1, None), (0.3, None), (0.7, None), (0.9, None), (None, None))

AugParams = namedtuple("AugParams", "geom photo")
AugParams.__doc__ = """One image's device parameters: geom int32 [12] = h0, w0, crop x, y, w, h, mirror, rw, rh, left, top, flags;
photo float32 [7] = brightness, contrast, saturation, hue (float32 of the float64 draws), letterbox pad B, G, R."""


def letterbox(h0, w0, size):
    """Resize.__call__'s geometry (data/transforms.py:79-116) for an h0 x w0 image: (rw, rh, left, top, scale, offset).
    The same expressions as ValTransforms.geometry, without torch."""
    if h0 > w0:
        r = w0 / h0
        w, h = int(r * size), size
        left = (h - w) // 2
        return w, h, left, 0, np.array([[w / h, 1., w / h, 1.]]), np.array([[left / h, 0., left / h, 0.]])
    if h0 < w0:
        r = h0 / w0
        w, h = size, int(r * size)
        top = (w - h) // 2
        return w, h, 0, top, np.array([1., h / w, 1., h / w]), np.array([[0., top / w, 0., top / w]])
    return size, size, 0, 0, 1., np.zeros([1, 4])


def draw_photometric():
    """PhotometricDistort.__call__'s draws (:363-370): (flags, [brightness, contrast, saturation, hue]) as float64."""
    flags, u = 0, [0.0, 0.0, 0.0, 0.0]
    if random.randint(2):                                       # RandomBrightness(delta=32) :221-223
        u[0] = random.uniform(-32, 32)
        flags |= BRIGHTNESS
    first = random.randint(2)                                   # Compose(pd[:-1]) or Compose(pd[1:])

    def contrast():                                             # RandomContrast(0.5, 1.5) :208-210
        nonlocal flags
        if random.randint(2):
            u[1] = random.uniform(0.5, 1.5)
            flags |= CONTRAST
    if first:
        flags |= CONTRAST_FIRST
        contrast()
    if random.randint(2):                                       # RandomSaturation(0.5, 1.5) :146-147
        u[2] = random.uniform(0.5, 1.5)
        flags |= SATURATION
    if random.randint(2):                                       # RandomHue(18.0) :159-160
        u[3] = random.uniform(-18.0, 18.0)
        flags |= HUE
    if not first:
        contrast()
    return flags, u


def sample_crop(height, width, boxes, labels):
    """RandomSampleCrop.__call__ (:258-307) on the shape alone: (rect or None, boxes, labels)."""
    while True:
        mode = SAMPLE_OPTIONS[np.random.randint(len(SAMPLE_OPTIONS))]
        if mode is None:
            return None, boxes, labels
        for _ in range(50):
            w = random.uniform(0.3 * width, width)
            h = random.uniform(0.3 * height, height)
            if h / w < 0.5 or h / w > 2:
                continue
            left = random.uniform(width - w)                    # uniform(low=width - w, high=1.0): the reversed interval, kept
            top = random.uniform(height - h)
            rect = np.array([int(left), int(top), int(left + w), int(top + h)])
            # the IoU test (:281-286) needs max_iou < overlap.max() with max_iou always inf: it never rejects, so it is not computed
            centers = (boxes[:, :2] + boxes[:, 2:]) / 2.0
            m1 = (rect[0] < centers[:, 0]) * (rect[1] < centers[:, 1])
            m2 = (rect[2] > centers[:, 0]) * (rect[3] > centers[:, 1])
            mask = m1 * m2
            if not mask.any():
                continue
            current_boxes = boxes[mask, :].copy()
            current_labels = labels[mask]
            current_boxes[:, :2] = np.maximum(current_boxes[:, :2], rect[:2])
            current_boxes[:, :2] -= rect[:2]
            current_boxes[:, 2:] = np.minimum(current_boxes[:, 2:], rect[2:])
            current_boxes[:, 2:] -= rect[:2]
            return rect, current_boxes, current_labels


class TrainTransforms(object):
    """data/transforms.py:402-421: ConvertFromInts, ToAbsoluteCoords, PhotometricDistort, RandomSampleCrop, RandomMirror,
    ToPercentCoords, Resize, Normalize, ToTensor.  Same constructor, call signature and return tuple; `image` is the uint8 HxWx3
    BGR frame cv2.imread gives, and comes back as a CUDA float32 [3,size,size] tensor (`out=` writes into one slot of a batch).
    The caller's `boxes` are not changed (the reference scales its input view in place)."""

    crop = True

    def __init__(self, size=640, mean=(0.406, 0.456, 0.485), std=(0.225, 0.224, 0.229), handle=None, device=None):
        self.mean = mean
        self.size = size
        self.std = std
        self._mean32 = np.array(mean, dtype=np.float32)                 # Normalize(self.mean, self.std)
        self._std32 = np.array(std, dtype=np.float32)
        self._pad = np.array([v * 255 for v in mean]).astype(np.float32)  # Resize.mean: float64 products, float32 in the output
        self._handle = handle
        self._device = device

    def sample(self, shape, boxes, labels):
        """The host half: consumes np.random as the reference does -> (AugParams, boxes, labels, scale, offset)."""
        height, width = int(shape[0]), int(shape[1])
        boxes = np.array(boxes, copy=True)
        boxes[:, 0] *= width                                             # ToAbsoluteCoords :122-130
        boxes[:, 2] *= width
        boxes[:, 1] *= height
        boxes[:, 3] *= height
        flags, u = draw_photometric()
        x, y, cw, ch = 0, 0, width, height
        if self.crop:
            rect, boxes, labels = sample_crop(height, width, boxes, labels)
            if rect is not None:                                         # current_image[rect[1]:rect[3], rect[0]:rect[2]]
                y, y1, _ = slice(int(rect[1]), int(rect[3])).indices(height)
                x, x1, _ = slice(int(rect[0]), int(rect[2])).indices(width)
                cw, ch = x1 - x, y1 - y
        mirror = int(random.randint(2))                                  # RandomMirror :311-315, with the crop's width
        if mirror:
            boxes = boxes.copy()
            boxes[:, 0::2] = cw - boxes[:, 2::-2]
        boxes[:, 0] /= cw                                                # ToPercentCoords :133-141
        boxes[:, 2] /= cw
        boxes[:, 1] /= ch
        boxes[:, 3] /= ch
        rw, rh, left, top, scale, offset = letterbox(ch, cw, self.size)
        boxes = boxes * scale + offset
        geom = np.array([height, width, x, y, cw, ch, mirror, rw, rh, left, top, flags], dtype=np.int32)
        photo = np.concatenate([np.array(u, dtype=np.float64).astype(np.float32), self._pad])
        return AugParams(geom, photo), boxes, labels, scale, offset

    def _h(self):
        if self._handle is None:                                         # a bare handle: only its stream / error plumbing is used
            import torch
            from . import arch, capi
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._handle = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=dev)
        return self._handle

    def batch(self, images, records, out=None):
        """The device half: uint8 HxWx3 BGR frames (numpy arrays or CUDA uint8 tensors) and their records -> x float32
        [n,3,size,size] on the device, one kernel launch per 32 images."""
        import torch
        hd = self._h()
        assert len(images) == len(records)
        frames = [im if isinstance(im, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(im, dtype=np.uint8))
                  for im in images]
        frames = [f.to(hd.device, non_blocking=True).contiguous() for f in frames]
        geom = np.stack([r.geom for r in records]) if records else np.zeros((0, 12), np.int32)
        photo = np.stack([r.photo for r in records]) if records else np.zeros((0, 7), np.float32)
        return hd.train_transform_batch(frames, geom, photo, self.size, self._mean32, self._std32, out=out)

    def __call__(self, image, boxes, labels, scale=None, offset=None, out=None):
        rec, boxes, labels, scale, offset = self.sample(image.shape, boxes, labels)
        x = self.batch([image], [rec], out=None if out is None else out.view(1, *out.shape))
        return x.view(x.shape[1:]), boxes, labels, scale, offset


class ColorTransforms(TrainTransforms):
    """data/transforms.py:424-442: TrainTransforms without RandomSampleCrop (the colour pass of mosaic batches)."""

    crop = False
