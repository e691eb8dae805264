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

`Mosaic` (data/voc.py:140-233: load_mosaic, then the dataset's ColorTransforms) splits the same way: `sample_ids` / `sample` on the host
(Python's `random` for the ids and the centre, np.random inside the colour pass), `batch` on the device, where the four uint8 frames
become one network input without the float64 2S x 2S canvas ever being built (DESIGN.md "Mosaic on the device").  `sample_item` and
`collate` restate pull_item's branch and fill one batch tensor from a mixed list of single-image and mosaic records.
"""
import random as pyrandom
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


MosaicParams = namedtuple("MosaicParams", "geom photo")
MosaicParams.__doc__ = """One mosaic's device parameters: geom int32 [50] = per frame k (12 values at 12*k) h0, w0, rw, rh, canvas
rectangle x1a, y1a, x2a, y2a, source rectangle x1b, y1b, x2b, y2b; then mirror, flags; photo float32 [7] as AugParams (the pad is
the canvas fill)."""


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


def place(i, h, w, xc, yc, s):
    """load_mosaic's four placement cases (data/voc.py:174-185) for resized frame i of h x w around the centre (xc, yc) of the
    2s x 2s canvas: (x1a, y1a, x2a, y2a) on the canvas, (x1b, y1b, x2b, y2b) in the frame."""
    if i == 0:                                                          # top left
        x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
        x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
    elif i == 1:                                                        # top right
        x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
        x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
    elif i == 2:                                                        # bottom left
        x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
        x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
    else:                                                               # bottom right
        x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
        x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
    return (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b)


def use_mosaic(mosaic):
    """pull_item's branch (data/voc.py:216): `self.mosaic and np.random.randint(2)` - the draw happens only when mosaic is on."""
    return bool(mosaic and np.random.randint(2))


class Mosaic(object):
    """load_mosaic (data/voc.py:140-211, data/coco.py:126-197) followed by the dataset's `color_augment` (ColorTransforms), with the
    pixel work on the device: four uint8 BGR frames -> one float32 [3,size,size] network input, the 2S x 2S canvas never built.

    `sample_ids` and `sample` are the host half (Python's `random` for load_mosaic's own draws, `np.random` inside
    `color_augment.sample`, as in the reference; numpy only); `batch` is the device half.  Quirks kept: the canvas is float64 and its
    fill float64(mean) * 255 goes through the photometric chain as part of the image; `int()` truncates the centre and the resized
    extents; a frame whose long side equals `img_size` is pasted unresized (`r != 1`)."""

    def __init__(self, img_size, color_augment):
        self.img_size = int(img_size)
        self.color_augment = color_augment

    def sample_ids(self, index, n_ids):
        """[index, j2, j3, j4]: `random.sample(self.ids[:index] + self.ids[index+1:], 3)` (:141-145) by position.  Sampling
        range(n_ids - 1) consumes the same draws and picks the same positions as sampling the list itself."""
        picks = pyrandom.sample(range(n_ids - 1), 3)
        return [index] + [j if j < index else j + 1 for j in picks]

    def compose(self, shapes, targets, center=None):
        """load_mosaic without the pixels: the four (h0, w0) shapes and four target lists (rows x1, y1, x2, y2 as fractions, class;
        a list may be empty) -> (frames int32 [4,12] = the per-frame part of MosaicParams.geom, (yc, xc), mosaic_tg float64 [n,5]).
        `center=(yc, xc)` replaces the two `random.uniform` draws."""
        s = self.img_size
        if center is None:
            yc, xc = [int(pyrandom.uniform(-x, 2 * s + x)) for x in [(-s) // 2, (-s) // 2]]     # :158, yc first
        else:
            yc, xc = int(center[0]), int(center[1])
        frames = np.zeros((4, 12), np.int32)
        mosaic_tg = []
        for i in range(4):
            target_i = np.array(targets[i])
            h0, w0 = int(shapes[i][0]), int(shapes[i][1])
            r = s / max(h0, w0)                                          # :168
            h, w = h0, w0
            if r != 1:
                w, h = int(w0 * r), int(h0 * r)                          # cv2.resize(img_i, (int(w0 * r), int(h0 * r)))
                if w <= 0 or h <= 0:
                    raise ValueError("mosaic frame %d: %dx%d resizes to %dx%d at img_size %d" % (i, w0, h0, w, h, s))
            a, b = place(i, h, w, xc, yc, s)
            frames[i] = (h0, w0, w, h) + a + b
            padw = a[0] - b[0]
            padh = a[1] - b[1]
            target_i_ = target_i.copy()
            if len(target_i) > 0:                                        # :193-200
                target_i_[:, 0] = (w * (target_i[:, 0]) + padw)
                target_i_[:, 1] = (h * (target_i[:, 1]) + padh)
                target_i_[:, 2] = (w * (target_i[:, 2]) + padw)
                target_i_[:, 3] = (h * (target_i[:, 3]) + padh)
                mosaic_tg.append(target_i_)
        if len(mosaic_tg) == 0:                                          # :202-209
            mosaic_tg = np.zeros([1, 5])
        else:
            mosaic_tg = np.concatenate(mosaic_tg, axis=0)
            np.clip(mosaic_tg[:, :4], 0, 2 * s, out=mosaic_tg[:, :4])
            mosaic_tg[:, :4] /= (s * 2)
        return frames, (yc, xc), mosaic_tg

    def sample(self, shapes, targets, center=None):
        """The host half of one mosaic sample -> (MosaicParams, boxes, labels, scale, offset), as pull_item's mosaic branch
        (:218-220) returns them."""
        s = self.img_size
        frames, _, target = self.compose(shapes, targets, center)
        rec, boxes, labels, scale, offset = self.color_augment.sample((2 * s, 2 * s), target[:, :4], target[:, 4])
        geom = np.concatenate([frames.reshape(-1), [rec.geom[6], rec.geom[11]]]).astype(np.int32)
        return MosaicParams(geom, rec.photo), boxes, labels, scale, offset

    def batch(self, frame_quads, records, out=None):
        """The device half: per mosaic its four uint8 HxWx3 BGR frames (numpy arrays or CUDA uint8 tensors) and its record -> x
        float32 [n,3,size,size] on the device."""
        import torch
        ca = self.color_augment
        hd = ca._h()
        assert len(frame_quads) == len(records) and all(len(q) == 4 for q in frame_quads)
        frames = [im if isinstance(im, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(im, dtype=np.uint8))
                  for q in frame_quads for im in q]
        frames = [f.to(hd.device, non_blocking=True).contiguous() for f in frames]
        geom = np.stack([r.geom for r in records]) if records else np.zeros((0, 50), np.int32)
        photo = np.stack([r.photo for r in records]) if records else np.zeros((0, 7), np.float32)
        return hd.mosaic_transform_batch(frames, geom, photo, self.img_size, ca.size, ca._mean32, ca._std32, out=out)


def sample_item(index, n_ids, load, transform, mosaic=None):
    """pull_item (data/voc.py:214-233) up to the pixels, for a worker: `load(j) -> (uint8 frame, target list)` is the dataset's
    load_img_targets, `transform` its TrainTransforms, `mosaic` its Mosaic or None.  -> (frames, record, target): `frames` is the one
    frame or the list of four, `record` an AugParams or MosaicParams for `collate`, `target` the [n,5] rows of :233."""
    if use_mosaic(mosaic is not None):
        ids = mosaic.sample_ids(index, n_ids)
        loaded = [load(j) for j in ids]
        frames = [f for f, _ in loaded]
        rec, boxes, labels, _, _ = mosaic.sample([f.shape for f in frames], [t for _, t in loaded])
    else:
        frames, target = load(index)
        target = np.zeros([1, 5]) if len(target) == 0 else np.array(target)
        rec, boxes, labels, _, _ = transform.sample(frames.shape, target[:, :4], target[:, 4])
    return frames, rec, np.hstack((boxes, np.expand_dims(labels, axis=1)))


def collate(transform, mosaic, items, out=None):
    """The mixed batch: items = [(frames, record), ...] from `sample_item` -> ONE float32 [B,3,size,size] tensor on the device, in the
    items' order, with one yn_train_transform_batch call for all single images and one yn_mosaic_transform_batch call for all
    mosaics.  A kind whose samples fill a run of neighbouring slots is written in place; otherwise it is computed into a buffer of
    its own and copied to its slots on the device."""
    import torch
    size = transform.size
    hd = transform._h()
    if out is None:
        out = torch.empty((len(items), 3, size, size), dtype=torch.float32, device=hd.device)
    assert tuple(out.shape) == (len(items), 3, size, size)
    kinds = [[k for k, (_, r) in enumerate(items) if isinstance(r, MosaicParams) == m] for m in (False, True)]
    for slots, run in zip(kinds, (transform.batch, None if mosaic is None else mosaic.batch)):
        if not slots:
            continue
        frames, recs = [items[k][0] for k in slots], [items[k][1] for k in slots]
        if slots[-1] - slots[0] + 1 == len(slots):
            run(frames, recs, out=out[slots[0]:slots[-1] + 1])
        else:
            out.index_copy_(0, torch.as_tensor(slots, device=out.device), run(frames, recs))
    return out
