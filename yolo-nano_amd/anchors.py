"""Anchor boxes for a dataset of one's own: kmeans_anchor.py's k-means on the device, through yn_kmeans_*.

    boxes = dataset_boxes(annotations, image_sizes, img_size=416)       # (N, 2) float64 [w, h], as the reference's loader builds them
    centroids = anchor_box_kmeans(boxes, 9)                             # (9, 2) float64, the reference's run for np.random's state
    model = YOLONano(device, anchor_size=as_anchor_table(centroids), ...)

The distance is 1 - IoU of boxes centred at the origin, in float64 and in the reference's operation order; assignment, centroid update,
loss, the convergence loop and k-means++ seeding are the reference's.  Every sum is the correctly rounded exact sum (the device adds
integers and rounds once), so the result does not depend on box order or on the launch, and tests/kmeans_oracle.py reproduces it bit for
bit on the host.  The host draws the random numbers, in the reference's order; the device does every pass.  Boxes must lie in
1 <= w, h < 65536 (the reference's loader already drops anything below 1).
"""
import ctypes
import random

import numpy as np

MAX_BOXES = 1 << 24
MAX_ANCHORS = 32


def check_boxes(boxes):
    """`boxes` as a C-contiguous (N, 2) float64 array; ValueError, with their number, if any lies outside 1 <= w, h < 65536."""
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64))
    if b.ndim != 2 or b.shape[1] != 2 or not 1 <= b.shape[0] <= MAX_BOXES:
        raise ValueError("boxes must be an (N, 2) array of [w, h] with 1 <= N <= 2^24, got shape %r" % (b.shape,))
    with np.errstate(invalid="ignore"):
        bad = int((~((b >= 1.0) & (b < 65536.0)).all(axis=1)).sum())
    if bad:
        raise ValueError("%d of %d boxes are outside the domain 1 <= w, h < 65536 or not finite" % (bad, len(b)))
    return b


def dataset_boxes(annotations, image_sizes, img_size):
    """The reference's loader (kmeans_anchor.py:187-226) on arrays: `annotations[i]` holds image i's boxes as rows xmin, ymin, xmax, ymax
    (further columns, such as the label, are ignored) in the units of `image_sizes[i]` = (width, height).  Per box
    bw = (xmax - xmin) / max(w, h) * img_size, bh likewise; boxes with bw < 1 or bh < 1 are dropped.  -> (N, 2) float64."""
    if len(annotations) != len(image_sizes):
        raise ValueError("one (width, height) per annotation array")
    out = []
    for ann, (w, h) in zip(annotations, image_sizes):
        a = np.asarray(ann, dtype=np.float64)
        if a.size == 0:
            continue
        a = a.reshape(len(a), -1)
        side = max(w, h)
        bw = (a[:, 2] - a[:, 0]) / side * img_size
        bh = (a[:, 3] - a[:, 1]) / side * img_size
        keep = ~((bw < 1.0) | (bh < 1.0))
        out.append(np.stack([bw[keep], bh[keep]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.float64)


def as_anchor_table(centroids):
    """Centroids -> the nested-list form of arch.MULTI_ANCHOR_SIZE: rows sorted by area (ascending, as the tables in data/config.py are),
    each side rounded to 2 decimals as the reference prints it.  YOLONano(anchor_size=...) wants a multiple of 3 rows (9 for 3 scales)."""
    c = np.asarray(centroids, dtype=np.float64).reshape(-1, 2)
    rows = [[round(float(w), 2), round(float(h), 2)] for w, h in c]
    rows.sort(key=lambda r: (r[0] * r[1], r[0], r[1]))
    return rows


class AnchorKMeans:
    """The boxes of one dataset on the device (yn_kmeans), clustered any number of times.

        km = AnchorKMeans(boxes)
        km.seed(9)                      # k-means++ with np.random, or seed(9, plus=False), or km.set_centroids(array)
        centroids, counts, loss = km.step()                 # one do_kmeans
        centroids, counts, loss, iterations = km.run()      # anchor_box_kmeans's loop from the current centroids
        groups = km.assign()            # int32 device tensor [N]
    """

    def __init__(self, boxes, max_anchors=MAX_ANCHORS, device=None, handle=None):
        import torch
        from . import capi
        self.lib = capi.load_library()
        self._handle, self._device = handle, device
        self.e = None
        if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
            if boxes.ndim != 2 or boxes.shape[1] != 2 or not 1 <= boxes.shape[0] <= MAX_BOXES:
                raise ValueError("boxes must be an (N, 2) tensor of [w, h] with 1 <= N <= 2^24, got shape %r" % (tuple(boxes.shape),))
            if self._device is None and handle is None:
                self._device = boxes.device
            h = self._h()
            dev = h._in(boxes, torch.float64)                  # the domain is checked on the device (yn_kmeans_set_boxes)
        else:
            host = check_boxes(boxes.cpu().numpy() if isinstance(boxes, torch.Tensor) else boxes)
            h = self._h()
            dev = torch.from_numpy(host).to(h.device)
        self.n = int(dev.shape[0])
        self._src = boxes if isinstance(boxes, torch.Tensor) else host      # what seed_from picks its rows from
        self.k = 0
        self.picked = None
        e = ctypes.c_void_p()
        h._ck(self.lib.yn_kmeans_create(h.h, self.n, int(max_anchors), ctypes.byref(e)), "yn_kmeans_create")
        self.e = e
        try:
            h._ck(self.lib.yn_kmeans_set_boxes(h.h, self.e, dev.data_ptr(), self.n), "yn_kmeans_set_boxes")
        except Exception:
            self.close()
            raise

    def _h(self, handle=None):
        if handle is not None:
            return handle
        if self._handle is None:                               # a bare handle: only its stream / error plumbing is used
            import torch
            from . import arch, capi
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._handle = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=dev)
        return self._handle

    def close(self):
        if getattr(self, "e", None):
            self.lib.yn_kmeans_destroy(self.e)
            self.e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def seed(self, n_anchors, plus=True, rng=None, handle=None):
        """Initial centroids as anchor_box_kmeans chooses them.  plus=True: init_centroids, with np.random (or the RandomState `rng`)
        drawn in the reference's order: choice(N, 1), then one random() per further centroid.  plus=False: random.sample(range(N),
        n_anchors) (or `rng.sample`, a random.Random).  -> centroids (n_anchors, 2); .picked holds the box indices (-1: none, (0, 0))."""
        k = int(n_anchors)
        if not 1 <= k <= MAX_ANCHORS:
            raise ValueError("n_anchors must be 1..%d" % MAX_ANCHORS)
        if not plus:
            idx = (rng or random).sample(range(self.n), k)
            return self.seed_from(idx, handle=handle)
        r = rng if rng is not None else np.random
        first = int(r.choice(self.n, 1)[0])
        u = np.zeros(max(k - 1, 1), dtype=np.float64)
        for i in range(k - 1):
            u[i] = r.random() if hasattr(r, "random") else r.random_sample()
        return self.seed_draws(k, first, u[:k - 1], handle=handle)

    def seed_draws(self, n_anchors, first_index, draws, handle=None):
        """k-means++ from explicit draws: the first box index and the n_anchors - 1 uniform numbers (yn_kmeans_seed)."""
        h = self._h(handle)
        k = int(n_anchors)
        u = np.ascontiguousarray(np.asarray(draws, dtype=np.float64).reshape(-1))
        if len(u) != k - 1:
            raise ValueError("n_anchors - 1 draws are needed")
        cent = np.zeros((k, 2), dtype=np.float64)
        picked = np.zeros(k, dtype=np.int32)
        h._ck(self.lib.yn_kmeans_seed(h.h, self.e, k, int(first_index), u.ctypes.data if k > 1 else None, cent.ctypes.data, picked.ctypes.data),
              "yn_kmeans_seed")
        self.k, self.picked = k, picked
        return cent

    def seed_from(self, indices, handle=None):
        """The boxes at `indices` as centroids (the plus=False branch)."""
        h = self._h(handle)
        idx = [int(i) for i in indices]
        if any(not 0 <= i < self.n for i in idx):
            raise ValueError("a centroid index is outside 0..N-1")
        cent = np.asarray(self._src[idx].cpu().numpy() if hasattr(self._src, "cpu") else self._src[idx], dtype=np.float64).reshape(-1, 2)
        self.set_centroids(cent, handle=h)
        self.picked = np.asarray(idx, dtype=np.int32)
        return cent

    def set_centroids(self, centroids, handle=None):
        h = self._h(handle)
        c = np.ascontiguousarray(np.asarray(centroids, dtype=np.float64).reshape(-1, 2))
        h._ck(self.lib.yn_kmeans_set_centroids(h.h, self.e, c.ctypes.data, len(c)), "yn_kmeans_set_centroids")
        self.k, self.picked = len(c), None

    def step(self, handle=None):
        """One do_kmeans -> (centroids (k, 2) float64, counts (k,) int64, loss)."""
        h = self._h(handle)
        cent, counts, loss = np.zeros((max(self.k, 1), 2)), np.zeros(max(self.k, 1), dtype=np.int64), ctypes.c_double()
        h._ck(self.lib.yn_kmeans_pass(h.h, self.e, cent.ctypes.data, counts.ctypes.data, ctypes.byref(loss)), "yn_kmeans_pass")
        return cent, counts, loss.value

    def run(self, loss_convergence=1e-6, iters=1000, handle=None):
        """anchor_box_kmeans's loop from the current centroids -> (centroids, counts, loss, iterations) of its last pass."""
        h = self._h(handle)
        cent, counts = np.zeros((max(self.k, 1), 2)), np.zeros(max(self.k, 1), dtype=np.int64)
        loss, it = ctypes.c_double(), ctypes.c_int32()
        h._ck(self.lib.yn_kmeans_run(h.h, self.e, float(loss_convergence), int(iters), cent.ctypes.data, counts.ctypes.data,
                                     ctypes.byref(loss), ctypes.byref(it)), "yn_kmeans_run")
        return cent, counts, loss.value, it.value

    def stats(self):
        """(passes, host reads) of the last run()"""
        p, r = ctypes.c_int64(), ctypes.c_int64()
        self.lib.yn_kmeans_stats(self.e, ctypes.byref(p), ctypes.byref(r))
        return p.value, r.value

    def assign(self, handle=None):
        """The group of every box for the current centroids: an int32 device tensor [N]."""
        import torch
        h = self._h(handle)
        with torch.cuda.stream(h._torch_stream()):
            g = torch.empty(self.n, dtype=torch.int32, device=h.device)
        h._ck(self.lib.yn_kmeans_assign(h.h, self.e, g.data_ptr()), "yn_kmeans_assign")
        h._ck(self.lib.yn_synchronize(h.h), "yn_synchronize")
        return g


def anchor_box_kmeans(boxes, n_anchors, loss_convergence=1e-6, iters=1000, plus=True, rng=None, handle=None, return_info=False):
    """kmeans_anchor.py's anchor_box_kmeans(total_gt_boxes, n_anchors, loss_convergence, iters, plus) on the device.  `boxes` is an
    (N, 2) float64 array or CUDA tensor of [w, h].  -> centroids (n_anchors, 2) float64; with return_info=True also a dict with
    'loss', 'counts', 'iterations' and 'picked' (the seed box indices)."""
    km = AnchorKMeans(boxes, max_anchors=max(int(n_anchors), 1), handle=handle)
    try:
        km.seed(n_anchors, plus=plus, rng=rng)
        cent, counts, loss, it = km.run(loss_convergence, iters)
        info = {"loss": loss, "counts": counts, "iterations": it, "picked": km.picked}
    finally:
        km.close()
    return (cent, info) if return_info else cent
