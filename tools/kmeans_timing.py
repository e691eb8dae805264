#!/usr/bin/env python3
"""Anchor k-means timing (yn_kmeans_*): N = 900 000 synthetic log-normal boxes (about VOC0712 + COCO train2017), K = 9.  Times, after a
warm-up of every call, the k-means++ seeding, a fixed 50 passes (loss_convergence = 0, iters = 49) and a run to convergence, each with a
host clock around a call that ends in a device synchronise (best of three).  Also times one pass of the vectorised host restatement
tests/kmeans_oracle.py on the same boxes, and a scalar pure-Python pass in the reference's style (one IoU call per box and centroid, on
attribute-carrying box objects) on a 20 000-box subset, scaled by N: that figure is EXTRAPOLATED and marked so.  Prints one JSON line.

The 16 B/box floor is the time the spec HBM bandwidth (8 TB/s) needs to deliver the boxes once per pass; the 14.4 MB of boxes fit the
256 MiB cache in front of HBM, so a pass of a running loop need not touch HBM at all: the share is an accounting figure, not a bound.

    python tools/kmeans_timing.py [--boxes 900000] [--subset 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo_nano_amd import AnchorKMeans  # noqa: E402
import kmeans_oracle  # noqa: E402

K = 9
HBM_BYTES_PER_S = 8.0e12


class _Box:
    def __init__(self, w, h):
        self.x, self.y, self.w, self.h = 0, 0, w, h


def _iou(a, b):
    ax0, ax1, ay0, ay1 = a.x - a.w / 2, a.x + a.w / 2, a.y - a.h / 2, a.y + a.h / 2
    bx0, bx1, by0, by1 = b.x - b.w / 2, b.x + b.w / 2, b.y - b.h / 2, b.y + b.h / 2
    iw, ih = min(ax1, bx1) - max(ax0, bx0), min(ay1, by1) - max(ay0, by0)
    if iw < 0 or ih < 0:
        return 0
    inter = iw * ih
    return inter / (a.w * a.h + b.w * b.h - inter)


def scalar_pass(boxes, centroids):
    """one pass as a scalar interpreter loop: N * K IoU calls on objects, running sums"""
    sums = [[0.0, 0.0, 0] for _ in centroids]
    loss = 0
    for box in boxes:
        best, g = 1, 0
        for k, c in enumerate(centroids):
            d = 1 - _iou(box, c)
            if d < best:
                best, g = d, k
        loss += best
        s = sums[g]
        s[0] += box.w; s[1] += box.h; s[2] += 1
    return [[s[0] / max(s[2], 1), s[1] / max(s[2], 1)] for s in sums], loss


def best_of(fn, n=3):
    best = None
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if best is None or t < best[0]:
            best = (t, r)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=900000)
    ap.add_argument("--subset", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_timing: needs a GPU")
    rng = np.random.RandomState(0)
    boxes = np.clip(np.exp(rng.normal(4.0, 0.9, size=(a.boxes, 2))), 1.0, 512.0)
    first, draws = kmeans_oracle.draws_from(np.random.RandomState(1), a.boxes, K)

    km = AnchorKMeans(boxes, max_anchors=K)
    seeds = km.seed_draws(K, first, draws)                             # warm-up of the seeding kernels
    km.run(0.0, 3)                                                     # and of the pass
    t_seed, seeds = best_of(lambda: km.seed_draws(K, first, draws))

    def fixed():
        km.set_centroids(seeds)
        return km.run(0.0, 49)

    def converge():
        km.set_centroids(seeds)
        return km.run(1e-6, 1000)

    t_set, _ = best_of(lambda: km.set_centroids(seeds))
    t_fixed, r_fixed = best_of(fixed)
    passes_fixed, reads_fixed = km.stats()
    t_conv, r_conv = best_of(converge)
    passes_conv, reads_conv = km.stats()
    assert r_fixed[3] == 50 == passes_fixed
    us_pass = (t_fixed - t_set) / 50 * 1e6
    floor_us = 16.0 * a.boxes / HBM_BYTES_PER_S * 1e6

    t0 = time.perf_counter()
    want = kmeans_oracle.do_kmeans(boxes, seeds)
    oracle_s = time.perf_counter() - t0
    got = (km.set_centroids(seeds), km.step())[1]
    bit_equal = bool(np.array_equal(got[0].view(np.int64), want[0].view(np.int64)) and got[2] == want[3])

    sub = [_Box(float(w), float(h)) for w, h in boxes[:a.subset]]
    cents = [_Box(float(w), float(h)) for w, h in seeds]
    t0 = time.perf_counter()
    scalar_pass(sub, cents)
    scalar_s = (time.perf_counter() - t0) * a.boxes / len(sub)

    out = {"gpu": torch.cuda.get_device_name(0), "boxes": a.boxes, "k": K,
           "seed_ms": round(t_seed * 1e3, 3),
           "pass_us": round(us_pass, 2), "fixed_passes": 50, "fixed_ms": round(t_fixed * 1e3, 3),
           "hbm_floor_us": round(floor_us, 2), "floor_share": round(floor_us / us_pass, 3),
           "passes_per_host_read": round(passes_fixed / reads_fixed, 1),
           "converge_ms": round(t_conv * 1e3, 3), "converge_iterations": int(r_conv[3]), "converge_host_reads": int(reads_conv),
           "converge_loss": r_conv[2],
           "oracle_pass_s": round(oracle_s, 4), "pass_bit_equal_to_oracle": bit_equal,
           "scalar_python_pass_s_extrapolated": round(scalar_s, 1), "scalar_python_subset": len(sub),
           "speedup_vs_oracle": round(oracle_s / (us_pass * 1e-6), 0),
           "speedup_vs_scalar_python_extrapolated": round(scalar_s / (us_pass * 1e-6), 0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
