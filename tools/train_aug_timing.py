#!/usr/bin/env python3
"""TrainTransforms timing (yn_train_transform_batch): a 32-image batch of 500x375 uint8 frames already in HBM, to 416 and to 608.
Times the device pass with events after warm-up (median over --iters samples of 20 back-to-back launches), reports images/s and the pass's share of its HBM
floor (output n*3*side^2*4 bytes plus the frames' bytes, against 8.0 TB/s), and the host sampler's cost per image in the process's
own CPU time.  Prints one JSON line.

    python tools/train_aug_timing.py [--iters 50] [--sampler 5000]
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
from yolo_nano_amd import TrainTransforms  # noqa: E402

N, H0, W0, HBM, REPS = 32, 375, 500, 8.0e12, 20


def workload(tf, seed):
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    frames, recs = [], []
    for _ in range(N):
        f = rs.randint(0, 256, (H0, W0, 3)).astype(np.uint8)
        xy = rs.rand(2, 2) * 0.6
        t = np.hstack([xy, xy + 0.1 + rs.rand(2, 2) * 0.3, np.ones((2, 1))])
        frames.append(torch.as_tensor(f).cuda())
        recs.append(tf.sample(f.shape, t[:, :4], t[:, 4])[0])
    return frames, recs


def device_us(size, iters):
    tf = TrainTransforms(size)
    frames, recs = workload(tf, size)
    out = torch.empty((N, 3, size, size), device="cuda")
    for _ in range(10):
        tf.batch(frames, recs, out=out)
    torch.cuda.synchronize()
    hd = tf._h()
    geom = np.stack([r.geom for r in recs])
    photo = np.stack([r.photo for r in recs])
    times = []
    for _ in range(iters):                                  # REPS launches back to back: the device time, not the host's enqueue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            hd.train_transform_batch(frames, geom, photo, size, tf._mean32, tf._std32, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / REPS)
    us = float(np.median(times))
    bytes_ = N * 3 * size * size * 4 + N * H0 * W0 * 3
    floor_us = bytes_ / HBM * 1e6
    return {"us_per_batch": round(us, 1), "images_per_s": round(N / us * 1e6), "hbm_floor_us": round(floor_us, 1),
            "floor_share": round(floor_us / us, 3), "min_us": round(float(np.min(times)), 1)}


def sampler_us(n):
    tf = TrainTransforms(416)
    rs = np.random.RandomState(1)
    targets = [np.hstack([xy, xy + 0.1 + rs.rand(3, 2) * 0.3, np.ones((3, 1))]) for xy in rs.rand(64, 3, 2) * 0.6]
    np.random.seed(1)
    t0 = time.process_time()
    for i in range(n):
        t = targets[i % 64]
        tf.sample((H0, W0, 3), t[:, :4], t[:, 4])
    return (time.process_time() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sampler", type=int, default=5000)
    a = ap.parse_args()
    res = {"batch": N, "frame": [H0, W0]}
    for size in (416, 608):
        res["device_%d" % size] = device_us(size, a.iters)
    res["sampler_us_per_image_cpu"] = round(sampler_us(a.sampler), 1)
    res["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
