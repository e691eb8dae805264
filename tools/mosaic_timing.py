#!/usr/bin/env python3
"""Mosaic timing (yn_mosaic_transform_batch): 32 mosaics from 128 uint8 frames of 500x375 already in HBM, to 416 and to 608, next to
the single-image pass (yn_train_transform_batch, 32 of the same frames) in the same run, a mixed batch of 16 single + 16 mosaic at
608, and the fp16 training step at 608 (batch 32) the augmentation budget is a share of.  Same protocol as tools/train_aug_timing.py:
events after warm-up, median over --iters samples of 20 back-to-back calls.  The HBM floor is the output (n*3*side^2*4 bytes) plus
the frames' bytes at 8.0 TB/s.  Prints one JSON line.

    python tools/mosaic_timing.py [--iters 50] [--no-step]
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_nano_amd import ColorTransforms, Mosaic, TrainTransforms  # noqa: E402

N, H0, W0, HBM, REPS = 32, 375, 500, 8.0e12, 20


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):                                  # REPS calls back to back: the device time, not the host's enqueue
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / REPS)
    return float(np.median(times)), float(np.min(times))


def workload(size, seed):
    """128 frames on the device; 32 mosaic records over all of them and 32 single-image records over the first 32."""
    rs = np.random.RandomState(seed)
    random.seed(seed)
    np.random.seed(seed)
    tf = TrainTransforms(size)
    mz = Mosaic(size, ColorTransforms(size, handle=tf._h()))
    frames = [torch.as_tensor(rs.randint(0, 256, (H0, W0, 3)).astype(np.uint8)).cuda() for _ in range(4 * N)]

    def target():
        xy = rs.rand(2, 2) * 0.6
        return np.hstack([xy, xy + 0.1 + rs.rand(2, 2) * 0.3, np.ones((2, 1))])
    mrec = [mz.sample([(H0, W0)] * 4, [target().tolist() for _ in range(4)])[0] for _ in range(N)]
    srec = []
    for _ in range(N):
        t = target()
        srec.append(tf.sample((H0, W0, 3), t[:, :4], t[:, 4])[0])
    return tf, mz, frames, mrec, srec


def report(us, mn, n_out, n_frames, size):
    floor_us = (n_out * 3 * size * size * 4 + n_frames * H0 * W0 * 3) / HBM * 1e6
    return {"us_per_batch": round(us, 1), "images_per_s": round(n_out / us * 1e6), "hbm_floor_us": round(floor_us, 1),
            "floor_share": round(floor_us / us, 3), "min_us": round(mn, 1)}


def device(size, iters, mixed):
    tf, mz, frames, mrec, srec = workload(size, size)
    hd = tf._h()
    out = torch.empty((N, 3, size, size), device="cuda")
    mg, mp = np.stack([r.geom for r in mrec]), np.stack([r.photo for r in mrec])
    sg, sp = np.stack([r.geom for r in srec]), np.stack([r.photo for r in srec])
    fill = float(np.mean([1.0 - sum((g[12 * k + 6] - g[12 * k + 4]) * (g[12 * k + 7] - g[12 * k + 5]) for k in range(4)) / (4.0 * size * size)
                          for g in mg]))
    res = {}
    us, mn = timed(lambda: hd.mosaic_transform_batch(frames, mg, mp, size, size, tf._mean32, tf._std32, out=out), iters)
    res["mosaic"] = report(us, mn, N, 4 * N, size)
    res["mosaic"]["fill_share_of_canvas"] = round(fill, 3)
    us1, mn1 = timed(lambda: hd.train_transform_batch(frames[:N], sg, sp, size, tf._mean32, tf._std32, out=out), iters)
    res["single"] = report(us1, mn1, N, N, size)
    res["mosaic_over_single"] = round(us / us1, 3)
    if mixed:
        h = N // 2

        def both():                                         # 16 single images into slots 0..15, 16 mosaics into slots 16..31
            hd.train_transform_batch(frames[:h], sg[:h], sp[:h], size, tf._mean32, tf._std32, out=out[:h])
            hd.mosaic_transform_batch(frames[4 * h:], mg[h:], mp[h:], size, size, tf._mean32, tf._std32, out=out[h:])
        usm, mnm = timed(both, iters)
        res["mixed_16_16"] = report(usm, mnm, N, h + 4 * h, size)
        tmp_s, tmp_m = torch.empty((h, 3, size, size), device="cuda"), torch.empty((h, 3, size, size), device="cuda")
        even, odd = torch.arange(0, N, 2, device="cuda"), torch.arange(1, N, 2, device="cuda")

        def scattered():                                    # the two kinds interleaved: each into its own buffer, then to its slots
            hd.train_transform_batch(frames[:h], sg[:h], sp[:h], size, tf._mean32, tf._std32, out=tmp_s)
            hd.mosaic_transform_batch(frames[4 * h:], mg[h:], mp[h:], size, size, tf._mean32, tf._std32, out=tmp_m)
            out.index_copy_(0, even, tmp_s)
            out.index_copy_(0, odd, tmp_m)
        uss, mns = timed(scattered, iters)
        res["mixed_16_16_interleaved"] = {"us_per_batch": round(uss, 1), "min_us": round(mns, 1)}
    return res


def step_us(size, iters):
    """The fp16 training step at `size`, batch 32, on an augmented batch."""
    from yolo_nano_amd import arch, capi, multi_gt_creator, weights
    tf, mz, frames, mrec, srec = workload(size, 1)
    x = tf.batch(frames[:N], srec)
    labels = [[[0.2, 0.2, 0.6, 0.7, 3.0], [0.5, 0.4, 0.9, 0.8, 7.0]] for _ in range(N)]
    target = multi_gt_creator(size, [8, 16, 32], labels, anchor_size=arch.MULTI_ANCHOR_SIZE)
    h = capi.Handle(size, 20, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=N)
    h.load_state_dict(weights.make_state_dict("1.0x", 20))
    h.train_bind()
    h.train_precision("f16")
    for _ in range(5):
        h.train_step(x, target, lr=1e-4)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        h.train_step(x, target, lr=1e-4)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    h.close()
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-step", action="store_true", help="skip the training-step measurement")
    a = ap.parse_args()
    res = {"batch": N, "frame": [H0, W0], "frames_per_mosaic": 4}
    for size in (416, 608):
        res["device_%d" % size] = device(size, a.iters, mixed=size == 608)
    if not a.no_step:
        st = step_us(608, a.iters)
        mixed = res["device_608"]["mixed_16_16"]["us_per_batch"]
        res["fp16_step_608_bs32_us"] = round(st, 1)
        res["budget_us_2pct_of_step"] = round(0.02 * st, 1)
        res["mixed_16_16_share_of_step"] = round(mixed / st, 4)
    res["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
