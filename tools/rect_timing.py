#!/usr/bin/env python3
"""Rectangular inference against the letterboxed square: 32 seeded uint8 frames of 1280x720, COCO head, 1.0x backbone, random weights, side 640.

  route A  the square: yn_preprocess_batch -> yn_infer -> yn_pack_detections on [32,3,640,640] (360 rows of picture between two 140-row bands of pad)
  route B  the 640x384 window at (0, 128) of that square (rect_window of the frames): yn_set_grid_rect, yn_preprocess_batch_rect -> yn_infer ->
           yn_pack_detections on [32,3,384,640] - 0.6 of the pixels, of the activation bytes and of the candidates
  both at conf 0.001 / nms 0.5 and at conf 0.1 / nms 0.45; yn_forward_raw alone on either canvas.

HIP events around --inner batches after a warm-up of every shape (the autotuner has picked its tiles by then: its table is per shape), the two
routes alternating window by window, median (min, max) of --repeats windows, ms per batch.  Prints ONE JSON line.

    python tools/rect_timing.py [--repeats 7] [--inner 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_nano_amd import arch, capi, rect_window, weights  # noqa: E402
from yolo_nano_amd.model import ValTransforms  # noqa: E402

B, W0, H0, SIDE, C = 32, 1280, 720, 640, 80


def window_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def stats(ts):
    return [round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rect_timing needs the GPU"
    rng = np.random.RandomState(0)
    frames = [torch.from_numpy(rng.randint(0, 256, size=(H0, W0, 3)).astype(np.uint8)).cuda() for _ in range(B)]
    h = capi.Handle(SIDE, C, arch.MULTI_ANCHOR_SIZE_COCO, "1.0x", 0.001, 0.5, max_batch=B)
    h.load_state_dict(weights.make_state_dict("1.0x", C))
    h.fold_bn()
    tf = ValTransforms(SIDE, handle=h)
    geoms = [tf.geometry(H0, W0)[:4] for _ in range(B)]
    left, top, W, H = rect_window(geoms, SIDE)
    assert (left, top, W, H) == (0, 128, 640, 384), (left, top, W, H)

    def grid_a():
        h.set_grid(SIDE)

    def grid_b():
        h.set_grid_rect(H, W, SIDE, left, top)

    grid_a()
    xa, outa = torch.empty((B, 3, SIDE, SIDE), device="cuda"), h.alloc_outputs(B)
    reca, offa = torch.empty((B * h.N, 6), device="cuda"), torch.empty((B + 1,), dtype=torch.int32, device="cuda")
    heads_a = [torch.empty(s, device="cuda") for s in h.head_shapes(B)]
    na = h.N
    grid_b()
    xb, outb = torch.empty((B, 3, H, W), device="cuda"), h.alloc_outputs(B)
    recb, offb = torch.empty((B * h.N, 6), device="cuda"), torch.empty((B + 1,), dtype=torch.int32, device="cuda")
    heads_b = [torch.empty(s, device="cuda") for s in h.head_shapes(B)]
    nb = h.N

    def route_a():
        h.preprocess_batch(frames, geoms, SIDE, tf.mean, tf.std, out=xa)
        h.pack_detections(h.infer(xa, outa), reca, offa)

    def route_b():
        h.preprocess_batch_rect(frames, geoms, SIDE, (left, top, W, H), tf.mean, tf.std, out=xb)
        h.pack_detections(h.infer(xb, outb), recb, offb)

    result = {"tool": "rect_timing", "frames": B, "frame": [W0, H0], "side": SIDE, "window": [left, top, W, H], "pixel_ratio": round(H * W / float(SIDE * SIDE), 4),
              "predictions": {"square": na, "rect": nb, "ratio": round(nb / float(na), 4)}, "inner": args.inner, "repeats": args.repeats, "cases": []}
    for conf, nms in ((0.001, 0.5), (0.1, 0.45)):
        h.set_thresholds(conf, nms)
        for g, r in ((grid_a, route_a), (grid_b, route_b)):           # warm-up: code objects, the autotuner's timed choices, the buffers' growth
            g()
            for _ in range(3):
                r()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.repeats):                                   # alternating: whatever else shares the machine hits both
            grid_a(); ta.append(window_ms(route_a, args.inner))
            grid_b(); tb.append(window_ms(route_b, args.inner))
        kept_a, kept_b = int(offa[-1].item()), int(offb[-1].item())
        a, b = stats(ta), stats(tb)
        result["cases"].append({"conf": conf, "nms": nms, "square_ms": a, "rect_ms": b, "rect_over_square": round(b[0] / a[0], 4),
                                "kept_square": kept_a, "kept_rect": kept_b, "rect_is_faster": bool(b[0] < a[0])})
    fa, fb = [], []
    grid_a(); h.forward_raw(xa, heads_a)
    grid_b(); h.forward_raw(xb, heads_b)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        grid_a(); fa.append(window_ms(lambda: h.forward_raw(xa, heads_a), args.inner))
        grid_b(); fb.append(window_ms(lambda: h.forward_raw(xb, heads_b), args.inner))
    a, b = stats(fa), stats(fb)
    result["forward_raw"] = {"square_ms": a, "rect_ms": b, "rect_over_square": round(b[0] / a[0], 4)}
    assert h.range_status() == (False, False)
    h.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
