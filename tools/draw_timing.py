#!/usr/bin/env python3
"""Drawing detections onto frames (yn_draw_*): 32 frames of 1280x720, 20 and 300 drawn detections per frame, labels, the built-in font.

  device   Visualizer.batch on the device frames, HIP events around --inner batches, median of --repeats windows, per batch
  prims    the same call on 1x1 frames: draw_prims_kernel does the same work, draw_tile_kernel shrinks to 32 workgroups, so
           tile_share = 1 - prims / device is the tile kernel's share of the batch (the two launches' overhead counts against it)
  host     the route without the device painter: the records are read back (two copies), then a numpy slice painter inside this tool
           (strips, bar and glyph blits as array slices; the same pixels as the device route - the tool compares them and reports
           host_matches_device).  Wall clock, median.  The frame copies this route needs when the frames live on the device (download
           before, upload after) are timed on their own, to and from page-locked host buffers: frames_d2h / frames_h2d
  floor    the painted bytes (pixels the batch touches x 3), and the time two passes over them (one read, one write) take at 8.0 TB/s

Prints ONE JSON line.

    python tools/draw_timing.py [--repeats 7] [--inner 20] [--host-repeats 3]
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
from yolo_nano_amd import draw  # noqa: E402

B, W0, H0, HBM = 32, 1280, 720, 8.0e12
NAMES = ["class%02d" % i for i in range(80)]


def make_records(rng, per_frame):
    w, h = rng.uniform(40, 400, size=(B * per_frame,)), rng.uniform(40, 300, size=(B * per_frame,))
    x1, y1 = rng.uniform(-20, W0 - 40, size=w.shape), rng.uniform(-20, H0 - 40, size=w.shape)
    rec = np.stack([x1, y1, x1 + w, y1 + h, rng.uniform(0.31, 1.0, size=w.shape), rng.randint(0, 80, size=w.shape)], axis=1).astype(np.float32)
    off = (np.arange(B + 1) * per_frame).astype(np.int32)
    return rec, off


def host_paint(frame, rows, colors, font, thickness, touched=None):
    """numpy slices: the same pixels as the device route (asserted by the caller)."""
    h0, w0 = frame.shape[:2]
    gh, gw = font.shape[1:]
    a, c = thickness // 2, (thickness - 1) // 2

    def fill(xa, ya, xb, yb, color):
        xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, w0 - 1), min(yb, h0 - 1)
        if xa <= xb and ya <= yb:
            frame[ya:yb + 1, xa:xb + 1] = color
            if touched is not None:
                touched[ya:yb + 1, xa:xb + 1] = True

    for x1, y1, x2, y2, score, cls in rows:
        x1, y1, x2, y2, cls = int(x1), int(y1), int(x2), int(y2), int(cls)
        k = int(np.rint(float(score) * 100.0))
        color = colors[cls]
        if x1 + c + 1 <= x2 - c - 1 and y1 + c + 1 <= y2 - c - 1:
            fill(x1 - a, y1 - a, x2 + a, y1 + c, color); fill(x1 - a, y2 - c, x2 + a, y2 + a, color)
            fill(x1 - a, y1 - a, x1 + c, y2 + a, color); fill(x2 - c, y1 - a, x2 + a, y2 + a, color)
        else:
            fill(x1 - a, y1 - a, x2 + a, y2 + a, color)
        text = "%s: %d.%02d" % (NAMES[cls], k // 100, k % 100)
        fill(x1, y1 - gh - 1, x1 + len(text) * gw + 1, y1, color)
        for j, ch in enumerate(text):
            gx, gy = x1 + 1 + j * gw, y1 - gh
            xa, ya, xb, yb = max(gx, 0), max(gy, 0), min(gx + gw, w0), min(gy + gh, h0)
            if xa >= xb or ya >= yb:
                continue
            cov = font[ord(ch) - 32, ya - gy:yb - gy, xa - gx:xb - gx].astype(np.uint16)[:, :, None]
            dst = frame[ya:yb, xa:xb].astype(np.uint16)
            frame[ya:yb, xa:xb] = ((dst * (255 - cov) + 127) // 255).astype(np.uint8)


def median_ms(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def event_ms(fn, inner, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "draw_timing needs the GPU"
    rng = np.random.RandomState(0)
    colors = draw.class_colors(80)
    font = draw.default_font()
    vis = draw.Visualizer(NAMES, colors, vis_thresh=0.3)
    colors_u8 = np.asarray(colors, dtype=np.uint8)
    clean = [rng.randint(0, 256, size=(H0, W0, 3)).astype(np.uint8) for _ in range(B)]
    dots = [torch.zeros((1, 1, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    result = {"tool": "draw_timing", "frames": B, "frame": [W0, H0], "font_cell": [draw.GLYPH_W, draw.GLYPH_H], "cases": []}
    for per_frame in (20, 300):
        rec_h, off_h = make_records(rng, per_frame)
        rec, off = torch.from_numpy(rec_h).cuda(), torch.from_numpy(off_h).cuda()
        frames = [torch.from_numpy(f).cuda() for f in clean]
        dev = event_ms(lambda: vis.batch(frames, rec, off, None, pixels=True), args.inner, args.repeats)
        st = vis.status()
        prims = event_ms(lambda: vis.batch(dots, rec, off, None, pixels=True), args.inner, args.repeats)
        # the host route on host frames; its pixels must be the device's
        touched = np.zeros((B, H0, W0), dtype=bool)
        host_frames = [f.copy() for f in clean]

        def host_route(mark=False):
            r, o = rec.cpu().numpy(), off.cpu().numpy()
            for b in range(B):
                rows = r[o[b]:o[b + 1]]
                host_paint(host_frames[b], rows[rows[:, 4] > np.float32(0.3)], colors_u8, font, 2, touched[b] if mark else None)

        host_route(mark=True)
        same = all(np.array_equal(f.cpu().numpy(), h) for f, h in zip(frames, host_frames))
        host = median_ms(host_route, args.host_repeats)
        pinned = [torch.empty((H0, W0, 3), dtype=torch.uint8).pin_memory() for _ in range(B)]      # page-locked: the copies a tuned pipeline makes
        d2h = median_ms(lambda: [p.copy_(f, non_blocking=True) for f, p in zip(frames, pinned)], args.host_repeats)
        h2d = median_ms(lambda: [f.copy_(p, non_blocking=True) for f, p in zip(frames, pinned)], args.host_repeats)
        del pinned
        painted = int(touched.sum()) * 3
        result["cases"].append({
            "detections_per_frame": per_frame, "drawn": st["drawn"], "skipped": st["skipped"],
            "device_ms": round(dev[0], 4), "device_ms_min_max": [round(dev[1], 4), round(dev[2], 4)],
            "prims_ms": round(prims[0], 4), "tile_share": round(1.0 - prims[0] / dev[0], 3),
            "host_ms": round(host, 2), "frames_d2h_ms": round(d2h, 2), "frames_h2d_ms": round(h2d, 2),
            "frame_copies": "pinned", "host_with_copies_ms": round(host + d2h + h2d, 2),
            "device_beats_host": bool(dev[0] < host), "device_beats_host_with_copies": bool(dev[0] < host + d2h + h2d), "host_matches_device": bool(same),
            "painted_bytes": painted, "frame_bytes": B * H0 * W0 * 3, "floor_ms": round(2.0 * painted / HBM * 1e3, 5),
        })
    print(json.dumps(result))


if __name__ == "__main__":
    main()
