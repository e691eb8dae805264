#!/usr/bin/env python3
"""Cutting detections out of frames as chips (yn_chip_*): 32 frames of 1280x720, 20 and 300 seeded detections per frame as
tools/draw_timing.py makes them, two configurations: 128x256 u8 stretch chips and 224x224 f32 letterbox chips.

  device   ChipExtractor.batch on the device frames, HIP events around --inner batches, median of --repeats windows, per batch
  select   the same call with max_chips = 1: the selection, the scan and one chip's resampling, so resample_share = 1 - select / device is
           the resample kernel's share of the batch (the launches' overhead counts against it)
  glue     the route from the public calls without the chip object: offsets and records read back, host geometry (the rule of DESIGN 32
           in Python integers), one torch slice + .contiguous() per box, yn_preprocess_batch over the slices (chunks of 1024).  Wall
           clock, median.  For the f32 letterbox case its output must be the device's, bit for bit (same_bits); for the u8 stretch case
           the public calls have no u8 output: the glue writes the stretched picture into a float32 256x256 square (more bytes, the
           same crops) and nothing is compared
  host     the numpy restatement (the crop + the cv2 8-bit resize per box) on --host-frames frames, scaled to the batch, plus the frame
           copies down (page-locked), which are also given alone: frames_d2h
  floor    the larger of two times: data movement (the source rectangles' bytes touched once + the chip bytes written, at 8.0 TB/s)
           and compute (operations per output pixel, counted from the kernel's linear path, times the pixels, at the VALU's unpacked
           issue rate); floor_share = floor / resample time and floor_bound names the larger

Prints ONE JSON line.

    python tools/chip_timing.py [--repeats 7] [--inner 20] [--glue-repeats 3] [--host-frames 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from yolo_nano_amd import arch, capi, chips  # noqa: E402
from oracle.preprocess import cv2_resize_linear_u8  # noqa: E402  (the host restatement's resize)
import draw_timing  # noqa: E402  (the seeded detections)

B, W0, H0, HBM = draw_timing.B, draw_timing.W0, draw_timing.H0, 8.0e12
VALU = 157.3e12 / 2.0                                          # unpacked vector operations per second: the FP32 vector peak counts an FMA as two
# per output pixel of the linear path, per channel: 4 multiplies + 2 adds (horizontal), 2 shifts, 2 multiplies, 2 shifts, 2 adds, 1 shift,
# 2 clamps = 17; x 3 channels; + 8 address / table operations; f32: + convert, divide, subtract, divide per channel; u8: + 2 per channel to pack
OPS_U8, OPS_F32 = 17 * 3 + 8 + 2 * 3, 17 * 3 + 8 + 4 * 3
CONFIGS = [dict(name="u8_stretch_128x256", size=(128, 256), fit="stretch", out="u8"), dict(name="f32_letterbox_224x224", size=(224, 224), fit="letterbox", out="f32")]


def host_rects(rec, off, cfg):
    """The rule of DESIGN 32 at margin 0 for in-range classes: -> [(frame, x, y, sw, sh, rw, rh, left, top)] in record order."""
    cw, ch = cfg["size"]
    out = []
    for b in range(B):
        for r in rec[off[b]:off[b + 1]]:
            if not r[4] > np.float32(0.3):
                continue
            X1, Y1, X2, Y2 = (int(v) for v in r[:4])
            xa, ya, xb, yb = max(X1, 0), max(Y1, 0), min(X2, W0 - 1), min(Y2, H0 - 1)
            sw, sh = xb - xa + 1, yb - ya + 1
            if X2 < X1 or Y2 < Y1 or sw < 2 or sh < 2:
                continue
            rw, rh, left, top = cw, ch, 0, 0
            if cfg["fit"] == "letterbox":
                if sh * cw > sw * ch:
                    rw = int(float(sw) / float(sh) * float(ch))
                    left = (cw - rw) // 2
                elif sh * cw < sw * ch:
                    rh = int(float(sh) / float(sw) * float(cw))
                    top = (ch - rh) // 2
            if rw and rh:
                out.append((b, xa, ya, sw, sh, rw, rh, left, top))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--glue-repeats", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "chip_timing needs the GPU"
    rng = np.random.RandomState(0)
    h = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", device=torch.device("cuda", torch.cuda.current_device()))
    clean = [rng.randint(0, 256, size=(H0, W0, 3)).astype(np.uint8) for _ in range(B)]
    frames = [torch.from_numpy(f).cuda() for f in clean]
    pinned = [torch.empty((H0, W0, 3), dtype=torch.uint8).pin_memory() for _ in range(B)]
    d2h = draw_timing.median_ms(lambda: [p.copy_(f, non_blocking=True) for f, p in zip(frames, pinned)], 3)
    del pinned
    result = {"tool": "chip_timing", "frames": B, "frame": [W0, H0], "hbm_bytes_per_s": HBM, "valu_ops_per_s": VALU, "frames_d2h_ms": round(d2h, 2), "cases": []}
    for per_frame in (20, 300):
        rec_h, off_h = draw_timing.make_records(np.random.RandomState(per_frame), per_frame)
        rec, off = torch.from_numpy(rec_h).cuda(), torch.from_numpy(off_h).cuda()
        for cfg in CONFIGS:
            cw, ch = cfg["size"]
            cut = chips.ChipExtractor(size=cfg["size"], fit=cfg["fit"], out=cfg["out"], min_score=0.3, min_side=2, max_chips=B * per_frame, num_classes=80, handle=h)
            one = chips.ChipExtractor(size=cfg["size"], fit=cfg["fit"], out=cfg["out"], min_score=0.3, min_side=2, max_chips=1, num_classes=80, handle=h)
            dev = draw_timing.event_ms(lambda: cut.batch(frames, rec, off, None, pixels=True), args.inner, args.repeats)
            sel = draw_timing.event_ms(lambda: one.batch(frames, rec, off, None, pixels=True), args.inner, args.repeats)
            got, index, _, rects = cut.batch(frames, rec, off, None, pixels=True)
            st = cut.status()
            n = st["chips"]

            # the glue from the public calls
            side = max(cw, ch)

            def glue():
                r, o = rec.cpu().numpy(), off.cpu().numpy()
                todo = host_rects(r, o, cfg)
                outs = []
                for c0 in range(0, len(todo), 1024):
                    part = todo[c0:c0 + 1024]
                    crops = [frames[b][y:y + sh, x:x + sw].contiguous() for b, x, y, sw, sh, _, _, _, _ in part]
                    if cfg["fit"] == "letterbox":
                        geoms = [(rw, rh, left, top) for _, _, _, _, _, rw, rh, left, top in part]
                    else:
                        geoms = [(cw, ch, (side - cw) // 2, (side - ch) // 2)] * len(part)
                    outs.append(h.preprocess_batch(crops, geoms, side, chips.DEFAULT_MEAN, chips.DEFAULT_STD))
                return outs, todo

            outs, todo = glue()
            same = None
            if cfg["fit"] == "letterbox":
                same = bool(len(todo) == n and all(torch.equal(o.view(torch.int32), got[k * 1024:k * 1024 + len(o)].view(torch.int32)) for k, o in enumerate(outs)))
            del outs
            glue_ms = draw_timing.median_ms(glue, args.glue_repeats)

            # the numpy restatement on a few frames, scaled
            few = [t for t in todo if t[0] < args.host_frames]

            def host():
                for b, x, y, sw, sh, rw, rh, _, _ in few:
                    cv2_resize_linear_u8(np.ascontiguousarray(clean[b][y:y + sh, x:x + sw]), (rw, rh))

            host_ms = draw_timing.median_ms(host, 1) * len(todo) / max(len(few), 1)

            src = sum(sw * sh * 3 for _, _, _, sw, sh, _, _, _, _ in todo)
            dst = n * cw * ch * 3 * (1 if cfg["out"] == "u8" else 4)
            ops = n * cw * ch * (OPS_U8 if cfg["out"] == "u8" else OPS_F32)
            move_ms, compute_ms = (src + dst) / HBM * 1e3, ops / VALU * 1e3
            floor_ms = max(move_ms, compute_ms)
            resample_ms = max(dev[0] - sel[0], 1e-6)
            result["cases"].append({
                "config": cfg["name"], "detections_per_frame": per_frame, "chips": n, "skipped": st["skipped"], "overflow": st["overflow"],
                "device_ms": round(dev[0], 4), "device_ms_min_max": [round(dev[1], 4), round(dev[2], 4)], "select_ms": round(sel[0], 4),
                "resample_share": round(1.0 - sel[0] / dev[0], 3), "glue_ms": round(glue_ms, 2), "same_bits": same,
                "host_ms_scaled": round(host_ms, 1), "host_boxes_measured": len(few), "host_with_copies_ms": round(host_ms + d2h, 1),
                "device_beats_glue": bool(dev[0] < glue_ms), "device_beats_host_with_copies": bool(dev[0] < host_ms + d2h),
                "device_beats_copies_alone": bool(dev[0] < d2h),
                "source_bytes": src, "chip_bytes": dst, "move_floor_ms": round(move_ms, 5), "ops": ops, "compute_floor_ms": round(compute_ms, 5),
                "floor_ms": round(floor_ms, 5), "floor_bound": "compute" if compute_ms > move_ms else "data movement",
                "floor_share": round(floor_ms / resample_ms, 4),
            })
            cut.close()
            one.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
