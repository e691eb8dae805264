#!/usr/bin/env python3
"""JPEG encode (yn_jpeg_enc_* / yn_jpeg_encode_*): 32 frames of 640x480 (what tests/golden/jpeg_bench.jpg decodes to) per batch, quality 95,
4:2:0.

  batch_ms     encode of one batch on the device, HIP events from before the table upload to after the last kernel
  kernel_us    the same per stage (yn_jpeg_enc_timing): table upload + clearing the stream, fdct, bits, the two scans with their layout
               kernels, emit, 0xFF count, files
  floor        the bytes the chain has to move (frames read once: 3 per pixel; int16 coefficients written once and read twice: 9 per pixel at
               4:2:0; the stream cleared once; the unstuffed bytes written, read twice, and the files written: 4 x file bytes) at 8.0 TB/s, and
               that time's share of batch_ms
  ratio        file bytes against frame bytes: what crosses PCIe against what a host encoder would need
  fetch_ms     yn_jpeg_encode_fetch into pinned memory (offsets + files), wall clock; it synchronises
  e2e          frames/s over --batches batches of encode + fetch, back to back
  pil          when PIL is importable: PIL saves of the same frame per second at 1 and 16 threads, and the pinned download of the 32 frames -
               the host route this feature replaces; e2e_16 = 32 / (download + 32 / rate_16)
The 32 frames are the SAME pixels.  All medians of --repeats.  Prints ONE JSON line.

    python tools/jpeg_encode_timing.py [--repeats 7] [--batches 20]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_nano_amd import jpeg  # noqa: E402

B, HBM, QUALITY = 32, 8.0e12, 95


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, default=20)
    a = ap.parse_args()
    frame = jpeg.imread(os.path.join(ROOT, "tests", "golden", "jpeg_bench.jpg"))
    h, w = int(frame.shape[0]), int(frame.shape[1])
    frames = [frame.clone() for _ in range(B)]
    enc = jpeg.JPEGEncoder(max_batch=B, quality=QUALITY, sampling="4:2:0")
    files = enc.batch(frames)                                 # grows the buffers; the timed calls below do not
    file_bytes = sum(len(f) for f in files)
    assert len(set(files)) == 1 and files[0][:2] == b"\xff\xd8" and files[0][-2:] == b"\xff\xd9"
    res = {"tool": "jpeg_encode_timing", "device": torch.cuda.get_device_name(0), "images": B, "w": w, "h": h, "quality": QUALITY,
           "sampling": "4:2:0", "identical_frames": True, "file_bytes": file_bytes, "frame_bytes": B * h * w * 3,
           "file_to_frame": round(file_bytes / (B * h * w * 3), 4), "stream_bytes": enc.stream_bytes}
    stages, total, fetch = [], [], []
    for i in range(a.repeats + 1):
        enc.encode(frames)
        t = enc.timing()
        t0 = time.perf_counter()
        enc.fetch()
        if i:
            fetch.append((time.perf_counter() - t0) * 1e3)
            stages.append(t)
            total.append(sum(t.values()))
    moved = B * h * w * 12 + enc.stream_bytes + 4 * file_bytes
    res.update({"batch_ms": round(med(total), 4), "kernel_us": {k: round(med([s[k] for s in stages]) * 1e3, 1) for k in stages[0]},
                "moved_bytes": moved, "floor_us": round(moved / HBM * 1e6, 2), "floor_share": round(moved / HBM * 1e3 / med(total), 4),
                "fetch_ms": round(med(fetch), 3)})
    rates = []
    for _ in range(max(a.repeats // 2, 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.batches):
            enc.encode(frames)
            enc.fetch()
        rates.append(a.batches * B / (time.perf_counter() - t0))
    res["e2e_images_s"] = round(med(rates), 1)
    enc.close()
    try:
        import io
        from PIL import Image
    except ImportError:
        res["pil"] = None
    else:
        rgb = np.ascontiguousarray(frame.cpu().numpy()[..., ::-1])

        def one(_):
            b = io.BytesIO()
            Image.fromarray(rgb).save(b, "JPEG", quality=QUALITY, subsampling=2)
            return b.getvalue()
        res["equals_pil"] = one(0) == files[0]
        out = {}
        for threads in (1, 16):
            with ThreadPoolExecutor(threads) as ex:
                rates = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    list(ex.map(one, range(B * (2 if threads > 1 else 1))))
                    rates.append(B * (2 if threads > 1 else 1) / (time.perf_counter() - t0))
            out["save_images_s_%d" % threads] = round(med(rates), 1)
        src = torch.stack(frames)
        pinned = torch.empty((B, h, w, 3), dtype=torch.uint8).pin_memory()
        downs = []
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); pinned.copy_(src, non_blocking=True); e1.record(); e1.synchronize()
            downs.append(e0.elapsed_time(e1))
        out["frames_d2h_ms"] = round(med(downs[1:]), 3)
        out["e2e_images_s_16"] = round(B / (med(downs[1:]) / 1e3 + B / out["save_images_s_16"]), 1)
        res["pil"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
