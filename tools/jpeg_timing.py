#!/usr/bin/env python3
"""JPEG decode (yn_jpeg_*): 32 copies of tests/golden/jpeg_bench.jpg (640x480, 4:2:0, quality 90) per batch.

  host_ms      the host stage of one batch (headers + Huffman decode into the pinned slot), wall clock inside the library, at 1 worker and
               at --threads workers.  The 32 files are the SAME bytes: the input stays in cache, which flatters this number a little
               (the output, 29 MB of coefficients per batch, does not fit any cache)
  h2d_ms       the upload of the batch's int16 coefficients + descriptor table (HIP events)
  kernel_us    jpeg_idct_kernel + jpeg_color_kernel for the batch (HIP events)
  floor        the bytes the two kernels move (coefficients read, planes written and read, frames written: 9 bytes per pixel at 4:2:0) at
               8.0 TB/s, and that time's share of kernel_us
  e2e          images/s over --batches batches issued back to back (two staging slots: the host decodes batch k+1 while batch k uploads
               and runs), one synchronisation at the end
  pil          when PIL is importable: PIL decodes of the same file per second at 1 and 16 threads, and the pinned upload of the 32 decoded
               frames - the host route this feature replaces
All medians of --repeats.  Prints ONE JSON line.

    python tools/jpeg_timing.py [--repeats 7] [--threads 16] [--batches 20]
"""
import argparse
import hashlib
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

B, HBM = 32, 8.0e12


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--threads", type=int, default=min(16, int(os.environ.get("OMP_NUM_THREADS", 8))))
    ap.add_argument("--batches", type=int, default=20)
    a = ap.parse_args()
    blob = open(os.path.join(ROOT, "tests", "golden", "jpeg_bench.jpg"), "rb").read()
    want = str(np.load(os.path.join(ROOT, "tests", "golden", "jpeg.npz"))["bench_md5"])
    meta = jpeg.info(blob)
    h, w = meta["h"], meta["w"]
    blobs = [blob] * B
    coef_bytes = 2 * jpeg.coefficient_count(meta) * B
    frames = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    res = {"tool": "jpeg_timing", "device": torch.cuda.get_device_name(0), "images": B, "w": w, "h": h, "file_bytes": len(blob),
           "sampling": "%dx%d" % (meta["h_samp"], meta["v_samp"]), "threads": a.threads, "identical_files": True,
           "note": "the 32 files are the same bytes: the input side of the host stage runs from cache"}
    for name, threads in (("1", 1), ("n", a.threads)):
        dec = jpeg.JPEGDecoder(max_batch=B, threads=threads, staging_bytes=coef_bytes)
        host, h2d, kern = [], [], []
        for i in range(a.repeats + 1):
            status, failed = dec.decode_into(blobs, frames)
            assert failed == 0
            t = dec.timing()
            if i:
                host.append(t["host_ms"]); h2d.append(t["h2d_ms"]); kern.append(t["kernel_ms"])
        res["host_ms_%s" % ("1_thread" if name == "1" else "threads")] = round(med(host), 3)
        if name == "n":
            assert hashlib.md5(frames[B - 1].cpu().numpy().tobytes()).hexdigest() == want, "the decoded frame differs from PIL's"
            moved = B * h * w * 9
            res.update({"coef_bytes": coef_bytes, "h2d_ms": round(med(h2d), 3), "h2d_gb_s": round(coef_bytes / med(h2d) / 1e6, 1),
                        "kernel_us": round(med(kern) * 1e3, 1), "kernel_bytes": moved, "floor_us": round(moved / HBM * 1e6, 2),
                        "floor_share": round(moved / HBM * 1e3 / med(kern), 4)})
            rates = []
            for _ in range(max(a.repeats // 2, 1)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.batches):
                    dec.decode_into(blobs, frames)
                torch.cuda.synchronize()
                rates.append(a.batches * B / (time.perf_counter() - t0))
            res["e2e_images_s"] = round(med(rates), 1)
        dec.close()
    try:
        import io
        from PIL import Image
    except ImportError:
        res["pil"] = None
    else:
        def one(_):
            return np.asarray(Image.open(io.BytesIO(blob)))[..., ::-1]
        out = {}
        for threads in (1, 16):
            with ThreadPoolExecutor(threads) as ex:
                rates = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    list(ex.map(one, range(B * (2 if threads > 1 else 1))))
                    rates.append(B * (2 if threads > 1 else 1) / (time.perf_counter() - t0))
            out["decode_images_s_%d" % threads] = round(med(rates), 1)
        pinned = torch.empty((B, h, w, 3), dtype=torch.uint8).pin_memory()
        dst = torch.empty((B, h, w, 3), dtype=torch.uint8, device="cuda")
        ups = []
        for _ in range(a.repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(pinned, non_blocking=True); e1.record(); e1.synchronize()
            ups.append(e0.elapsed_time(e1))
        out["frames_h2d_ms"] = round(med(ups[1:]), 3)
        out["frame_bytes"] = B * h * w * 3
        res["pil"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
