#!/usr/bin/env python3
"""JPEG decode, entropy stage on the host against entropy stage on the device (yn_jpeg_entropy), in ONE run on one machine:
32 files per batch, once 32 copies of tests/golden/jpeg_bench.jpg (640x480, 4:2:0, quality 90), once 32 different files (the bench frame
written again by imencode at qualities 60..95).

  per case, per mode ("host", "device"), per worker count (1, 4, 16):
    host_ms        the host's share of one batch, wall clock inside the library (host: headers + Huffman decode; device: headers + the copy
                   pass, plus any file the host decoded after all)
    upload_bytes   what goes up per batch (host: int16 coefficients; device: the unstuffed scans), upload_ms its copy (HIP events)
    kernel_us      device mode: clear, jpeg_huff_first_kernel, jpeg_huff_sync_kernel, jpeg_huff_write_kernel, jpeg_huff_dc_kernel; both: the two pixel kernels
    rounds         device mode: the most rounds a file of the batch needed; decodes_per_subseq: subsequence decodes of the synchronisation
                   per subsequence (1 = a serial decoder's work); host_files: files that fell back (0 unless something is wrong)
    e2e_images_s   images/s over --batches batches issued back to back, one synchronisation at the end
  sweep            device mode at --threads workers on the bench batch, subseq_bits 256 .. 4096: sync_us, rounds, decodes_per_subseq, e2e
The yardstick of the device mode is the host mode's e2e_images_s at the same worker count in the same run.  All medians of --repeats.
Prints ONE JSON line.

    python tools/jpeg_entropy_timing.py [--repeats 7] [--batches 20] [--subseq-bits N] [--max-rounds N]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_nano_amd import jpeg  # noqa: E402

B = 32


def med(v):
    return float(np.median(v))


def measure(blobs, frames, mode, threads, repeats, batches, staging, bits=None, rounds=None, e2e=True):
    dec = jpeg.JPEGDecoder(max_batch=B, threads=threads, staging_bytes=staging, entropy=mode, subseq_bits=bits, max_rounds=rounds, handle=jpeg._decoder()._h())
    host, h2d, pix, ent = [], [], [], []
    for i in range(repeats + 1):
        status, failed = dec.decode_into(blobs, frames)
        assert failed == 0
        t = dec.timing()
        e = dec.entropy_timing() if mode == "device" else None
        if i:
            host.append(t["host_ms"]); h2d.append(t["h2d_ms"]); pix.append(t["kernel_ms"]); ent.append(e)
    out = {"host_ms": round(med(host), 3), "pixel_kernels_us": round(med(pix) * 1e3, 1)}
    if mode == "device":
        st = dec.entropy_stats()
        out.update({"upload_bytes": sum(-(-len(jpeg.scan_prepare(b)["scan"]) // 16) * 16 for b in blobs),
                    "upload_ms": round(med([e["upload_ms"] for e in ent]), 3),
                    "kernel_us": {k[:-3]: round(med([e[k] for e in ent]) * 1e3, 1) for k in ("clear_ms", "first_ms", "sync_ms", "write_ms", "dc_ms")},
                    "rounds": st["rounds_last"], "subseqs": st["subseqs_last"],
                    "decodes_per_subseq": round(med([e["decodes_per_subseq"] for e in ent]), 3), "host_files": st["host_files"]})
    else:
        out.update({"upload_bytes": sum(2 * jpeg.coefficient_count(jpeg.info(b)) for b in blobs), "upload_ms": round(med(h2d), 3)})
    if e2e:
        rates = []
        for _ in range(max(repeats // 2, 1)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batches):
                dec.decode_into(blobs, frames)
            torch.cuda.synchronize()
            rates.append(batches * B / (time.perf_counter() - t0))
        out["e2e_images_s"] = round(med(rates), 1)
    dec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16, help="workers of the sweep")
    ap.add_argument("--subseq-bits", type=int, default=None)
    ap.add_argument("--max-rounds", type=int, default=None)
    ap.add_argument("--no-sweep", action="store_true")
    a = ap.parse_args()
    blob = open(os.path.join(ROOT, "tests", "golden", "jpeg_bench.jpg"), "rb").read()
    want = str(np.load(os.path.join(ROOT, "tests", "golden", "jpeg.npz"))["bench_md5"])
    meta = jpeg.info(blob)
    h, w = meta["h"], meta["w"]
    frames = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(B)]
    staging = 2 * jpeg.coefficient_count(meta) * B
    frame = jpeg.imread(blob)
    assert hashlib.md5(frame.cpu().numpy().tobytes()).hexdigest() == want
    qualities = [60 + (35 * i) // (B - 1) for i in range(B)]
    different = [jpeg.imencode(frame, quality=q) for q in qualities]
    res = {"tool": "jpeg_entropy_timing", "device": torch.cuda.get_device_name(0), "images": B, "w": w, "h": h, "repeats": a.repeats, "batches": a.batches,
           "subseq_bits": a.subseq_bits or "default", "max_rounds": a.max_rounds or "default"}
    for case, blobs in (("bench_x32", [blob] * B), ("requantised_q60_95", different)):
        block = {"file_bytes": sum(len(b) for b in blobs)}
        for mode in ("host", "device"):
            for threads in (1, 4, 16):
                block["%s_%d" % (mode, threads)] = measure(blobs, frames, mode, threads, a.repeats, a.batches, staging, a.subseq_bits, a.max_rounds)
        if case == "bench_x32":
            assert hashlib.md5(frames[B - 1].cpu().numpy().tobytes()).hexdigest() == want, "the device mode's frame differs from the recorded digest"
        block["device_over_host_16"] = round(block["device_16"]["e2e_images_s"] / block["host_16"]["e2e_images_s"], 3)
        res[case] = block
    if not a.no_sweep:
        sweep = {}
        for bits in (256, 512, 1024, 2048, 4096):
            m = measure([blob] * B, frames, "device", a.threads, a.repeats, a.batches, staging, bits, a.max_rounds)
            sweep[str(bits)] = {"first_us": m["kernel_us"]["first"], "sync_us": m["kernel_us"]["sync"], "write_us": m["kernel_us"]["write"], "rounds": m["rounds"],
                                "decodes_per_subseq": m["decodes_per_subseq"], "host_files": m["host_files"], "e2e_images_s": m["e2e_images_s"]}
        res["sweep_bench_x32"] = sweep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
