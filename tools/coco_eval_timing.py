#!/usr/bin/env python3
"""COCO box AP timing (yn_coco_*): a val2017-sized synthetic workload (5000 images, ~7 ground-truth boxes each, 80 categories,
detections built on the device) at 100 and 5600 detections per image (what conf 0.001 keeps with random weights), batches of 32.
Times the adds + yn_coco_finish + the host summarize after one warm-up pass (best of three, adds and finish also apart), and the
host restatement tests/coco_oracle.py on a subset of the same detections, per detection.  Prints one JSON line.

    python tools/coco_eval_timing.py [--images 5000] [--subset 20000]
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
from yolo_nano_amd import COCOEval, voc_geometry  # noqa: E402
import coco_oracle  # noqa: E402

C, SIDE, BATCH = 80, 416, 32


def workload(n_img, per_img, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    shapes = [(480, 640), (640, 480), (427, 640), (500, 500)]
    geoms = [voc_geometry(*shapes[i % 4], SIDE) for i in range(n_img)]
    ids = [int(v) for v in rng.permutation(600000)[:n_img]]
    gts = []
    for i in range(n_img):
        h0, w0 = shapes[i % 4]
        m = int(rng.integers(0, 15))
        w, h = rng.uniform(8, 200, m), rng.uniform(8, 200, m)
        gts.append(np.stack([rng.uniform(0, w0 - 200, m), rng.uniform(0, h0 - 200, m), w, h, w * h * rng.uniform(0.4, 1.0, m),
                             rng.integers(0, C, m), rng.random(m) < 0.05], 1).astype(np.float64).reshape(-1, 7))
    batches = []
    for s in range(0, n_img, BATCH):
        B = min(BATCH, n_img - s)
        n = B * per_img
        xy = torch.rand((n, 2), generator=g, device="cuda") * 0.8 + 0.05
        wh = torch.rand((n, 2), generator=g, device="cuda") * 0.3
        rec = torch.cat([xy, xy + wh, torch.rand((n, 1), generator=g, device="cuda"),
                         torch.randint(0, C, (n, 1), generator=g, device="cuda").float()], 1).contiguous()
        off = (torch.arange(B + 1, device="cuda", dtype=torch.int32) * per_img).contiguous()
        batches.append((rec, off, geoms[s:s + B], ids[s:s + B], gts[s:s + B]))
    return batches


def device_time(ev, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.reset()
    for rec, off, geoms, ids, gts in batches:
        ev.add(rec, off, geoms, ids, gts)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    stats = ev.compute()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, t2 - t1, stats


def host_time(batches, subset):
    """seconds per detection of the host restatement (ingest + evaluate + accumulate + summarize) on the first images that hold at
    most `subset` detections"""
    images, n = [], 0
    for rec, off, gm, ids, gt in batches:
        r = rec.cpu().numpy()
        o = off.cpu().numpy()
        for b in range(len(gm)):
            if images and n + int(o[b + 1] - o[b]) > subset:
                break
            images.append((ids[b], gt[b], (r[o[b]:o[b + 1], :4], r[o[b]:o[b + 1], 4], r[o[b]:o[b + 1], 5].astype(np.int64)), gm[b]))
            n += int(o[b + 1] - o[b])
        else:
            continue
        break
    t0 = time.perf_counter()
    coco_oracle.coco_eval([coco_oracle.image_from_arrays(*im) for im in images], C)
    return n, (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--subset", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_timing: needs a GPU")
    ev = COCOEval(C)
    out = {"gpu": torch.cuda.get_device_name(0), "images": a.images}
    for per_img in (100, 5600):
        batches = workload(a.images, per_img, seed=per_img)
        device_time(ev, batches)                                   # warm-up: code objects, allocations at this size
        t, t_add, t_fin, stats = min((device_time(ev, batches) for _ in range(3)), key=lambda r: r[0])
        n_host, oracle_s = host_time(batches, a.subset)
        total = a.images * per_img
        out["d%d" % per_img] = {"detections": total, "kept": ev.size()[0], "device_s": round(t, 4), "adds_s": round(t_add, 4),
                                "finish_s": round(t_fin, 4), "AP": float(stats[0]), "AP50": float(stats[1]), "host_subset": n_host,
                                "oracle_us_per_det": round(oracle_s * 1e6, 2), "speedup_vs_oracle": round(oracle_s * total / t, 1)}
        del batches
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
