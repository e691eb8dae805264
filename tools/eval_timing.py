#!/usr/bin/env python3
"""VOC mAP timing (yn_eval_*): a VOC07-sized synthetic workload (4952 images, ~2.4 ground-truth boxes each, detections built on the
device) at 100 and 3600 detections per image, batches of 32.  Times the adds + yn_eval_finish (11-point) after one warm-up pass,
and the host routes on a subset of the same detections: the stable oracle on the ingested records (tests/voc_oracle.py) and the
reference-style route (the results-file text written and parsed back, then the per-detection loop).  Prints one JSON line.

    python tools/eval_timing.py [--images 4952] [--subset 20000]
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
from yolo_nano_amd import VOCEval, voc_geometry  # noqa: E402
import voc_oracle  # noqa: E402

C, SIDE, BATCH = 20, 416, 32


def workload(n_img, per_img, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    shapes = [(375, 500), (500, 375), (333, 500), (500, 500)]
    geoms = [voc_geometry(*shapes[i % 4], SIDE) for i in range(n_img)]
    gts = []
    for i in range(n_img):
        h0, w0 = shapes[i % 4]
        m = int(rng.integers(0, 6))
        x1, y1 = rng.integers(0, w0 - 80, m), rng.integers(0, h0 - 80, m)
        gts.append(np.stack([x1, y1, x1 + rng.integers(10, 80, m), y1 + rng.integers(10, 80, m), rng.integers(0, C, m),
                             (rng.random(m) < 0.1).astype(int)], 1).astype(np.int32).reshape(-1, 6))
    batches = []
    for s in range(0, n_img, BATCH):
        B = min(BATCH, n_img - s)
        n = B * per_img
        xy = torch.rand((n, 2), generator=g, device="cuda") * 0.9
        wh = torch.rand((n, 2), generator=g, device="cuda") * 0.3
        rec = torch.cat([xy, xy + wh, torch.rand((n, 1), generator=g, device="cuda"),
                         torch.randint(0, C, (n, 1), generator=g, device="cuda").float()], 1).contiguous()
        off = (torch.arange(B + 1, device="cuda", dtype=torch.int32) * per_img).contiguous()
        batches.append((rec, off, geoms[s:s + B], gts[s:s + B]))
    return batches


def device_time(ev, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.reset()
    for rec, off, geoms, gts in batches:
        ev.add(rec, off, geoms, gts)
    aps, m = ev.compute(True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, aps, m


def host_times(batches, subset):
    """seconds per detection of (stable oracle on records, reference-style text route + loop) on the first `subset` detections"""
    boxes, scores, classes, offs, geoms, gts = [], [], [], [0], [], []
    for rec, off, gm, gt in batches:
        r = rec.cpu().numpy()
        o = off.cpu().numpy()
        for b in range(len(gm)):
            if offs[-1] >= subset:
                break
            boxes.append(r[o[b]:o[b + 1], :4]); scores.append(r[o[b]:o[b + 1], 4]); classes.append(r[o[b]:o[b + 1], 5].astype(np.int64))
            offs.append(offs[-1] + int(o[b + 1] - o[b])); geoms.append(gm[b]); gts.append(gt[b])
    n = offs[-1]
    gt = np.concatenate(gts)
    gt_off = np.cumsum([0] + [len(x) for x in gts])
    t0 = time.perf_counter()
    recs = voc_oracle.ingest(np.concatenate(boxes), np.concatenate(scores), np.concatenate(classes), offs, geoms)
    t1 = time.perf_counter()
    voc_oracle.voc_metric(recs, gt, gt_off, C, 0.5, True)
    t2 = time.perf_counter()
    return n, (t2 - t1) / n, (t2 - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--subset", type=int, default=20000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_timing: needs a GPU")
    ev = VOCEval(C)
    out = {"images": a.images}
    for per_img in (100, 3600):
        batches = workload(a.images, per_img, seed=per_img)
        device_time(ev, batches)                                   # warm-up: code objects, allocations at this size
        t, aps, m = min((device_time(ev, batches) for _ in range(3)), key=lambda r: r[0])
        n_host, oracle_s, ref_s = host_times(batches, a.subset)
        total = a.images * per_img
        out["d%d" % per_img] = {"detections": total, "device_s": round(t, 4), "mAP07": float(m),
                                "host_subset": n_host, "oracle_us_per_det": round(oracle_s * 1e6, 2),
                                "reference_route_us_per_det": round(ref_s * 1e6, 2),
                                "speedup_vs_reference_route": round(ref_s * total / t, 1)}
        del batches
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
