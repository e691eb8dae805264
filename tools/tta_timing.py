#!/usr/bin/env python3
"""Test-time augmentation timing: 32 images at 416, scales 320..640 step 32 (x flip: 22 forwards per image), COCO head, random weights.

  device  TestTimeAugmentation.batch(x, model): yn_tta_infer - per scale one resize + mirror launch, one yn_infer over the 64 images and
          one append; one read-back; one batched merge; two copies to the host
  loop    the unchanged TestTimeAugmentation.__call__ (the reference's loop: 22 serial bs = 1 forwards, F.interpolate, numpy
          concatenation, yn_nms_merge) over the same 32 images, one after the other, on the same box
  resize  tta_resize_flip_kernel alone for the eleven scales (64 output images each) against its HBM floor: input read once + output
          written once, at 8.0 TB/s

At the benchmark's conf 0.001 random weights keep about 5.6 k boxes per image and 416 forward: over these 22 forwards that is more rows per
merge list than the NMS's 131 072-row segment limit, for either route.  So conf_thresh is set from
the data: the score that --keep candidates per image exceed in a plain 416 forward (default 300); both routes run the same model, and
the merge lists' sizes are reported.  If a list does not fit --capacity the tool takes the size the failure names and starts over, once.
Wall-clock times (the loop is host-bound by construction): median over --iters runs after one warm-up run of each route (the autotuner
sees every scale at both batch sizes there).  Prints ONE JSON line.

    python tools/tta_timing.py [--iters 5] [--loop-images 32] [--capacity 16384] [--keep 300]
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
import yolo_nano_amd  # noqa: E402
from yolo_nano_amd import arch, capi, weights  # noqa: E402

N, S, C, HBM = 32, 416, 80, 8.0e12
RANGE = [320, 640, 32]


def make_model(conf):
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, trainable=False, conf_thresh=conf, nms_thresh=0.5,
                               anchor_size=arch.MULTI_ANCHOR_SIZE_COCO, backbone="1.0x")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in weights.make_state_dict("1.0x", C).items()}, strict=False)
    return m.to("cuda").eval()


def pick_conf(x, keep):
    """The score that `keep` candidates per image exceed in a plain 416 forward (yn_score_full: every candidate, no threshold, no NMS)."""
    m = make_model(0.0)
    h = m.handle(N)
    heads = [t.permute(0, 2, 3, 1).contiguous() for t in m.forward_raw(x)]
    _, cls = h.score_full(heads)                                # [B, N, C] class scores
    best = cls.max(dim=2).values.flatten()
    k = min(keep * N, best.numel() - 1)
    conf = float(torch.topk(best, k + 1).values[-1].item())
    h.close()
    m._handle = None
    return conf


def wall_ms(fn, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def resize_share(x, scales, iters):
    h = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=1)
    out = torch.empty((2 * N * 3 * scales[-1] * scales[-1],), dtype=torch.float32, device="cuda")
    per, floor_total, us_total = {}, 0.0, 0.0
    for s in scales:
        o = out[: 2 * N * 3 * s * s].view(2 * N, 3, s, s)
        for _ in range(5):
            h.resize_batch(x, s, True, out=o)
        times = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                h.resize_batch(x, s, True, out=o)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / 20)
        us = float(np.median(times))
        floor = (N * 3 * S * S * 4 + 2 * N * 3 * s * s * 4) / HBM * 1e6
        per[str(s)] = {"us": round(us, 1), "floor_us": round(floor, 1), "floor_share": round(floor / us, 3)}
        floor_total += floor
        us_total += us
    h.close()
    return {"us_all_scales": round(us_total, 1), "hbm_floor_us": round(floor_total, 1), "floor_share": round(floor_total / us_total, 3), "per_scale": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--loop-images", type=int, default=N, help="images the __call__ loop is timed over (scaled to 32 in the result)")
    ap.add_argument("--capacity", type=int, default=16384)
    ap.add_argument("--keep", type=int, default=300)
    a = ap.parse_args()
    x = torch.from_numpy(weights.make_input(N, S, seed=3)).cuda()
    conf = pick_conf(x, a.keep)
    model = make_model(conf)
    tta = yolo_nano_amd.TestTimeAugmentation(num_classes=C, nms_thresh=0.4, scale_range=RANGE)
    scales = [int(s) for s in tta.scales]
    tta.list_capacity = a.capacity
    res = {"images": N, "size": S, "scales": scales, "forwards_per_image": 2 * len(scales), "conf_thresh": conf, "nms_thresh": 0.4}
    try:
        dets = tta.batch(x, model)                              # warm-up run (autotune at bs 64, every scale)
    except capi.YnError as e:
        if "list_capacity" not in str(e):
            raise
        need = int(tta._tta.forwards_to_host(N)[3].max())
        if need > 131072:
            print(json.dumps(dict(res, error=str(e))))
            return 1
        tta.list_capacity = (need + 1023) // 1024 * 1024
        dets = tta.batch(x, model)
    counts = tta._tta.forwards_to_host(N)[3]
    res["list_capacity"] = int(tta.list_capacity)
    res["list_rows"] = {"mean": round(float(counts.mean()), 1), "max": int(counts.max())}
    res["merged_per_image"] = round(float(np.mean([len(d[1]) for d in dets])), 1)
    med, mn = wall_ms(lambda: tta.batch(x, model), a.iters)
    res["device_ms_per_batch"] = round(med, 2)
    res["device_ms_min"] = round(mn, 2)
    # the unchanged loop; a model of its own, so that its bs = 1 handle is the one the reference's caller would hold
    loop_model = make_model(conf)
    n_loop = max(1, min(N, a.loop_images))
    loop = lambda: [tta(x[i:i + 1], loop_model) for i in range(n_loop)]
    first = loop()                                              # warm-up run (autotune at bs 1, every scale)
    res["loop_merged_per_image"] = round(float(np.mean([len(d[1]) for d in first])), 1)
    med, mn = wall_ms(loop, max(1, a.iters // 2))
    res["loop_ms_per_batch"] = round(med * N / n_loop, 2)
    res["loop_ms_min"] = round(mn * N / n_loop, 2)
    res["loop_images_timed"] = n_loop
    res["speedup"] = round(res["loop_ms_per_batch"] / res["device_ms_per_batch"], 2)
    res["resize"] = resize_share(x, scales, a.iters)
    res["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
