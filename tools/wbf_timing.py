#!/usr/bin/env python3
"""Weighted box fusion timing on the merge lists of the two workloads the other tools measure:

  tta    32 images at 416, scales 320..640 step 32 x flip (22 forwards per image; tools/tta_timing.py's model and conf_thresh), E = 22
  slice  32 frames of 1280 x 720, tile 416, overlap 0.2, full frame on (tools/slice_timing.py's model and conf_thresh), E = 1

Per workload the lists of one run are taken to the host once and put into a yn_fuse object, so that both rules merge the SAME lists:

  merge        yn_fuse_merge alone (one read-back of the state words, the merge, the pack) with YN_MERGE_WBF against YN_MERGE_NMS: device
               time between two events around --reps calls, mean and min / max over --iters such regions
  host route   what a user without the kernel does: the lists to the host, tests/wbf_oracle.py there, the result back up - the copies
               alone (pinned buffers, timed like the merge) and the oracle's wall time (one run: it is numpy row by row)
  records      the whole records() batch of the workload's object with either rule, wall clock, median and min over --iters runs
  lists        rows, clusters and mean votes per list, and same_bits: the device's records against the oracle's

Prints ONE JSON line.

    python tools/wbf_timing.py [--workload tta|slice|both] [--iters 5] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import slice_timing as st  # noqa: E402
import tta_timing as tt  # noqa: E402
import wbf_oracle as wo  # noqa: E402
import yolo_nano_amd  # noqa: E402
from yolo_nano_amd import capi  # noqa: E402
from yolo_nano_amd.slicing import tile_table  # noqa: E402

THR = 0.55


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def device_us(fn, iters, reps):
    """mean / min / max over `iters` timed regions of `reps` calls each, microseconds per call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return {"mean_us": round(float(np.mean(ts)), 1), "min_us": round(float(np.min(ts)), 1), "max_us": round(float(np.max(ts)), 1)}


def with_capacity(obj, run, lists):
    """run(), and once more with the capacity the failure names"""
    try:
        return run()
    except capi.YnError as e:
        if "list_capacity" not in str(e):
            raise
        need = int(lists().max())
        obj.list_capacity = (need + 1023) // 1024 * 1024
        return run()


def measure(name, h, lists, C, E, records, iters, reps):
    """lists = (boxes [B, cap, 4], scores, cls, count) on the host; records(rule) runs the workload's whole batch with that rule"""
    lb, ls, lc, cnt = lists
    B, cap = lb.shape[0], lb.shape[1]
    rec = np.concatenate([np.concatenate([lb[b, :cnt[b]], ls[b, :cnt[b], None], lc[b, :cnt[b], None].astype(np.float32)], 1) for b in range(B)])
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    fu = capi.Fuse(h, max_units=B, list_capacity=cap)
    fu.open(B)
    fu.append(torch.from_numpy(rec.astype(np.float32)).to(h.device), torch.from_numpy(off).to(h.device), 1.0)
    res = {"lists": B, "expected": E, "iou_thr": THR, "rows_per_list": {"mean": round(float(cnt.mean()), 1), "max": int(cnt.max())}}
    # same_bits, and the oracle's wall time
    note(name, "lists:", res["rows_per_list"])
    fu.merge(B, capi.MERGE_WBF, THR, E)
    drec, doff, total = fu.result(total=True)
    drec, doff = drec[:total].cpu().numpy(), doff.cpu().numpy()
    t0 = time.perf_counter()
    wrec, woff = wo.wbf_records(lb, ls, lc, cnt, C, THR, E)
    oracle_ms = (time.perf_counter() - t0) * 1e3
    note(name, "oracle ms", round(oracle_ms, 1))
    res["same_bits"] = bool(np.array_equal(doff, woff) and wo.same_bits(drec, wrec))
    res["clusters_per_list"] = round(float(total) / B, 1)
    res["mean_votes"] = round(float(cnt.sum()) / max(total, 1), 2)
    res["merge_wbf"] = device_us(lambda: fu.merge(B, capi.MERGE_WBF, THR, E), iters, reps)
    res["merge_nms"] = device_us(lambda: fu.merge(B, capi.MERGE_NMS, THR), iters, reps)
    fu.merge(B, capi.MERGE_NMS, THR)
    res["nms_kept_per_list"] = round(float(fu.result(total=True)[2]) / B, 1)
    res["wbf_over_nms"] = round(res["merge_wbf"]["mean_us"] / res["merge_nms"]["mean_us"], 2)
    # the copies of the host route alone: the lists down, a result of the WBF result's size up (pinned on the host side)
    d = [torch.from_numpy(a).to(h.device) for a in (lb, ls, lc)]
    p = [torch.empty(a.shape, dtype=a.dtype).pin_memory() for a in d]
    up_h = torch.from_numpy(wrec).pin_memory() if len(wrec) else torch.zeros((1, 6)).pin_memory()
    up_d = torch.empty_like(up_h, device=h.device)

    def copies():
        for a, q in zip(d, p):
            q.copy_(a, non_blocking=True)
        up_d.copy_(up_h, non_blocking=True)
    res["host_copies"] = device_us(copies, iters, reps)
    res["host_oracle_ms"] = round(oracle_ms, 1)
    res["host_route_over_wbf"] = round((oracle_ms * 1e3 + res["host_copies"]["mean_us"]) / res["merge_wbf"]["mean_us"], 1)
    res["copies_over_wbf"] = round(res["host_copies"]["mean_us"] / res["merge_wbf"]["mean_us"], 2)
    fu.close()
    note(name, "merge:", res["merge_wbf"], res["merge_nms"])
    for rule in ("nms", "wbf"):
        records(rule)
        med, mn = tt.wall_ms(lambda: records(rule), iters)
        res["records_%s_ms" % rule] = {"median": round(med, 2), "min": round(mn, 2)}
    return res


def tta_workload(a):
    x = torch.from_numpy(tt.weights.make_input(tt.N, tt.S, seed=3)).cuda()
    conf = tt.pick_conf(x, a.keep_tta)
    model = tt.make_model(conf)
    objs = {m: yolo_nano_amd.TestTimeAugmentation(num_classes=tt.C, nms_thresh=THR, scale_range=tt.RANGE, merge=m) for m in ("nms", "wbf")}
    for o in objs.values():
        o.list_capacity = 16384
    o = objs["nms"]
    with_capacity(o, lambda: o.batch(x, model), lambda: o._tta.forwards_to_host(tt.N)[3])
    objs["wbf"].list_capacity = o.list_capacity
    lists = o._tta.forwards_to_host(tt.N)[:4]
    E = 2 * len(o.scales)
    res = measure("tta", model.handle(2 * tt.N), lists, tt.C, E, lambda rule: objs[rule].batch(x, model), a.iters, a.reps)
    return dict(res, images=tt.N, size=tt.S, forwards_per_image=E, conf_thresh=conf)


def slice_workload(a):
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, (st.H0, st.W0, 3), dtype=np.uint8)).cuda() for _ in range(st.F)]
    tiles = tile_table([(st.H0, st.W0)] * st.F, st.S, st.OVERLAP, True, st.S)
    objs = {m: yolo_nano_amd.SlicedInference(tile=st.S, overlap=st.OVERLAP, full_frame=True, nms_thresh=THR, list_capacity=8192, merge=m)
            for m in ("nms", "wbf")}
    for o in objs.values():
        o.chunk = st.CHUNK
    o = objs["nms"]
    conf = st.pick_conf(frames, tiles[:st.CHUNK], o, a.keep_slice)
    model = st.make_model(conf)
    with_capacity(o, lambda: o.batch(frames, model), lambda: o._obj.lists_to_host()[3])
    objs["wbf"].list_capacity = o.list_capacity
    lists = o._obj.lists_to_host()[:4]
    res = measure("slice", model.handle(st.CHUNK), lists, st.C, 1, lambda rule: objs[rule].batch(frames, model), a.iters, a.reps)
    return dict(res, frames=st.F, frame=[st.H0, st.W0], tile=st.S, tiles=int(len(tiles)), conf_thresh=conf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("tta", "slice", "both"), default="both")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keep-tta", type=int, default=300)
    ap.add_argument("--keep-slice", type=int, default=110)
    a = ap.parse_args()
    res = {}
    if a.workload in ("tta", "both"):
        res["tta"] = tta_workload(a)
    if a.workload in ("slice", "both"):
        res["slice"] = slice_workload(a)
    res["lds_clusters"] = capi.load_library().yn_wbf_lds_clusters()
    res["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
