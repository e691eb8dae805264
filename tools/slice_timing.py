#!/usr/bin/env python3
"""Sliced inference timing: 32 frames of 1280 x 720, tile 416, overlap 0.2, full frame on (9 tiles per frame: 288 tiles, nine yn_infer of 32),
1.0x, COCO head, random weights.

  device  SlicedInference.batch(frames, model): yn_slice_infer - per chunk of 32 tiles one tile launch (frames read in place), one yn_infer,
          one append; one read-back; one batched merge; two copies to the host
  glue    the same frames through the calls the package had before: torch crops made contiguous, ValTransforms.batch per 32 tiles, yn_infer,
          every tile's detections to the host (yn_pack_detections, two copies), the remap in numpy, one upload + yn_nms_merge per frame
  tile    slice_tile_kernel alone over the 288 tiles against its HBM floor: the tiles' source bytes read once + 12 * side^2 bytes written
          per tile, at 8.0 TB/s

conf_thresh is set from the data, as tools/tta_timing.py sets its own: the score that --keep candidates per tile exceed in a plain 416
forward of the first 32 tiles (default 110: a frame's merge list of about 10^3 rows).  Both routes run the same model and must return the
same bits, which is checked.  Wall-clock times in one process: median over --iters runs after one warm-up run of each route.
Prints ONE JSON line.

    python tools/slice_timing.py [--iters 5] [--keep 110] [--capacity 8192]
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
from yolo_nano_amd.slicing import tile_table  # noqa: E402

F, H0, W0, S, C, CHUNK, HBM = 32, 720, 1280, 416, 80, 32, 8.0e12
OVERLAP, NMS = 0.2, 0.5


def make_model(conf):
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, trainable=False, conf_thresh=conf, nms_thresh=NMS,
                               anchor_size=arch.MULTI_ANCHOR_SIZE_COCO, backbone="1.0x")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in weights.make_state_dict("1.0x", C).items()}, strict=False)
    return m.to("cuda").eval()


def pick_conf(frames, tiles, sl, keep):
    """The score that `keep` candidates per tile exceed in a plain forward of `tiles` (yn_score_full: every candidate, no threshold, no NMS)."""
    m = make_model(0.0)
    h = m.handle(CHUNK)
    tk = capi.Slice(h, len(frames), 16)
    x = tk.preprocess(frames, tiles, S, sl.mean, sl.std)
    tk.close()
    heads = [t.permute(0, 2, 3, 1).contiguous() for t in m.forward_raw(x)]
    _, cls = h.score_full(heads)
    best = cls.max(dim=2).values.flatten()
    k = min(keep * x.shape[0], best.numel() - 1)
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


def remap_host(b, tile, h0, w0):
    """DESIGN 28's remap of one tile's boxes in numpy: float64 steps rounded to float32, then the float32 add, clamp and divide (no edge filter)."""
    _, x, y, tw, th, rw, rh, left, top = [int(v) for v in tile]
    side = float(S)
    v = np.asarray(b, dtype=np.float32).reshape(-1, 4)
    v = (v.astype(np.float64) - np.array([left / side, top / side] * 2)).astype(np.float32)
    v = (v.astype(np.float64) / np.array([rw / side, rh / side] * 2)).astype(np.float32)
    v = (v.astype(np.float64) * np.array([tw, th] * 2, dtype=np.float64)).astype(np.float32)
    q = v + np.array([x, y, x, y], dtype=np.float32)
    hi = np.array([w0, h0, w0, h0], dtype=np.float32)
    q = np.where(q < np.float32(0), np.float32(0), np.where(q > hi, hi, q)).astype(np.float32)
    return q / np.float32(max(h0, w0))


def glue(frames, tiles, model, tf):
    """The public calls the package had before yn_slice_*."""
    h = model.handle(CHUNK)
    per = [[] for _ in frames]
    for t0 in range(0, len(tiles), CHUNK):
        rows = tiles[t0:t0 + CHUNK]
        crops = [frames[int(r[0])][int(r[2]):int(r[2]) + int(r[4]), int(r[1]):int(r[1]) + int(r[3])].contiguous() for r in rows]
        x = tf.batch(crops)[0]
        dets = model.forward_batch(x)
        for r, (bb, sc, cl) in zip(rows, dets):
            f = int(r[0])
            per[f].append((remap_host(bb, r, int(frames[f].shape[0]), int(frames[f].shape[1])), sc, cl))
    out = []
    for f in range(len(frames)):
        bb = np.concatenate([p[0] for p in per[f]])
        sc = np.concatenate([p[1] for p in per[f]])
        cl = np.concatenate([p[2] for p in per[f]])
        if len(sc) == 0:
            out.append((bb, sc, cl))
            continue
        ob, osc, oc, _ = h.nms_merge(torch.from_numpy(bb).to(h.device), torch.from_numpy(sc).to(h.device),
                                     torch.from_numpy(cl.astype(np.int32)).to(h.device), C, NMS)
        out.append((ob.cpu().numpy(), osc.cpu().numpy(), oc.cpu().numpy().astype(np.int64)))
    return out


def tile_share(frames, tiles, iters, h):
    """All tiles, then the two kinds on their own: the 416 x 416 crops (copy path, four pixels per thread) and the full frames (1280 x 720 resized
    to 416 x 234 between two bands of pad: cv2's linear resize, pixel by pixel)."""
    sl = capi.Slice(h, len(frames), 16)
    crop = (tiles[:, 3] == S) & (tiles[:, 4] == S)
    res = _tile_share(sl, frames, tiles, iters)
    res["crops_only"] = _tile_share(sl, frames, tiles[crop], iters)
    res["full_frames_only"] = _tile_share(sl, frames, tiles[~crop], iters)
    sl.close()
    return res


def _tile_share(sl, frames, tiles, iters):
    sli = yolo_nano_amd.SlicedInference(tile=S)
    out = torch.empty((len(tiles), 3, S, S), dtype=torch.float32, device="cuda")
    for _ in range(5):
        sl.preprocess(frames, tiles, S, sli.mean, sli.std, out=out)
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            sl.preprocess(frames, tiles, S, sli.mean, sli.std, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / 10)
    us = float(np.median(times))
    src = int(sum(3 * int(r[3]) * int(r[4]) for r in tiles))
    dst = len(tiles) * 12 * S * S
    floor = (src + dst) / HBM * 1e6
    return {"tiles": int(len(tiles)), "us": round(us, 1), "source_bytes": src, "written_bytes": dst, "hbm_floor_us": round(floor, 1), "floor_share": round(floor / us, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--keep", type=int, default=110)
    ap.add_argument("--capacity", type=int, default=8192)
    a = ap.parse_args()
    rng = np.random.default_rng(3)
    frames = [torch.from_numpy(rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)).cuda() for _ in range(F)]
    tiles = tile_table([(H0, W0)] * F, S, OVERLAP, True, S)
    sl = yolo_nano_amd.SlicedInference(tile=S, overlap=OVERLAP, full_frame=True, nms_thresh=NMS, list_capacity=a.capacity)
    sl.chunk = CHUNK
    conf = pick_conf(frames, tiles[:CHUNK], sl, a.keep)
    model = make_model(conf)
    res = {"frames": F, "frame": [H0, W0], "tile": S, "overlap": OVERLAP, "tiles": int(len(tiles)), "forwards_of_32": -(-len(tiles) // CHUNK),
           "conf_thresh": conf, "nms_thresh": NMS, "edge_margin": -1.0}
    try:
        dets = sl.batch(frames, model)                          # warm-up run (autotune at bs 32)
    except capi.YnError as e:
        if "list_capacity" not in str(e):
            raise
        need = int(sl._obj.lists_to_host()[3].max())
        if need > 131072:
            print(json.dumps(dict(res, error=str(e))))
            return 1
        sl.list_capacity = (need + 1023) // 1024 * 1024
        dets = sl.batch(frames, model)
    counts = sl._obj.lists_to_host()[3]
    res["list_capacity"] = int(sl.list_capacity)
    res["list_rows"] = {"mean": round(float(counts.mean()), 1), "max": int(counts.max())}
    res["merged_per_frame"] = round(float(np.mean([len(d[1]) for d in dets])), 1)
    med, mn = wall_ms(lambda: sl.batch(frames, model), a.iters)
    res["device_ms_per_batch"] = round(med, 2)
    res["device_ms_min"] = round(mn, 2)
    glue_model = make_model(conf)
    tf = yolo_nano_amd.ValTransforms(S, handle=glue_model.handle(CHUNK))
    ref = glue(frames, tiles, glue_model, tf)                   # warm-up run
    res["same_bits"] = bool(all(np.array_equal(d[0].view(np.uint32), r[0].view(np.uint32)) and np.array_equal(d[1].view(np.uint32), r[1].view(np.uint32))
                                and np.array_equal(d[2], r[2]) for d, r in zip(dets, ref)))
    med, mn = wall_ms(lambda: glue(frames, tiles, glue_model, tf), a.iters)
    res["glue_ms_per_batch"] = round(med, 2)
    res["glue_ms_min"] = round(mn, 2)
    res["speedup"] = round(res["glue_ms_per_batch"] / res["device_ms_per_batch"], 2)
    res["tile_kernel"] = tile_share(frames, tiles, a.iters, model.handle(CHUNK))
    res["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
