#!/usr/bin/env python3
"""Tracking detections across frames (yn_track_*): 32 camera streams, 200 steps after warm-up, about 40 random-walk objects plus clutter
per stream and frame, generated from a seed; every step's records are on the device before the clock starts, as yn_pack_detections leaves them.

  device   Tracker.update for all streams at once, HIP events around the 200 asynchronous updates, per update; launches per update
  host     the route without the device tracker, in the same run: offsets and records read back into page-locked buffers, the float32
           numpy restatement (tests/track_oracle.py) stepped for every stream, the result (rows, ids, offsets) uploaded again.  Wall clock
  copies   the read-back and the upload of that route alone: what any host tracker pays before it computes anything
  same_bits  every step's rows, ids and offsets of the two routes compared, all bits
  sweep    device and copies at 1 / 8 / 32 / 128 streams (100 steps each)

The kernel is latency-bound by construction (one workgroup per stream), so it is reported as time per update, not against a roofline.
Prints ONE JSON line.

    python tools/track_timing.py [--streams 32] [--steps 200] [--warmup 20] [--seed 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import track_oracle as orc  # noqa: E402
from yolo_nano_amd import track  # noqa: E402

OBJECTS, CLUTTER = 40, 8


def workload(seed, streams, steps):
    """-> per step (rec float32 [total][6], offsets int32 [streams + 1]): random-walk boxes in a 1280 x 720 frame, 8% dropouts, scores
    0.3 .. 1, three classes, up to CLUTTER low-score boxes, records in shuffled order."""
    rng = np.random.RandomState(seed)
    pos = rng.uniform([0, 0], [1280, 720], size=(streams, OBJECTS, 2))
    vel = rng.uniform(-4, 4, size=(streams, OBJECTS, 2))
    size = rng.uniform(30, 120, size=(streams, OBJECTS, 2))
    cls = rng.randint(0, 3, size=(streams, OBJECTS))
    out = []
    for _ in range(steps):
        pos = pos + vel + rng.normal(0, 0.7, size=pos.shape)
        rows, off = [], [0]
        for s in range(streams):
            keep = rng.uniform(size=OBJECTS) > 0.08
            wh = size[s][keep] * rng.uniform(0.97, 1.03, size=(int(keep.sum()), 2))
            r = np.concatenate([pos[s][keep] - wh / 2, pos[s][keep] + wh / 2, rng.uniform(0.3, 1.0, size=(len(wh), 1)), cls[s][keep][:, None]], axis=1)
            n = rng.randint(0, CLUTTER + 1)
            xy, cwh = rng.uniform([0, 0], [1280, 720], size=(n, 2)), rng.uniform(20, 100, size=(n, 2))
            c = np.concatenate([xy - cwh / 2, xy + cwh / 2, rng.uniform(0.05, 0.55, size=(n, 1)), rng.randint(0, 3, size=(n, 1))], axis=1)
            r = np.concatenate([r, c])[rng.permutation(len(r) + n)]
            rows.append(r)
            off.append(off[-1] + len(r))
        out.append((np.concatenate(rows).astype(np.float32), np.asarray(off, np.int32)))
    return out


def device_route(tr, dev_steps, warmup):
    """ms per update from events around the timed updates"""
    tr.reset()
    for rec, off in dev_steps[:warmup]:
        tr.update(rec, off)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for rec, off in dev_steps[warmup:]:
        tr.update(rec, off)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (len(dev_steps) - warmup)


class HostRoute:
    def __init__(self, streams, cap):
        self.streams = streams
        self.rec_pin = torch.empty((cap, 6), dtype=torch.float32).pin_memory()
        self.off_pin = torch.empty((streams + 1,), dtype=torch.int32).pin_memory()
        rows = streams * 128
        self.out_pin = [torch.zeros((rows, 6), dtype=torch.float32).pin_memory(), torch.zeros((rows,), dtype=torch.int32).pin_memory(),
                        torch.zeros((streams + 1,), dtype=torch.int32).pin_memory()]
        self.out_dev = [torch.zeros_like(t, device="cuda") for t in self.out_pin]

    def down(self, rec, off):
        self.off_pin.copy_(off, non_blocking=True)
        self.rec_pin[:rec.shape[0]].copy_(rec, non_blocking=True)
        torch.cuda.synchronize()

    def up(self, n):
        self.out_dev[0][:n].copy_(self.out_pin[0][:n], non_blocking=True)
        self.out_dev[1][:n].copy_(self.out_pin[1][:n], non_blocking=True)
        self.out_dev[2].copy_(self.out_pin[2], non_blocking=True)
        torch.cuda.synchronize()

    def run(self, dev_steps, warmup, tracker=None, keep=None, sizes=None):
        """tracker None: the copies alone; the upload has the size of the tracked route's result (`sizes`, rows per step) or, unknown, of the input."""
        t0 = None
        for k, (rec, off) in enumerate(dev_steps):
            if k == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            self.down(rec, off)
            n = int(self.off_pin[-1])
            if tracker is not None:
                o, r = self.off_pin.numpy(), self.rec_pin.numpy()
                e_rec, e_ids, e_off = tracker.update([r[o[b]:o[b + 1]] for b in range(self.streams)])
                n = len(e_ids)
                self.out_pin[0].numpy()[:n] = e_rec
                self.out_pin[1].numpy()[:n] = e_ids
                self.out_pin[2].numpy()[:] = e_off
                if keep is not None:
                    keep.append((e_rec.copy(), e_ids.copy(), e_off.copy()))
            else:
                n = sizes[k] if sizes is not None else min(n, self.out_pin[0].shape[0])
            self.up(n)
        return (time.perf_counter() - t0) * 1e3 / (len(dev_steps) - warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "track_timing needs the GPU"
    result = {"tool": "track_timing", "device": torch.cuda.get_device_name(0), "streams": args.streams, "steps": args.steps, "warmup": args.warmup,
              "objects_per_stream": OBJECTS, "clutter_up_to": CLUTTER, "seed": args.seed}

    S = args.streams
    steps = workload(args.seed, S, args.warmup + args.steps)
    dev_steps = [(torch.from_numpy(r).cuda(), torch.from_numpy(o).cuda()) for r, o in steps]
    tr = track.Tracker(S)
    device_route(tr, dev_steps, args.warmup)                    # once untimed: first-launch costs
    dev_ms = sorted(device_route(tr, dev_steps, args.warmup) for _ in range(3))
    # the two routes, bit for bit (an untimed pass of the device route, read back step by step)
    host = HostRoute(S, max(len(r) for r, _ in steps))
    kept = []
    host_ms = host.run(dev_steps, args.warmup, orc.Tracker(S), kept)
    copies_ms = sorted(host.run(dev_steps, args.warmup, sizes=[len(k[1]) for k in kept]) for _ in range(3))
    tr.reset()
    same, tracks = True, 0
    for (rec, off), (e_rec, e_ids, e_off) in zip(dev_steps, kept):
        g_rec, g_ids, g_off = (t.cpu().numpy() for t in tr.update(rec, off))
        n = len(e_ids)
        tracks += n
        same = same and np.array_equal(g_off, e_off) and np.array_equal(g_ids[:n], e_ids) and np.array_equal(g_rec[:n].view(np.int32), e_rec.view(np.int32))
    st = tr.status()
    result.update({
        "records_per_update": round(float(np.mean([len(r) for r, _ in steps])), 1), "tracks_out_per_update": round(tracks / len(kept), 1),
        "births": st["births"], "launches_per_update": (S + 255) // 256 + 1,
        "device_ms_per_update": round(dev_ms[1], 4), "device_ms_min_max": [round(dev_ms[0], 4), round(dev_ms[2], 4)],
        "host_route_ms_per_update": round(host_ms, 3), "copies_alone_ms_per_update": round(copies_ms[1], 4),
        "copies_ms_min_max": [round(copies_ms[0], 4), round(copies_ms[2], 4)], "copies": "pinned",
        "same_bits": bool(same), "device_beats_host_route": bool(dev_ms[1] < host_ms), "device_beats_copies_alone": bool(dev_ms[1] < copies_ms[1]),
    })
    tr.close()

    sweep, first = [], None
    for n in (1, 8, 32, 128):
        sw = workload(args.seed + 1, n, 20 + 100)
        d = [(torch.from_numpy(r).cuda(), torch.from_numpy(o).cuda()) for r, o in sw]
        t = track.Tracker(n)
        device_route(t, d, 20)
        dm = sorted(device_route(t, d, 20) for _ in range(3))[1]
        hr = HostRoute(n, max(len(r) for r, _ in sw))
        cm = sorted(hr.run(d, 20) for _ in range(3))[1]
        t.close()
        sweep.append({"streams": n, "device_ms": round(dm, 4), "copies_alone_ms": round(cm, 4), "device_beats_copies": bool(dm < cm)})
        if dm < cm and first is None:
            first = n
    result["sweep"] = sweep
    result["device_beats_copies_from_streams"] = first
    print(json.dumps(result))


if __name__ == "__main__":
    main()
