#!/usr/bin/env python3
"""Soft-NMS timing (yn_soft_nms_merge's rule; csrc/kernels_soft.hip) against the per-class NMS it stands in for:

  tta    the merge lists of tools/tta_timing.py's workload (32 images at 416, scales 320..640 step 32 x flip, its model and conf_thresh)
  slice  the merge lists of tools/slice_timing.py's workload (32 frames of 1280 x 720, tile 416, overlap 0.2, its model and conf_thresh)
  infer  yn_infer at 416, bs 32, COCO head, random weights, at both threshold pairs the README uses (conf 0.001 / nms 0.5 and
         conf 0.1 / nms 0.45): the whole call with the NMS chain and with the soft suppression (score_floor = conf_thresh)

For tta and slice the lists of one run are taken to the host once and put into a yn_fuse object, so that every suppression merges the
SAME lists (score_floor 0.001 there, so that hardly a row dies of decay: the walk's cost is not flattered):

  merge        yn_fuse_merge alone (one read-back of the state words, the merge, the pack) under the NMS rule with the suppression off,
               linear and gaussian: device time between two events around --reps calls, mean and min / max over --iters such regions
  host route   what a user without the kernel does: the lists to the host, tests/soft_nms_oracle.py there, the result back up - the
               copies alone (pinned buffers, timed like the merge) and the restatement's wall time (one run)
  records      the whole records() batch of the workload's object with each suppression, wall clock, median and min over --iters runs
  same_bits    the device's records against the restatement's, per method

For infer: device time per yn_infer (events around --reps calls), kept rows per image, and same_bits on the first --check-images images
(their candidates through yn_score_full and tests/nms_stage_oracle.candidates; the restatement walks thousands of rows per class there).

No target is fixed in advance: the yardsticks are the NMS route and the host route.  Every workload runs in a process of its own under
its own time limit (--limit seconds); after a failure or an expired limit nothing more is started.  Prints ONE JSON line per workload.

    python tools/soft_nms_timing.py [--workload tta|slice|infer|all] [--iters 5] [--reps 10] [--limit 420]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, SIGMA, FLOOR = 0.5, 0.5, 0.001                             # FLOOR: of the tta and slice lists (fusion.soft_nms's default: hardly a row dies of decay)
SOFTS = ("linear", "gaussian")


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def parent(a):
    """One child process per workload, each under its own time limit; the GPU is never touched here."""
    todo = ("tta", "slice", "infer") if a.workload == "all" else (a.workload,)
    for w in todo:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--workload", w, "--iters", str(a.iters), "--reps", str(a.reps),
               "--keep-tta", str(a.keep_tta), "--keep-slice", str(a.keep_slice), "--check-images", str(a.check_images)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            note("soft_nms_timing: workload %s passed its limit of %d s; nothing more is started" % (w, a.limit))
            return 124
        if rc:
            note("soft_nms_timing: workload %s ended with status %d; nothing more is started" % (w, rc))
            return rc
    return 0


def child(a):
    import numpy as np
    import torch

    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
    import nms_stage_oracle as ns
    import soft_nms_oracle as so
    import tta_timing as tt
    import yolo_nano_amd
    from wbf_timing import device_us, with_capacity
    from yolo_nano_amd import arch, capi, weights

    def floor_of(conf):
        return float(np.float32(conf))

    def measure(name, h, lists, C, floor, records):
        """lists = (boxes [B, cap, 4], scores, cls, count) on the host; records(soft) runs the workload's whole batch with that suppression"""
        lb, ls, lc, cnt = lists
        B, cap = lb.shape[0], lb.shape[1]
        rec = np.concatenate([np.concatenate([lb[b, :cnt[b]], ls[b, :cnt[b], None], lc[b, :cnt[b], None].astype(np.float32)], 1) for b in range(B)])
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        fu = capi.Fuse(h, max_units=B, list_capacity=cap)
        fu.open(B)
        fu.append(torch.from_numpy(rec.astype(np.float32)).to(h.device), torch.from_numpy(off).to(h.device), 1.0)
        res = {"lists": B, "iou_thr": THR, "sigma": SIGMA, "score_floor": floor, "rows_per_list": {"mean": round(float(cnt.mean()), 1), "max": int(cnt.max())}}
        note(name, "lists:", res["rows_per_list"])
        fu.merge_soft(None)
        fu.merge(B, capi.MERGE_NMS, THR)
        nms_total = fu.result(total=True)[2]
        res["nms_kept_per_list"] = round(float(nms_total) / B, 1)
        res["merge_nms"] = device_us(lambda: fu.merge(B, capi.MERGE_NMS, THR), a.iters, a.reps)
        d = [torch.from_numpy(x).to(h.device) for x in (lb, ls, lc)]
        p = [torch.empty(x.shape, dtype=x.dtype).pin_memory() for x in d]
        for soft in SOFTS:
            fu.merge_soft(soft, SIGMA, floor)
            fu.merge(B, capi.MERGE_NMS, THR)
            drec, doff, total = fu.result(total=True)
            drec, doff = drec[:total].cpu().numpy(), doff.cpu().numpy()
            t0 = time.perf_counter()
            wrec, woff = so.soft_records(lb, ls, lc, cnt, C, so.METHODS[soft], THR, SIGMA, floor)
            oracle_ms = (time.perf_counter() - t0) * 1e3
            r = {"same_bits": bool(np.array_equal(doff, woff) and so.same_bits(drec, wrec)), "kept_per_list": round(float(total) / B, 1)}
            r["merge"] = device_us(lambda: fu.merge(B, capi.MERGE_NMS, THR), a.iters, a.reps)
            r["over_nms"] = round(r["merge"]["mean_us"] / res["merge_nms"]["mean_us"], 2)
            # the copies of the host route alone: the lists down, a result of this result's size up (pinned on the host side)
            up_h = torch.from_numpy(wrec).pin_memory() if len(wrec) else torch.zeros((1, 6)).pin_memory()
            up_d = torch.empty_like(up_h, device=h.device)

            def copies():
                for x, q in zip(d, p):
                    q.copy_(x, non_blocking=True)
                up_d.copy_(up_h, non_blocking=True)
            r["host_copies"] = device_us(copies, a.iters, a.reps)
            r["host_oracle_ms"] = round(oracle_ms, 1)
            r["host_route_over_soft"] = round((oracle_ms * 1e3 + r["host_copies"]["mean_us"]) / r["merge"]["mean_us"], 1)
            r["copies_over_soft"] = round(r["host_copies"]["mean_us"] / r["merge"]["mean_us"], 2)
            res[soft] = r
            note(name, soft, r)
        fu.close()
        for soft in (None,) + SOFTS:
            records(soft)
            med, mn = tt.wall_ms(lambda: records(soft), a.iters)
            res["records_%s_ms" % (soft or "nms")] = {"median": round(med, 2), "min": round(mn, 2)}
        return res

    def tta_workload():
        x = torch.from_numpy(weights.make_input(tt.N, tt.S, seed=3)).cuda()
        conf = tt.pick_conf(x, a.keep_tta)
        model = tt.make_model(conf)
        objs = {s: yolo_nano_amd.TestTimeAugmentation(num_classes=tt.C, nms_thresh=THR, scale_range=tt.RANGE, soft=s, sigma=SIGMA, score_floor=FLOOR) for s in (None,) + SOFTS}
        for o in objs.values():
            o.list_capacity = 16384
        o = objs[None]
        with_capacity(o, lambda: o.batch(x, model), lambda: o._tta.forwards_to_host(tt.N)[3])
        for s in SOFTS:
            objs[s].list_capacity = o.list_capacity
        lists = o._tta.forwards_to_host(tt.N)[:4]
        res = measure("tta", model.handle(2 * tt.N), lists, tt.C, FLOOR, lambda s: objs[s].batch(x, model))
        return dict(res, images=tt.N, size=tt.S, forwards_per_image=2 * len(o.scales), conf_thresh=conf)

    def slice_workload():
        import slice_timing as st
        from yolo_nano_amd.slicing import tile_table
        rng = np.random.default_rng(3)
        frames = [torch.from_numpy(rng.integers(0, 256, (st.H0, st.W0, 3), dtype=np.uint8)).cuda() for _ in range(st.F)]
        tiles = tile_table([(st.H0, st.W0)] * st.F, st.S, st.OVERLAP, True, st.S)
        objs = {s: yolo_nano_amd.SlicedInference(tile=st.S, overlap=st.OVERLAP, full_frame=True, nms_thresh=THR, list_capacity=8192, soft=s, sigma=SIGMA, score_floor=FLOOR)
                for s in (None,) + SOFTS}
        for o in objs.values():
            o.chunk = st.CHUNK
        o = objs[None]
        conf = st.pick_conf(frames, tiles[:st.CHUNK], o, a.keep_slice)
        model = st.make_model(conf)
        with_capacity(o, lambda: o.batch(frames, model), lambda: o._obj.lists_to_host()[3])
        for s in SOFTS:
            objs[s].list_capacity = o.list_capacity
        lists = o._obj.lists_to_host()[:4]
        res = measure("slice", model.handle(st.CHUNK), lists, st.C, FLOOR, lambda s: objs[s].batch(frames, model))
        return dict(res, frames=st.F, frame=[st.H0, st.W0], tile=st.S, tiles=int(len(tiles)), conf_thresh=conf)

    def infer_workload():
        B, S, C = 32, 416, 80
        x = torch.from_numpy(weights.make_input(B, S, seed=3)).cuda()
        h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE_COCO, "1.0x", max_batch=B)
        h.load_state_dict(weights.make_state_dict("1.0x", C))
        h.fold_bn()
        out = h.alloc_outputs(B)
        heads = h.forward_raw(x)
        bbox, conf_all = [t.cpu().numpy() for t in h.score_full(heads)]
        res = {"images": B, "size": S, "classes": C, "sigma": SIGMA, "pairs": []}
        for conf, thr in ((0.001, 0.5), (0.1, 0.45)):
            h.set_thresholds(conf, thr)
            r = {"conf_thresh": conf, "nms_thresh": thr, "score_floor": floor_of(conf)}
            h.soft_nms(None)
            h.infer(x, out=out)
            r["nms"] = dict(device_us(lambda: h.infer(x, out=out), a.iters, a.reps), kept_per_image=round(float(out[4].sum().item()) / B, 1))
            cand = [ns.candidates(conf_all[b], conf) for b in range(a.check_images)]
            r["candidates_per_image"] = round(float(np.mean([(c[0] >= 0).sum() for c in cand])), 1) if cand else None
            r["largest_class_rows"] = int(max(np.bincount(c[0][c[0] >= 0], minlength=C).max() for c in cand)) if cand else None
            for soft in SOFTS:
                h.soft_nms(soft, SIGMA, floor_of(conf))
                h.infer(x, out=out)
                q = dict(device_us(lambda: h.infer(x, out=out), a.iters, a.reps), kept_per_image=round(float(out[4].sum().item()) / B, 1))
                q["over_nms"] = round(q["mean_us"] / r["nms"]["mean_us"], 2)
                got = [t.cpu().numpy() for t in out]
                same, t0 = True, time.perf_counter()
                for b in range(a.check_images):
                    want = so.soft_nms(bbox[b], cand[b][1], cand[b][0], C, so.METHODS[soft], thr, SIGMA, floor_of(conf))
                    k = int(got[4][b])
                    same = same and k == len(want[3]) and all(so.same_bits(g[b, :k], w) for g, w in zip(got[:4], want))
                q["same_bits"] = bool(same) if a.check_images else None
                q["host_oracle_ms_per_image"] = round((time.perf_counter() - t0) * 1e3 / max(a.check_images, 1), 1)
                r[soft] = q
                note("infer", conf, thr, soft, q)
            res["pairs"].append(r)
        h.soft_nms(None)
        h.close()
        return res

    res = {a.workload: {"tta": tta_workload, "slice": slice_workload, "infer": infer_workload}[a.workload]()}
    res["lds_rows"] = capi.load_library().yn_soft_lds_rows()
    res["gpu"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("tta", "slice", "infer", "all"), default="all")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keep-tta", type=int, default=300)
    ap.add_argument("--keep-slice", type=int, default=110)
    ap.add_argument("--check-images", type=int, default=2, help="images of the infer workload whose bits are compared with the restatement")
    ap.add_argument("--limit", type=int, default=420, help="seconds a workload's process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    return child(a) if a.child else parent(a)


if __name__ == "__main__":
    sys.exit(main())
