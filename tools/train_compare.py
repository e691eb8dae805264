"""Compare the training step of two source trees (a refactor's parent and the refactor): same launches, same numbers.

  python tools/train_compare.py run FORM OUT.npz [--root TREE] [--size 128 --batch 8 --steps 4 --classes 20]
      FORM = f32 | f16_one | f16_fork (the fp16 step with the head-tower fork pinned: left alone, a handle times itself in steps 3-6
      and two runs may choose differently).  Runs the steps with updates on TREE's library (default: this tree) and stores the four
      losses of every step and the flat parameter / gradient buffers after the last one.  Under `rocprofv3 --kernel-trace` the same
      run gives the launch list (--no-autotune: the fp32 step's pointwise tile choice is timed once per process, so two runs of one
      tree may launch different, bit-identical, tile variants).
  python tools/train_compare.py numbers A.npz B.npz       max |a - b| per buffer, relative to the buffer's largest magnitude
  python tools/train_compare.py launches A_kernel_trace.csv B_kernel_trace.csv
      (kernel, grid, workgroup) per queue of the last complete step (between two sgd_kernel launches, as tools/train_timeline.py takes
      it): ordered lists, multisets, and - where the order differs - the blocks that moved.  A different number of memsets is reported
      and then set aside.
"""
import argparse, collections, csv, difflib, gzip, os, re, sys
import numpy as np


def run(a):
    root = os.path.abspath(a.root or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    import torch
    from yolo_nano_amd import arch, weights, capi
    assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == root, capi.__file__
    S, C, B = a.size, a.classes, a.batch
    rs = np.random.RandomState(5)                            # a seeded target, as tools/diag_train.py builds one
    N = arch.num_predictions(S)
    target = np.zeros((B, N, 11), np.float32)
    for b in range(B):
        idx = rs.choice(N, 6, replace=False)
        target[b, idx, 0] = 1.0; target[b, idx, 1] = rs.randint(0, C, 6); target[b, idx, 2:4] = rs.uniform(0, 1, (6, 2))
        target[b, idx, 4:6] = rs.standard_normal((6, 2)) * 0.3; target[b, idx, 6] = rs.uniform(1.0, 2.0, 6)
        c = rs.uniform(0.2, 0.8, (6, 2)); wh = rs.uniform(0.05, 0.4, (6, 2))
        target[b, idx, 7:9], target[b, idx, 9:11] = c - wh / 2, c + wh / 2
    dev = torch.device("cuda:0")
    own = torch.cuda.Stream(device=dev)                      # never the legacy null stream (bench.py train_bench)
    with torch.cuda.stream(own):
        h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=B, device=dev)
        h.load_state_dict(weights.make_state_dict("1.0x", C))
        h.train_bind()
        if a.no_autotune:
            h.autotune(False)                                # fp32: the pointwise tile choice is timed per process (bit-identical tiles, other kernel names)
        h.train_precision("f32" if a.form == "f32" else "f16")
        if a.form != "f32":
            h.head_fork(a.form == "f16_fork")
        x = torch.as_tensor(weights.make_input(B, S, seed=10)).to(dev)
        t = torch.as_tensor(target).to(dev)
        losses = [h.train_step(x, t, lr=1e-4).cpu().numpy() for _ in range(a.steps)]
        torch.cuda.synchronize(dev)
        np.savez(a.out, losses=np.stack(losses), params=h.flat_params.cpu().numpy(), grads=h.flat_grads.cpu().numpy())
    print("%s %s: losses of the last step %s" % (root, a.form, losses[-1]))


def numbers(a):
    x, y = np.load(a.a), np.load(a.b)
    worst = 0.0
    for k in ("losses", "params", "grads"):
        p, q = x[k].astype(np.float64), y[k].astype(np.float64)
        same = x[k].tobytes() == y[k].tobytes()
        rel = float(np.abs(p - q).max() / max(np.abs(p).max(), 1e-300)) if np.isfinite(p).all() and np.isfinite(q).all() else float("nan")
        worst = max(worst, rel)
        print("%-7s %s  max|a-b| / max|a| = %.3e  (%d elements)" % (k, "bit-identical" if same else "DIFFERENT    ", rel, p.size))
    return worst


def last_step(path):
    rows = list(csv.DictReader(gzip.open(path, "rt") if path.endswith(".gz") else open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    sgd = [i for i, r in enumerate(rows) if "sgd_kernel" in r["Kernel_Name"]]
    step = rows[sgd[-3] + 1:sgd[-2] + 1]
    q = collections.OrderedDict()
    for r in step:
        name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("ynk::", "").replace("void ", ""))
        q.setdefault(r.get("Queue_Id", "0"), []).append((name, int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1) * int(r.get("Grid_Size_Z", 1) or 1), int(r["Workgroup_Size_X"])))
    return sorted(q.values(), key=len, reverse=True)          # queue ids differ from run to run: the main queue first, then by length


def launches(a):
    A, B = last_step(a.a), last_step(a.b)
    print("launches per queue: A %s   B %s" % ([len(q) for q in A], [len(q) for q in B]))
    fills = lambda Q: [sum("fillBuffer" in k[0] for k in q) for q in Q]
    if fills(A) != fills(B):                                  # hipMemsetAsync shows as a runtime fill kernel: counted, then left out of the lists
        print("memsets per queue: A %s   B %s  (left out of the comparison below)" % (fills(A), fills(B)))
        A, B = [[[k for k in q if "fillBuffer" not in k[0]] for q in Q] for Q in (A, B)]
    ok = len(A) == len(B)
    for i, (qa, qb) in enumerate(zip(A, B)):
        if qa == qb:
            print("queue %d: ordered lists identical (%d launches)" % (i, len(qa)))
            continue
        multi = collections.Counter(qa) == collections.Counter(qb)
        print("queue %d: order differs, multisets %s" % (i, "identical" if multi else "DIFFERENT"))
        if not multi:
            ok = False
            d = collections.Counter(qa); d.subtract(collections.Counter(qb))
            for k, v in d.items():
                if v:
                    print("   %+d %s" % (v, k))
        loss = [j for j, k in enumerate(qa) if "loss" in k[0]]
        gone, come = [], []
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, qa, qb, autojunk=False).get_opcodes():
            if tag != "equal":
                gone += qa[i1:i2]; come += qb[j1:j2]
                print("   %-7s A[%d:%d] (%d)  B[%d:%d] (%d)   first: %s" % (tag, i1, i2, i2 - i1, j1, j2, j2 - j1, (qa[i1:i2] or qb[j1:j2])[0][0]))
                if loss and max(i2, j2) > loss[0] + 8:
                    ok = False
                    print("   ^ past the loss kernel (A[%d]): NOT a forward reordering" % loss[0])
        moved = collections.Counter(gone) == collections.Counter(come)
        print("   blocks that moved: %d launches, %s; the rest of the ordered list is identical" % (len(gone), "the same multiset on both sides" if moved else "NOT the same launches"))
        ok = ok and moved
    print("RESULT", "same launches" if ok else "DIFFERENT launches")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("run"); p.add_argument("form", choices=("f32", "f16_one", "f16_fork")); p.add_argument("out"); p.add_argument("--root")
    p.add_argument("--size", type=int, default=128); p.add_argument("--batch", type=int, default=8); p.add_argument("--steps", type=int, default=4); p.add_argument("--classes", type=int, default=20)
    p.add_argument("--no-autotune", action="store_true")
    for c in ("numbers", "launches"):
        p = sub.add_parser(c); p.add_argument("a"); p.add_argument("b")
    a = ap.parse_args()
    if a.cmd == "run":
        run(a)
    elif a.cmd == "numbers":
        numbers(a)
    else:
        sys.exit(launches(a))
