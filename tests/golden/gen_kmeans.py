"""Generate tests/golden/kmeans.npz: the reference's own kmeans_anchor.py (imported unmodified) run on small box sets.

    python tests/golden/gen_kmeans.py [path/to/reference]     (default: $YN_REFERENCE, else ../reference beside the repository)

kmeans_anchor.py parses its command line and imports the cv2-based dataset loaders at import time, so it is imported with sys.argv
reduced to the script name and with stub modules for data.voc and data.coco.  Its init_centroids, do_kmeans and anchor_box_kmeans are
then called under np.random.seed.  Per set the file holds the boxes, the seed, the draws the seed produces, the picked centroids, the
centroids / groups / loss of each of the first 40 passes and the final centroids and iteration count of the full loop.

The comparison of an exact-sum implementation with the reference's sequentially rounded sums is only sound where no decision hangs on
the last bits, so this generator ASSERTS, for every stored set:
  - every box's gap between its two nearest centroids is > 1e-9 in every stored pass (sets with duplicate centroids excepted where the
    tie is exact: both implementations send an exact tie to the lower index);
  - every k-means++ threshold is at least 1e-9 * sum_distance away from the neighbouring prefix sums;
  - every |old_loss - loss| before the stop is either > 1e-3 or exactly 0.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("YN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "kmeans.npz")
PASSES = 40


def import_reference():
    data = types.ModuleType("data")
    data.__path__ = []
    voc, coco = types.ModuleType("data.voc"), types.ModuleType("data.coco")
    voc.VOCDetection = coco.COCODataset = object
    saved = {k: sys.modules.get(k) for k in ("data", "data.voc", "data.coco")}
    sys.modules.update({"data": data, "data.voc": voc, "data.coco": coco})
    argv = sys.argv
    sys.argv = [argv[0]]
    sys.path.insert(0, REF)
    try:
        import kmeans_anchor
    finally:
        sys.argv = argv
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return kmeans_anchor


def lognormal(n, seed):
    r = np.random.RandomState(seed)
    return np.clip(np.exp(r.normal(4.0, 0.9, size=(n, 2))), 1.0, 416.0)


def sets():
    r = np.random.RandomState(5)
    ints = r.randint(1, 40, size=(257, 2)).astype(np.float64)
    ints[100:180] = ints[:80]                                          # many duplicates
    return [("ln300", lognormal(300, 1), 9, 3), ("ln5000", lognormal(5000, 2), 9, 11), ("int257", ints, 5, 7),
            ("same5", np.tile(np.array([[10.0, 20.0]]), (5, 1)), 3, 1), ("four", lognormal(4, 3), 9, 2)]


def wh(boxes):
    return np.array([[b.w, b.h] for b in boxes], dtype=np.float64).reshape(-1, 2)


def main():
    ka = import_reference()
    quiet = io.StringIO()
    out = {"source": np.array("kmeans_anchor.py of the reference, imported unmodified (tests/golden/gen_kmeans.py)"),
           "names": np.array([s[0] for s in sets()])}
    for name, arr, K, seed in sets():
        assert ((arr >= 1.0) & (arr < 65536.0)).all()
        boxes = [ka.Box(0, 0, float(w), float(h)) for w, h in arr]
        N = len(boxes)
        # the draws the seed produces, in the reference's order
        np.random.seed(seed)
        first = int(np.random.choice(N, 1)[0])
        draws = np.array([np.random.random() for _ in range(K - 1)], dtype=np.float64)
        np.random.seed(seed)
        with contextlib.redirect_stdout(quiet):
            cent = ka.init_centroids(boxes, K)
        seeds = np.zeros((K, 2))
        seeds[:len(cent)] = wh(cent)                                   # the reference's list is shorter where no index qualified
        picked = np.full(K, -1, dtype=np.int32)
        for r, c in enumerate(cent):
            picked[r] = next(i for i, b in enumerate(boxes) if b is c)
        # threshold margins
        md = np.ones(N)
        for r in range(1, len(cent)):
            md = np.minimum(md, [1 - ka.iou(b, cent[r - 1]) for b in boxes])
            s = float(np.sum(md))
            t = s * draws[r - 1]
            pre = np.cumsum(md)
            margin = np.min(np.abs(pre[max(picked[r] - 1, 0):picked[r] + 1] - t)) / s
            assert margin >= 1e-9, (name, r, margin)
        # the passes
        cents, groups, losses = [], [], []
        cur = list(cent) + [ka.Box(0, 0, 0, 0) for _ in range(K - len(cent))]
        exact_ties = name in ("same5", "int257", "four")
        for p in range(PASSES):
            d = np.array([[1 - ka.iou(b, c) if c.w > 0 else 1.0 for c in cur] for b in boxes]).reshape(N, K)
            d = np.concatenate([d, np.ones((N, 1))], axis=1)           # the start value 1 competes too
            two = np.sort(d, axis=1)[:, :2]
            gap = two[:, 1] - two[:, 0]
            assert ((gap > 1e-9) | ((gap == 0) & exact_ties)).all(), (name, p, gap.min())
            cur, grp, loss = ka.do_kmeans(K, boxes, cur)
            g = np.zeros(N, dtype=np.int8)
            index = {id(b): i for i, b in enumerate(boxes)}
            for k, members in enumerate(grp):
                for b in members:
                    g[index[id(b)]] = k
            cents.append(wh(cur)); groups.append(g); losses.append(float(loss))
        # the full loop
        np.random.seed(seed)
        with contextlib.redirect_stdout(quiet):
            final = ka.anchor_box_kmeans(boxes, K, 1e-6, 1000, plus=True)
        # iterations: replay the loop on the recorded losses
        cur = list(cent) + [ka.Box(0, 0, 0, 0) for _ in range(K - len(cent))]
        cur, _, old = ka.do_kmeans(K, boxes, cur)
        it = 1
        while True:
            cur, _, loss = ka.do_kmeans(K, boxes, cur)
            it += 1
            delta = abs(old - loss)
            if delta < 1e-6 or it > 1000:
                assert delta == 0, (name, it, delta)
                break
            assert delta > 1e-3, (name, it, delta)
            old = loss
        fin = np.zeros((K, 2))
        fin[:len(final)] = wh(final)
        if len(final) == K:
            assert np.array_equal(fin, wh(cur)), name
        out.update({name + "_boxes": arr, name + "_k": np.int32(K), name + "_seed": np.int32(seed), name + "_first": np.int32(first),
                    name + "_draws": draws, name + "_seeds": seeds, name + "_picked": picked,
                    name + "_cents": np.array(cents), name + "_groups": np.array(groups), name + "_losses": np.array(losses),
                    name + "_final": wh(cur), name + "_final_loss": np.float64(loss), name + "_iterations": np.int32(it)})
        print("%-7s N=%-5d K=%d picked=%s iterations=%d loss=%.6f" % (name, N, K, picked.tolist(), it, loss))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
