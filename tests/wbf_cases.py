"""Case builders for the weighted box fusion tests (tests/test_wbf_cpu.py, tests/test_gpu_wbf.py).  numpy only.

Every builder returns (boxes [n, 4] f32, scores [n] f32, cls [n] i32); the hand-built ones carry their outcome next to them."""
import numpy as np

F = np.float32


def clustered(seed, C=3, objects=12, views=22, sigma=0.012, clutter=40):
    """`objects` objects seen by up to `views` forwards each (the box jittered with `sigma` of the side, a view missing now and then)
    plus `clutter` boxes that one forward alone saw; distinct scores; rows shuffled.  With the defaults about 220 rows end in about 55
    clusters at thr 0.55, a quarter of them with two or more votes."""
    rng = np.random.default_rng(seed)
    b, c = [], []
    for _ in range(objects):
        ctr = rng.random(2) * 0.7 + 0.15
        wh = rng.random(2) * 0.2 + 0.1
        k = int(rng.integers(0, C))
        nv = int(rng.integers(views // 2, views + 1))
        for _ in range(nv):
            j = rng.standard_normal(4) * sigma
            b.append([ctr[0] - wh[0] / 2 + j[0], ctr[1] - wh[1] / 2 + j[1], ctr[0] + wh[0] / 2 + j[2], ctr[1] + wh[1] / 2 + j[3]])
            c.append(k)
    for _ in range(clutter):
        ctr = rng.random(2) * 0.9 + 0.05
        wh = rng.random(2) * 0.08 + 0.02
        b.append([ctr[0] - wh[0] / 2, ctr[1] - wh[1] / 2, ctr[0] + wh[0] / 2, ctr[1] + wh[1] / 2])
        c.append(int(rng.integers(0, C)))
    n = len(b)
    order = rng.permutation(n)
    boxes = np.asarray(b, F)[order]
    cls = np.asarray(c, np.int32)[order]
    scores = ((rng.permutation(n).astype(F) + F(1)) / F(2 * n) + F(0.25)).astype(F)      # all different, 0.25 .. 0.75
    return boxes, scores, cls


def grid(n, C=1, cell=0.04, size=0.03, cols=24, seed=0):
    """n boxes on a grid that do not touch each other (IoU 0 between any two), class i % C, distinct scores in shuffled order."""
    i = np.arange(n)
    x = (i % cols).astype(F) * F(cell); y = (i // cols).astype(F) * F(cell)
    boxes = np.stack([x, y, x + F(size), y + F(size)], 1).astype(F)
    scores = ((np.random.default_rng(seed).permutation(n).astype(F) + F(1)) / F(2 * n + 2) + F(0.25)).astype(F)
    return boxes, scores, (i % C).astype(np.int32)


def straddle(K, joiners=3, head=5, C=3):
    """One class-1 segment that ends in exactly K clusters: K grid boxes with DESCENDING scores (cluster k = grid box k) plus `joiners`
    copies, shifted by a tenth of the box, of the LAST `joiners` grid boxes with lower scores (each joins its box: IoU 0.9 / 1.1 = 0.82);
    `head` class-0 rows in front, so that the segment does not start at row 0.  Outcome: head + K clusters, the last `joiners` class-1
    clusters with 2 votes."""
    gb, _, _ = grid(K)
    gs = (F(0.9) - np.arange(K).astype(F) / F(4 * K)).astype(F)
    jb = gb[K - joiners:].copy()
    jb[:, [0, 2]] += F(0.003)
    js = (F(0.2) - np.arange(joiners).astype(F) / F(64)).astype(F)
    hb, hs, _ = grid(head, seed=9)
    hb = hb + F(0.5)                                           # (anywhere: another class)
    boxes = np.concatenate([hb, gb, jb]).astype(F)
    scores = np.concatenate([hs, gs, js]).astype(F)
    cls = np.concatenate([np.zeros(head), np.ones(K + joiners)]).astype(np.int32)
    assert C >= 2
    return boxes, scores, cls


def _rows(rows):
    a = np.asarray(rows, np.float64)
    return a[:, :4].astype(F), a[:, 4].astype(F), a[:, 5].astype(np.int32)


# ---- hand-built exact cases: (name, rows [x1, y1, x2, y2, score, class], thr, E, expected votes per delivered cluster, expected founders) ----
EXACT = [
    # IoU of exactly 0.5 (inter 1, union 2) is not above thr 0.5: two clusters
    ("iou_equal_thr_no_join", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 2, .8, 0]], 0.5, 1, [1, 1], [0, 1]),
    # the neighbour just above (inter 1, union 1.9): one cluster of two
    ("iou_above_thr_joins", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 1.9, .8, 0]], 0.5, 1, [2], [0]),
    # equal scores: the higher row is visited first and founds the cluster
    ("equal_scores_higher_row_first", [[0, 0, 1, 1, .8, 0], [0, 0, 1, 1.1, .8, 0]], 0.5, 2, [2], [1]),
    # row 2 meets clusters 0 and 1 at the same ovr 0.5 / 2.5: the lowest cluster (founder row 0) takes it
    ("equal_ovr_lowest_cluster", [[0, 0, 1, 1, .9, 0], [2, 0, 3, 1, .8, 0], [.5, 0, 2.5, 1, .7, 0]], 0.1, 1, [2, 1], [0, 1]),
    # the same with the rows of the two founders swapped: the earlier CLUSTER is now the one founded by row 1
    ("equal_ovr_lowest_cluster_swapped", [[0, 0, 1, 1, .8, 0], [2, 0, 3, 1, .9, 0], [.5, 0, 2.5, 1, .7, 0]], 0.1, 1, [1, 2], [0, 1]),
    # drift: row 2 has IoU 0.38 with the founder but 0.54 with the fused box of rows 0 + 1 - it joins
    ("drift_joins_fused_not_founder", [[0, 0, 1, 1, .9, 0], [.3, 0, 1.3, 1, .89, 0], [.45, 0, 1.45, 1, .5, 0]], 0.5, 1, [3], [0]),
    # drift the other way: row 2 has IoU 0.54 with the founder but 0.38 with the fused box - it founds its own cluster
    ("drift_leaves_founder", [[0, 0, 1, 1, .9, 0], [.3, 0, 1.3, 1, .89, 0], [-.3, 0, .7, 1, .5, 0]], 0.5, 1, [2, 1], [0, 2]),
    # classes never mix, and a class without rows delivers nothing
    ("classes_apart", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 1, .8, 2]], 0.5, 1, [1, 1], [0, 1]),
    # a zero-area box: its floors make inter 1e-28 * h, far below any threshold; two identical ones have union -inter, ovr -1
    ("zero_area", [[.2, .2, .2, .5, .9, 0], [.2, .2, .2, .5, .8, 0], [.1, .1, .4, .6, .7, 0]], 0.5, 1, [1, 1, 1], [0, 1, 2]),
    # a NaN coordinate makes every ovr with that row NaN: it never joins and nothing joins it
    ("nan_coordinate", [[0, 0, 1, 1, .9, 0], [0, float("nan"), 1, 1, .8, 0], [0, 0, 1, 1.05, .7, 0]], 0.5, 1, [2, 1], [0, 1]),
    # more votes than expected are capped: 3 votes at E = 2 score (S / 3) * (2 / 2)
    ("votes_above_expected", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 1.02, .8, 0], [0, 0, 1.02, 1, .7, 0]], 0.5, 2, [3], [0]),
    # a single row
    ("single_row", [[.1, .2, .3, .4, .6, 1]], 0.55, 22, [1], [0]),
]


def exact_case(name):
    for c in EXACT:
        if c[0] == name:
            return _rows(c[1]) + c[2:]
    raise KeyError(name)
