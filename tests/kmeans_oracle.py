"""Host restatement of kmeans_anchor.py (iou, init_centroids, do_kmeans, anchor_box_kmeans) with exact sums: what the device is tested
against bit for bit.  Distances are numpy float64 element operations in the reference's order (no fused multiply-add); every sum is
math.fsum, the correctly rounded exact sum; the k-means++ prefix comparison is done in Python integers (units of 2^-53).  Vectorised
over the boxes, never over anything that would change a bit.  Test infrastructure: the package never imports it."""
import math
from fractions import Fraction

import numpy as np

SCALE = 1 << 53


def distance(boxes, cw, ch):
    """1 - IoU of every box with the centroid (cw, ch), all centred at the origin (iou :35-55)"""
    w, h = boxes[:, 0], boxes[:, 1]
    inter = np.minimum(w, cw) * np.minimum(h, ch)
    return 1.0 - inter / ((w * h + cw * ch) - inter)


def assign(boxes, centroids):
    """-> (group int32 [N], min_distance [N]): start at (1, 0), replace on strict <, in centroid order"""
    best = np.ones(len(boxes), dtype=np.float64)
    group = np.zeros(len(boxes), dtype=np.int32)
    for k, (cw, ch) in enumerate(np.asarray(centroids, dtype=np.float64).reshape(-1, 2)):
        d = distance(boxes, cw, ch)
        m = d < best
        best[m] = d[m]
        group[m] = k
    return group, best


def do_kmeans(boxes, centroids):
    """-> (new centroids [K, 2], group [N], counts int64 [K], loss)"""
    centroids = np.asarray(centroids, dtype=np.float64).reshape(-1, 2)
    group, best = assign(boxes, centroids)
    new = np.zeros_like(centroids)
    counts = np.zeros(len(centroids), dtype=np.int64)
    for k in range(len(centroids)):
        sel = boxes[group == k]
        counts[k] = len(sel)
        new[k, 0] = math.fsum(sel[:, 0]) / max(len(sel), 1)
        new[k, 1] = math.fsum(sel[:, 1]) / max(len(sel), 1)
    return new, group, counts, math.fsum(best)


def prefix_exceeds(v, t):
    """P_i > t for the exact prefix sums P of the integers v (each <= 2^53, at most 2^24 of them) and a Python integer t.  The prefix
    sums need up to 77 bits, so they are carried as two int64 limbs of 27 and 50 bits: integer arithmetic, exact like Python's own
    (prefix_exceeds_plain, which the CPU test holds this against)."""
    bits = 27
    mask = (1 << bits) - 1
    lo = np.cumsum(v & mask)                                           # < 2^24 * 2^27
    hi = np.cumsum(v >> bits) + (lo >> bits)                           # < 2^24 * 2^26 + 2^24
    lo = lo & mask
    th, tl = t >> bits, t & mask
    if th >= 1 << 62:
        return np.zeros(len(v), dtype=bool)
    return (hi > th) | ((hi == th) & (lo > tl))


def prefix_exceeds_plain(v, t):
    total, out = 0, []
    for x in v:
        total += int(x)
        out.append(total > t)
    return np.array(out, dtype=bool)


def init_centroids(boxes, n_anchors, first_index, draws):
    """k-means++ from the first index and the n_anchors - 1 uniform draws -> (centroids [K, 2], picked int32 [K], sums, thresholds)"""
    cent = np.zeros((n_anchors, 2), dtype=np.float64)
    picked = np.full(n_anchors, -1, dtype=np.int32)
    cent[0], picked[0] = boxes[first_index], first_index
    md = np.ones(len(boxes), dtype=np.float64)
    sums, threshs = [], []
    for r in range(1, n_anchors):
        md = np.minimum(md, distance(boxes, cent[r - 1, 0], cent[r - 1, 1]))
        sum_distance = math.fsum(md)
        thresh = sum_distance * float(draws[r - 1])
        t = math.floor(Fraction(thresh) * SCALE)
        over = prefix_exceeds((md * float(SCALE)).astype(np.int64), t)
        if over.any():
            picked[r] = int(np.argmax(over))
            cent[r] = boxes[picked[r]]
        sums.append(sum_distance)
        threshs.append(thresh)
    return cent, picked, sums, threshs


def run(boxes, centroids, loss_convergence, iters):
    """anchor_box_kmeans :147-155 -> (centroids, counts, loss, iterations) of the last pass"""
    centroids, _, counts, old_loss = do_kmeans(boxes, centroids)
    loss = old_loss
    iterations = 1
    while True:
        centroids, _, counts, loss = do_kmeans(boxes, centroids)
        iterations += 1
        if abs(old_loss - loss) < loss_convergence or iterations > iters:
            break
        old_loss = loss
    return centroids, counts, loss, iterations


def draws_from(rng, n, n_anchors):
    """the reference's draws, in its order: choice(N, 1), then one random() per further centroid"""
    first = int(rng.choice(n, 1)[0])
    return first, np.array([rng.random_sample() for _ in range(n_anchors - 1)], dtype=np.float64)


def halfway_sets():
    """Box sets whose column sums lie exactly halfway between two doubles, built from integer multiples of the boxes' ulp: (boxes, the
    correctly rounded sums [2]).  In the first two sets the first column's tie rounds down to the even neighbour, the second's up; the
    third has no tie."""
    e, f = 2.0 ** -52, 2.0 ** -37                                      # the ulp at 1 and at 32768
    small = np.array([[1.0 + e, 1.0], [1.0, 1.0 + 3 * e]])             # 2 + e -> 2;  2 + 3e -> 2 + 4e
    large = np.array([[32768.0 + f, 40000.0], [32768.0, 40000.0 + 3 * f]])   # 65536 + f -> 65536;  80000 + 3f -> 80000 + 4f
    three = np.array([[1.0 + e, 1.0 + e], [1.0, 1.0 + 2 * e], [2.0, 2.0 + 4 * e]])   # no tie: 4 + e -> 4;  4 + 7e -> 4 + 8e
    return [(small, [2.0, 2.0 + 4 * e]), (large, [65536.0, 80000.0 + 4 * f]), (three, [4.0, 4.0 + 8 * e])]
