"""Case builders for the Soft-NMS tests (tests/test_soft_nms_cpu.py, tests/test_gpu_soft_nms.py).  numpy only.

Every builder returns (boxes [n, 4] f32, scores [n] f32, cls [n] i32); the hand-built cases carry their outcome next to them."""
import numpy as np

from wbf_cases import clustered, grid  # noqa: F401  (the random crowded lists and the lists without overlap)

F = np.float32
HARD, LINEAR, GAUSSIAN = 1, 2, 3
METHODS = (HARD, LINEAR, GAUSSIAN)
FLOOR_W = F(1e-28)                                             # the floor of w and h in the overlap


def straddle(n, head=5, seed=0):
    """One class-1 segment of exactly n rows beside a class-0 segment of `head` rows (so that the large segment does not start at row 0).
    The n boxes sit on a grid without touching, except that every eighth one is moved onto its right-hand neighbour, a fifth of the box
    aside (IoU 0.8 / 1.2 = 0.67): about one row in eight overlaps a neighbour.  Distinct scores in shuffled order."""
    gb, _, _ = grid(n, cols=64)
    for i in range(0, n - 1, 8):
        if (i + 1) % 64:                                       # (the neighbour is in the same grid row)
            gb[i] = gb[i + 1]
            gb[i, [0, 2]] -= F(0.006)
    rng = np.random.default_rng(seed)
    gs = ((rng.permutation(n).astype(F) + F(1)) / F(n + 1) * F(0.7) + F(0.25)).astype(F)
    hb, hs, _ = grid(head, seed=9)
    hb = hb + F(20.0)                                          # (anywhere: another class)
    boxes = np.concatenate([hb, gb]).astype(F)
    scores = np.concatenate([hs, gs]).astype(F)
    cls = np.concatenate([np.zeros(head), np.ones(n)]).astype(np.int32)
    return boxes, scores, cls


def _rows(rows):
    a = np.asarray(rows, np.float64).reshape(-1, 6)
    return a[:, :4].astype(F), a[:, 4].astype(F), a[:, 5].astype(np.int32)


NAN = float("nan")
W15 = float(F(1.5) * FLOOR_W)                                  # a box 1.5 floors wide
# the boxes of the chain cases: A covers B's upper half exactly (ovr 2 / 4 = 0.5), C reaches into B (ovr 0.5 / 3.5 = 1 / 7) and barely
# into A (ovr 0.5 / 5.5 = 1 / 11)
A, B, C = [0, 0, 2, 2], [0, 0, 2, 1], [1.5, 0, 3.5, 1]
B_AFTER_C = F(0.25) * (F(1.0) - F(0.5) / F(3.5))               # 0.25 decayed by linear at ovr 1 / 7: 0.2142857

# ---- hand-built cases: (name, rows [x1, y1, x2, y2, score, class], method, thr, sigma, score_floor, kept rows, their scores; None = not exact)
EXACT = [
    # a duplicate box under linear: ovr 1, weight 0, the score becomes 0 and 0 > 0 is false
    ("duplicate_linear_dropped", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 1, .8, 0]], LINEAR, 0.5, 0.5, 0.0, [0], [.9]),
    # ovr exactly 0.5 (inter 1, union 2) at thr 0.5 is not a hit: both rows keep their scores
    ("ovr_equal_thr_not_hit", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 2, .8, 0]], LINEAR, 0.5, 0.5, 0.0, [0, 1], [.9, .8]),
    ("ovr_equal_thr_not_hit_hard", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 2, .8, 0]], HARD, 0.5, 0.5, 0.0, [0, 1], [.9, .8]),
    # A decays B from 0.5 to 0.25, C is 0.25 from the start: the HIGHER row (C) is picked first and decays B once more (ovr 1 / 7 > 0.1);
    # picked the other way round B would keep 0.25 and C would fall
    ("equal_after_decay_higher_row_first", [A + [.9, 0], B + [.5, 0], C + [.25, 0]], LINEAR, 0.1, 0.5, 0.0, [0, 1, 2], [.9, float(B_AFTER_C), .25]),
    # equal scores from the start: the higher row is picked and removes the lower one
    ("equal_scores_higher_row_first", [[0, 0, 1, 1, .8, 0], [0, 0, 1, 1.1, .8, 0]], HARD, 0.5, 0.5, 0.0, [1], [.8]),
    # B falls to exactly the floor (0.5 * (1 - 0.5) = 0.25) and a far row starts at it: both dropped, the compare is strict
    ("falls_to_the_floor_exactly", [A + [.9, 0], B + [.5, 0], [7, 7, 8, 8, .25, 0]], LINEAR, 0.25, 0.5, 0.25, [0], [.9]),
    # a NaN score is never live: the row is not kept and suppresses nothing
    ("nan_score", [[0, 0, 1, 1, NAN, 0], [0, 0, 1, 1, .5, 0], [3, 3, 4, 4, .4, 0]], HARD, 0.5, 0.5, 0.0, [1, 2], [.5, .4]),
    # an inverted box of area -1 apart from a box of area 1: inter 1e-28 * 1e-28 = 0, union (1 - 1) - 0 = 0, ovr 0 / 0 = NaN - a hit
    ("inverted_box_nan_ovr_hard", [[0, 0, 1, 1, .9, 0], [3, 2, 2, 3, .8, 0]], HARD, 0.5, 0.5, 0.0, [0], [.9]),
    ("inverted_box_nan_ovr_linear", [[0, 0, 1, 1, .9, 0], [3, 2, 2, 3, .8, 0]], LINEAR, 0.5, 0.5, 0.0, [0], [.9]),
    ("inverted_box_nan_ovr_gaussian", [[0, 0, 1, 1, .9, 0], [3, 2, 2, 3, .8, 0]], GAUSSIAN, 0.5, 0.5, 0.0, [0], [.9]),
    # a box 1.5 floors wide and a zero-width box apart from it: inter = one floor, union = 1.5 - 1 = half a floor, ovr 2 - linear's
    # weight is 1 - 2 = -1, the score turns negative and the row is dropped
    ("ovr_above_one_linear_negative", [[0, 0, W15, 1, .9, 0], [5, 0, 5, 1, .8, 0]], LINEAR, 0.5, 0.5, 0.0, [0], [.9]),
    # the chain A-B-C (scores 0.9, 0.8, 0.7): A's pick takes B below C, so C is picked second and decays B again; a static order A, B, C
    # would let B decay C.  Gaussian, sigma 0.5: B = 0.8 e^-0.5 e^-(2/49) = 0.4658 falls under the floor 0.47 (static: 0.4852 stays)
    ("chain_dynamic_argmax_gaussian", [A + [.9, 0], B + [.8, 0], C + [.7, 0]], GAUSSIAN, 0.5, 0.5, 0.47, [0, 2], [.9, None]),
    # the same chain under linear at thr 0.1: B = 0.8 * 0.5 = 0.4, C (ovr 1 / 11 with A: no hit) is picked at 0.7 and takes B to 0.343
    ("chain_dynamic_argmax_linear", [A + [.9, 0], B + [.8, 0], C + [.7, 0]], LINEAR, 0.1, 0.5, 0.0, [0, 1, 2],
     [.9, float(F(F(0.8) * F(0.5)) * (F(1.0) - F(0.5) / F(3.5))), .7]),
    # classes never mix, a class with one row keeps it, a class without rows delivers nothing
    ("one_row_per_class", [[0, 0, 1, 1, .9, 0], [0, 0, 1, 1, .8, 2]], GAUSSIAN, 0.5, 0.5, 0.0, [0, 1], [.9, .8]),
    ("single_row", [[.1, .2, .3, .4, .6, 1]], LINEAR, 0.5, 0.5, 0.001, [0], [.6]),
    ("empty_list", [], GAUSSIAN, 0.5, 0.5, 0.001, [], []),
]


def exact_case(name):
    for c in EXACT:
        if c[0] == name:
            return _rows(c[1]) + c[2:]
    raise KeyError(name)
