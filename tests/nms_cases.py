"""The case table of the NMS-chain suite (tests/test_gpu_nms_stages.py on the device, tests/test_nms_cases_cpu.py without one).

A case is one call shape (entry, B, N, C) with its images and a list of runs; a run is (nms threshold, prefilter mode, the launch plan the
call must take).  The plan is written out here, field by field in PLAN order, and test_nms_cases_cpu.py checks it against the restated launch
rules (nms_stage_oracle.plan) - a change of launch_nms_pipeline's conditions that moves a case onto other kernels fails the plan assertion
on the device instead of leaving the suite green on a route it no longer tests.

PLAN = (few, fused, chunks, merge, prefilter, pre_ranks, sweep, sweep_maxn, sweep_slots, sweep_split, resolve_one, resolve_split, diou)

Branches of launch_nms_pipeline that NO case reaches, because no handle that ensure_post prepared can take them (ensure_post always provides
ctr and large_list, and N <= matrix_stride always holds):
  - `few && !wk.ctr`: bucket_kernel followed by the one-launch sort_kernel on (B, C) 1 024-thread workgroups;
  - the non-`chunks` branch: sort_kernel on 256-thread workgroups, its second launch on the large list, and the `N > YN_SORT_LARGE &&
    !chunks` launch with keys in the matrix area.
So `fused == few` and `chunks == !few` in every reachable plan.  pre_ranks = 0 under the prefilter is reached through the few route; the
other way (more than 1 024 images in one call) is not built.  sweep_split is covered in all its values (2 .. 8) with the 60 KB form; the
120 KB form (N > 16 384) is run at one image (8).

Content of the large segments (hard_segment): scores from five values (ties straddle the 64-box chunk-0 boundary and every 1 024-key chunk
boundary), partner pairs with IoU = thresh (1 + eps), exact duplicates, zero-area / negative-extent / +-1e30 / denormal / NaN / inf boxes -
the generators of test_nms_guard_band_stress_vs_oracle - with a share of small boxes so that a good part of a segment survives the prefilter.
The sweep cases (spread_segment) are built so that every box beyond the first 64 survives it; test_nms_cases_cpu.py checks that claim and
each boundary's.
"""
import functools
import zlib

import numpy as np

F = np.float32
CONF = 0.001                                                 # conf threshold of every case; class-less rows score 0.0005
PLAN = ("few", "fused", "chunks", "merge", "prefilter", "pre_ranks", "sweep", "sweep_maxn", "sweep_slots", "sweep_split", "resolve_one",
        "resolve_split", "diou")
EPS = [0.0, 1e-7, -1e-7, 3e-6, -3e-6, 2e-5, -2e-5, 1e-3, -1e-3]
SCORES = np.array([0.9, 0.7, 0.5, 0.3, 0.1], F)


def _partner(b, iou):
    """b stretched in x so that IoU(b, partner) = iou: same y extent, same x1, x2' = x1 + w / iou."""
    p = b.copy()
    p[2] = F(b[0] + (b[2] - b[0]) / iou)
    return p


def _degenerate():
    return np.array([[0.3, 0.3, 0.3, 0.3], [0.5, 0.5, 0.4, 0.4], [-1e30, -1e30, 1e30, 1e30], [0.2, 0.2, 0.2 + 1e-20, 0.2 + 1e-20],
                     [np.nan, 0.1, 0.5, 0.5], [0.1, 0.1, np.inf, 0.5]], F)       # zero area, negative extent, inf area, denormal area, NaN, inf


def hard_segment(rs, n, thresh, small=0.5):
    """n boxes + scores of one class: the guard-band test's content (see the module docstring)."""
    base = rs.uniform(0.1, 0.6, (n, 2)); wh = rs.uniform(0.05, 0.3, (n, 2))
    if small == 0.0:                                          # clustered: 40 centres, boxes of similar size around them (the prefilter removes most)
        base = rs.uniform(0.1, 0.8, (40, 2))[rs.randint(0, 40, n)] + rs.normal(0, 0.01, (n, 2)); wh = rs.uniform(0.05, 0.08, (n, 2))
    sm = rs.rand(n) < small
    base[sm] = rs.uniform(0.02, 0.95, (int(sm.sum()), 2)); wh[sm] *= 0.03
    boxes = np.concatenate([base, base + wh], 1).astype(F)
    t = max(thresh, 0.05)
    for k in range(0, n - 1, 2):
        if rs.rand() < 0.6:
            boxes[k + 1] = _partner(boxes[k], min(t * (1.0 + EPS[rs.randint(len(EPS))]), 0.999))
    for k in rs.randint(0, n, n // 30):                       # exact duplicates
        boxes[k] = boxes[rs.randint(0, n)]
    deg = _degenerate()
    if n >= 8:
        for r in range(1 + n // 2000):
            boxes[rs.choice(n, len(deg), replace=False)] = deg
    else:
        boxes[:n] = np.roll(deg, n, 0)[:n]
    return boxes, SCORES[rs.randint(0, len(SCORES), n)]


def spread_segment(rs, n, thresh, irregular=0, wide=0, lo=-0.3, hi=1.4):
    """n boxes + scores whose boxes beyond the first 64 ALL survive the prefilter (n2 = n - 64): the 64 best-scored ones (one tie group, 0.99)
    are isolated near-points; the rest are near-points over [lo, hi) (negative coordinates and coordinates above 1) with, among them,
    threshold-adjacent partner pairs (intersecting x-extents), pairs whose x-extents touch exactly (x2_i == x1_j) with overlapping y,
    `irregular` zero-area / negative-extent / denormal boxes and `wide` full-width strips."""
    ctr = rs.uniform(lo, hi, (n, 2)); wh = rs.uniform(1e-5, 2e-3, (n, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(F)
    score = SCORES[rs.randint(0, len(SCORES), n)]
    score[:64] = F(0.99)
    t = max(thresh, 0.05)
    k = 64
    for _ in range(min(40, (n - 64) // 8)):                   # partner pairs, then touching pairs
        boxes[k + 1] = _partner(boxes[k], min(t * (1.0 + EPS[rs.randint(len(EPS))]), 0.999)); k += 2
    for _ in range(min(40, (n - 64) // 8)):
        boxes[k + 1] = boxes[k]; boxes[k + 1, 0] = boxes[k, 2]; boxes[k + 1, 2] = F(boxes[k, 2] + (boxes[k, 2] - boxes[k, 0])); k += 2
    for i in range(wide):                                     # full-width strips at distinct heights
        y = F(lo + (hi - lo) * (i + 0.5) / wide)
        boxes[k] = [lo - 0.01, y, hi + 0.01, y + F(1e-4)]; k += 1
    for i in range(irregular):
        p = rs.uniform(0.0, 1.0, 2)
        boxes[k] = ([p[0], p[1], p[0], p[1] + 0.01], [p[0] + 0.01, p[1] + 0.01, p[0], p[1]], [p[0], p[1], p[0] + 1e-20, p[1] + 1e-20])[i % 3]
        score[k] = F(0.1); k += 1
    assert k <= n
    return boxes, score


def make_image(rs, N, C, segs):
    """segs: {class: (boxes, scores)} -> (boxes [N, 4], conf [N, C] one-hot rows; the rest are class-less rows below CONF), rows shuffled."""
    boxes = np.zeros((N, 4), F); conf = np.zeros((N, C), F)
    k = 0
    for c, (b, s) in segs.items():
        boxes[k:k + len(b)] = b; conf[np.arange(k, k + len(b)), c] = s; k += len(b)
    assert k <= N, (k, N)
    ctr = rs.uniform(0.05, 0.95, (N - k, 2)); wh = rs.uniform(0.02, 0.09, (N - k, 2))
    boxes[k:] = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
    conf[np.arange(k, N), rs.randint(0, C, N - k)] = F(0.0005)
    perm = rs.permutation(N)
    return boxes[perm], conf[perm]


class Case:
    def __init__(self, name, entry, B, N, C, build, image_of, runs, diou=False, repeat=False, claims=None):
        self.name, self.entry, self.B, self.N, self.C, self.diou, self.repeat = name, entry, B, N, C, diou, repeat
        self._build, self.image_of, self.runs, self.claims = build, image_of, runs, claims or {}
        assert len(image_of) == B

    @functools.lru_cache(maxsize=None)
    def images(self, thresh):
        """The distinct images of the case (the partner pairs follow the threshold), each (boxes [N, 4], conf [N, C])."""
        imgs = self._build(np.random.RandomState(zlib.crc32(self.name.encode()) % 100000 + int(thresh * 1000)), thresh)
        for b, c in imgs:
            assert b.shape == (self.N, 4) and c.shape == (self.N, self.C)
        return imgs

    def plan_of(self, run):
        return dict(zip(PLAN, run[2]))


def _sizes(rs, thresh, N, C, sizes, small=0.5):
    return make_image(rs, N, C, {c: hard_segment(rs, n, thresh, small) for c, n in sizes.items() if n})


# ---- the route cases ---------------------------------------------------------------------------------------------------------------------
FEW_SIZES = dict(zip(range(11), [0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]))
MANY_A = dict(zip(range(7), [1023, 1024, 1025, 2047, 2048, 2049, 3000]))               # class 7 stays empty
MANY_B = dict(zip(range(7), [576, 577, 640, 641, 1088, 1089, 700]))                    # 700: a fifth sliceable class (one workgroup)
#          few fu ch mg pre rk  sw  maxn sl sp one rs diou
P_FEW0 = (1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0)
P_FEW2 = (1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0)
P_MANY = (0, 0, 1, 1, 1, 4, 1, 3072, 4, 8, 0, 1, 0)
P_MANY_NOSWEEP = (0, 0, 1, 1, 1, 4, 0, 0, 0, 0, 0, 1, 0)
P_MERGE = (0, 0, 1, 1, 1, 4, 1, 3072, 3, 8, 0, 1, 0)
P_17K0 = (0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0)
P_17K2 = (0, 0, 1, 1, 1, 3, 1, 6144, 3, 8, 1, 0, 0)
P_DIOU = (0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1)


def _sweep_a(rs, t):
    # n2 = 1 024 stays dense, 1 025 is swept; 3 072 is swept, 3 073 stays dense (sweep_maxn = 3 072): the image's four largest classes
    return make_image(rs, 12288, 70, {0: spread_segment(rs, 1088, t), 1: spread_segment(rs, 1089, t), 2: spread_segment(rs, 3136, t),
                                      3: spread_segment(rs, 3137, t), 9: hard_segment(rs, 500, t)})


def _sweep_b(rs, t):
    # 64 irregular boxes: swept, 65: dense; 260 full-width strips among ~2 800 near-points (more than YN_SWEEP_WIDE: the estimate sits
    # between half the limit and the limit - either decision allowed, same bits both ways); a plain spread class; a FIFTH listed class: dense
    return make_image(rs, 12288, 70, {0: spread_segment(rs, 1264, t, irregular=64), 1: spread_segment(rs, 1265, t, irregular=65),
                                      2: spread_segment(rs, 3124, t, wide=260), 3: spread_segment(rs, 1500, t), 4: spread_segment(rs, 1100, t)})


SWEEP_A_CLAIMS = {0: dict(n2=1024, sparse=0), 1: dict(n2=1025, sparse=1), 2: dict(n2=3072, sparse=1), 3: dict(n2=3073, sparse=0)}
SWEEP_B_CLAIMS = {0: dict(n2=1200, sparse=1, irregular=64), 1: dict(n2=1201, sparse=0, irregular=65), 2: dict(n2=3060, sparse=None, wide=260),
                  3: dict(n2=1436, sparse=1), 4: dict(n2=1036, sparse=0, fifth=True)}
# N > 16 384: sweep_maxn = 6 144.  n2 = 6 144 is swept, 6 145 stays dense; 260 full-width strips among 4 323 near-points: swept, unambiguously
SWEEP_C_CLAIMS = {0: dict(n2=6144, sparse=1), 1: dict(n2=6145, sparse=0), 2: dict(n2=4519, sparse=1, wide=260)}


def _plan_image(N, C):
    def build(rs, t):
        segs = {0: spread_segment(rs, min(N - 40, 1090), t)}
        if C > 1:
            segs[C - 1] = hard_segment(rs, 30, t)
        return [make_image(rs, N, C, segs)]
    return build


def _plan_case(B, N, C, plan):
    return Case("plan-B%d-N%d-C%d" % (B, N, C), "postprocess", B, N, C, _plan_image(N, C), [0] * B, [(0.5, 1, plan)])


CASES = [
    Case("few-fused", "postprocess", 1, 4096, 20, lambda rs, t: [_sizes(rs, t, 4096, 20, FEW_SIZES)], [0],
         [(0.5, 0, P_FEW0), (0.5, 2, P_FEW2), (0.3, 0, P_FEW0), (0.3, 2, P_FEW2)]),
    Case("few-full-lds", "postprocess", 1, 16384, 2, lambda rs, t: [_sizes(rs, t, 16384, 2, {1: 16384})], [0],
         [(0.5, 0, P_FEW0), (0.5, 2, P_FEW2), (0.3, 0, P_FEW0), (0.3, 2, P_FEW2)]),
    Case("many", "postprocess", 4, 12288, 70, lambda rs, t: [_sizes(rs, t, 12288, 70, MANY_A), _sizes(rs, t, 12288, 70, MANY_B, small=0.0)],
         [0, 1, 1, 0], [(0.5, 1, P_MANY), (0.3, 1, P_MANY), (1e-6, 1, P_MANY), (0.0, 1, P_MANY_NOSWEEP)], repeat=True),
    Case("merge", "merge", 1, 3000, 300, lambda rs, t: [_sizes(rs, t, 3000, 300, {7: 2500, 150: 300, 299: 150, 0: 50})], [0],
         [(0.5, 2, P_MERGE), (0.3, 2, P_MERGE)], repeat=True),
    Case("n17000", "postprocess", 1, 17000, 3, lambda rs, t: [_sizes(rs, t, 17000, 3, {0: 16400, 1: 500, 2: 100})], [0],
         [(0.5, 0, P_17K0), (0.5, 2, P_17K2), (0.3, 0, P_17K0), (0.3, 2, P_17K2)]),
    Case("diou", "postprocess", 4, 3200, 70, lambda rs, t: [_sizes(rs, t, 3200, 70, {3: 1025, 40: 2049, 69: 100})], [0, 0, 0, 0],
         [(0.5, 1, P_DIOU), (0.3, 1, P_DIOU)], diou=True, repeat=True),
    Case("sweep-3072", "postprocess", 4, 12288, 70, lambda rs, t: [_sweep_a(rs, t), _sweep_b(rs, t)], [0, 1, 1, 0],
         [(0.5, 1, P_MANY), (0.3, 1, P_MANY)], repeat=True, claims={0: SWEEP_A_CLAIMS, 1: SWEEP_B_CLAIMS}),
    Case("sweep-6144", "postprocess", 1, 17000, 3,
         lambda rs, t: [make_image(rs, 17000, 3, {0: spread_segment(rs, 6208, t), 1: spread_segment(rs, 6209, t), 2: spread_segment(rs, 4583, t, wide=260)})],
         [0], [(0.5, 2, P_17K2), (0.3, 2, P_17K2)], claims={0: SWEEP_C_CLAIMS}),
    # the remaining values of the plan's fields: pre_ranks 1 .. 3, sweep_slots 1 .. 3, sweep_split 2 .. 7, no merge on the chunked route
    _plan_case(257, 1100, 1, (0, 0, 1, 1, 1, 1, 1, 3072, 1, 2, 0, 1, 0)),
    _plan_case(129, 130, 2, (0, 0, 1, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0)),
    _plan_case(86, 1100, 3, (0, 0, 1, 1, 1, 3, 1, 3072, 2, 2, 0, 1, 0)),
    _plan_case(65, 2100, 4, (0, 0, 1, 1, 1, 4, 1, 3072, 3, 3, 0, 1, 0)),
    _plan_case(52, 1100, 5, (0, 0, 1, 1, 1, 4, 1, 3072, 2, 4, 0, 1, 0)),
    _plan_case(43, 1100, 6, (0, 0, 1, 1, 1, 4, 1, 3072, 2, 5, 0, 1, 0)),
    _plan_case(37, 1100, 7, (0, 0, 1, 1, 1, 4, 1, 3072, 2, 6, 0, 1, 0)),
    _plan_case(33, 1100, 8, (0, 0, 1, 1, 1, 4, 1, 3072, 2, 7, 0, 1, 0)),
]
BY_NAME = {c.name: c for c in CASES}
RUNS = [(c.name, i) for c in CASES for i in range(len(c.runs))]
