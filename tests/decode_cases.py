"""What tests/test_gpu_decode_ops.py and tests/test_decode_cases_cpu.py share: the case tables of the score / box decode front ends of
csrc/kernels_post.hip, a restatement in Python of the rules by which the launchers pick a kernel (launch_decode's KMAX, launch_head_decode's
(NT, KMAX), head_tail_ok, the fusion decision of the forward), the float64 reference of the decode (and a float32 numpy evaluation of the same
formulas: the e32 of f64_bar.bar), the float64 / float32 reference of the head tail (layers .2, .3, .4), and the regimes the steered data must reach.

Layout.  A raw head is NHWC [B, w, w, A (5 + C)], one row per pixel = [A objectness | A x C class logits | A x 4 box logits]; candidate n of an
image = off[scale] + cell * A + anchor, cell = gy * w + gx (models/yolo_nano.py:308-330).

Which candidates share a wavefront (the fast / general / skip decisions are taken per wavefront of four candidates) differs per front end:
  decode_kernel          four consecutive candidates of the flat index b * N + n
  head_decode_block      four consecutive candidates of one scale's flat index (b * hw + cell) * A + anchor
  head_tail_block        four consecutive candidates of an 8 x 4 pixel tile, (ty * 8 + tx) * A + anchor
wave_groups() restates the three; the regimes that are a property of a wavefront are computed per grouping.
"""
import functools
import math

import numpy as np

from yolo_nano_amd import arch

A = 3
B = 2
ANCHORS = np.asarray(arch.MULTI_ANCHOR_SIZE, dtype=np.float64).reshape(3, A, 2)
NECK = 96

# =====================================================================================================================================
# the launchers' rules
# =====================================================================================================================================
KMAX_ALL = (1, 2, 5, 16, 64)
HEAD_DECODE_VARIANTS = ((1, 1), (1, 2), (1, 5), (2, 5))


def kmax(C):
    """launch_decode: 16 * KMAX >= C"""
    return 1 if C <= 16 else (2 if C <= 32 else (5 if C <= 80 else (16 if C <= 256 else 64)))


def decode_kernel(C, full):
    return "decode_kernel<%s,%d>" % ("true" if full else "false", kmax(C))


def npad(C):
    return (A * (5 + C) + 31) // 32 * 32


def head_decode_supported(C):
    return npad(C) <= 256 and C <= 80


def head_decode_variant(C):
    """launch_head_decode(_group): (NT, KMAX)"""
    if npad(C) > 128:
        return (2, 5)
    return (1, 1) if C <= 16 else ((1, 2) if C <= 32 else (1, 5))


def head_tail_ok(C):
    return 32 < C <= 80 and 128 < npad(C) <= 256


SWITCHES = [(tail, fuse, group) for tail in (0, 1) for fuse in (0, 1, 2) for group in (0, 1)]     # yn_tail_fuse, yn_fuse_decode, yn_group_launch


def front_end(C, S, tail, fuse, group):
    """the decode kernels a forward over B images of S x S runs behind layer .1, in launch order (head_fuse_all + run_head_tail of csrc/yn_api.hip;
    the weights of every case fit the split-f16 range, so the grouped launches are available)"""
    fuse_all = fuse != 0 and head_decode_supported(C)
    tail_possible = fuse_all and tail and group and C > 32 and 128 < npad(C) <= 256
    if fuse != 2 and B * (S // 8) ** 2 < 8192 and not tail_possible:
        fuse_all = False
    if not fuse_all:
        return [decode_kernel(C, False)]
    if group and tail and head_tail_ok(C):
        return ["head_tail_group_kernel<5>"]
    if group:
        return ["head_decode_group_kernel<%d,%d>" % head_decode_variant(C)]
    return ["head_decode_kernel<%d,%d>" % head_decode_variant(C)] * 3


def is_decode_kernel(name):
    return name.startswith(("decode_kernel", "head_decode", "head_tail"))


# =====================================================================================================================================
# geometry
# =====================================================================================================================================
def maps(S):
    return [S // s for s in arch.STRIDES]


def num_pred(S):
    return sum(A * w * w for w in maps(S))


@functools.lru_cache(maxsize=None)
def geometry(S):
    """per candidate of one image: scale, gx, gy, anchor (int arrays [N])"""
    sc, gx, gy, an = [], [], [], []
    for s, w in enumerate(maps(S)):
        cell = np.repeat(np.arange(w * w), A)
        sc.append(np.full(w * w * A, s)); gx.append(cell % w); gy.append(cell // w); an.append(np.tile(np.arange(A), w * w))
    return tuple(np.concatenate(v) for v in (sc, gx, gy, an))


def wave_groups(front, S):
    """[B * N] an id per candidate, equal for the candidates that share a wavefront in that front end ("decode", "head_decode", "head_tail").
    A wavefront with fewer than four candidates (the end of an index range; in head_tail also a tile that reaches past the image, whose outside
    pixels the reference does not model) has id -1."""
    N = num_pred(S)
    sc, gx, gy, an = geometry(S)
    out = np.empty((B, N), np.int64)
    if front == "decode":
        out[:] = (np.arange(B * N) // 4).reshape(B, N)
    else:
        base = 0
        for s, w in enumerate(maps(S)):
            m = sc == s
            for b in range(B):
                if front == "head_decode":
                    out[b, m] = base + ((b * w * w + gy[m] * w + gx[m]) * A + an[m]) // 4
                else:
                    tx_n, ty_n = (w + 7) // 8, (w + 3) // 4
                    tile = (b * ty_n + gy[m] // 4) * tx_n + gx[m] // 8
                    out[b, m] = base + tile * 24 + (((gy[m] % 4) * 8 + gx[m] % 8) * A + an[m]) // 4
            base += 1 << 20
    flat = out.reshape(-1)
    _, inv, cnt = np.unique(flat, return_inverse=True, return_counts=True)
    return np.where(cnt[inv] == 4, flat, -1)


def unpack_heads(heads, C):
    """three raw heads [B, w, w, A (5 + C)] -> obj [B, N], cls [B, N, C], box [B, N, 4] in candidate order"""
    o, c, t = [], [], []
    for h in heads:
        Bn, w = h.shape[0], h.shape[1]
        r = h.reshape(Bn, w * w, A * (5 + C))
        o.append(r[:, :, :A].reshape(Bn, w * w * A))
        c.append(r[:, :, A:A * (1 + C)].reshape(Bn, w * w * A, C))
        t.append(r[:, :, A * (1 + C):].reshape(Bn, w * w * A, 4))
    return np.concatenate(o, 1), np.concatenate(c, 1), np.concatenate(t, 1)


def pack_heads(obj, cls, box, S):
    """the inverse of unpack_heads"""
    Bn, N, C = cls.shape
    heads, off = [], 0
    for w in maps(S):
        n = w * w * A
        h = np.concatenate([obj[:, off:off + n].reshape(Bn, w * w, A), cls[:, off:off + n].reshape(Bn, w * w, A * C),
                            box[:, off:off + n].reshape(Bn, w * w, A * 4)], -1)
        heads.append(np.ascontiguousarray(h.reshape(Bn, w, w, A * (5 + C)), dtype=np.float32))
        off += n
    return heads


# =====================================================================================================================================
# the reference: models/yolo_nano.py:308-330 (split), :120-156 (boxes), :362-367 (scores), :253-261 (arg-max, threshold)
# =====================================================================================================================================
def decode_ref(heads, S, C, dtype=np.float64):
    """-> dict: all_bbox [B,N,4], all_class [B,N,C], best [B,N] (first maximum), score [B,N], x [B,N,C] = logit - max, p [B,N,C] the softmax,
    obj [B,N] the sigmoid, obj_raw; every operation in `dtype` (float64: the reference; float32: its e32)"""
    f = dtype
    obj_raw, cls, t = (v.astype(f) for v in unpack_heads(heads, C))
    sc, gx, gy, an = geometry(S)
    with np.errstate(all="ignore"):
        x = cls - cls.max(-1, keepdims=True)
        e = np.exp(x)
        p = e / e.sum(-1, keepdims=True)
        obj = f(1) / (f(1) + np.exp(-obj_raw))
        all_class = p * obj[..., None]
        stride = np.asarray(arch.STRIDES, dtype=f)[sc]
        anc = ANCHORS.astype(f)[sc, an]                                                  # [N, 2]
        cxy = (f(1) / (f(1) + np.exp(-t[..., :2])) + np.stack([gx, gy], -1).astype(f)) * stride[:, None]
        wh = np.exp(t[..., 2:]) * anc
        box = np.concatenate([cxy - wh / f(2), cxy + wh / f(2)], -1) / f(S)
        pre = box.copy()
        box = np.clip(box, f(0), f(1))
    key = np.where(np.isnan(all_class), -np.inf, all_class)                              # numpy's argmax returns the first NaN; such rows never pass the threshold
    best = key.argmax(-1)
    score = np.take_along_axis(all_class, best[..., None], -1)[..., 0]
    return dict(all_bbox=box, pre_clamp=pre, all_class=all_class, best=best, score=score, x=x, p=p, obj=obj, obj_raw=obj_raw, cls=cls, t=t)


def skip_logit(conf):
    return math.log(conf / (1.0 - conf)) - 0.01 if 0.0 < conf < 1.0 else -math.inf


# =====================================================================================================================================
# the head tail: depthwise 3x3 + bias + leaky, pointwise 96 -> 96 + bias + leaky, last conv + bias (models/yolo_nano.py:60-82, 299-301)
# =====================================================================================================================================
def tail_ref(x, wd, bd, wp, bp, wf, bf, dtype=np.float64):
    """x [B,w,w,96] NHWC, folded weights wd [96,1,3,3], wp [96,96,1,1], wf [A(5+C),96,1,1] -> raw head [B,w,w,A(5+C)], every operation in dtype"""
    f = dtype
    x, wd, bd, wp, bp, wf, bf = (np.asarray(v).astype(f) for v in (x, wd, bd, wp, bp, wf, bf))
    leaky = lambda v: np.where(v > 0, v, f(0.1) * v)
    Bn, H, W, Cc = x.shape
    xp = np.zeros((Bn, H + 2, W + 2, Cc), f)
    xp[:, 1:-1, 1:-1] = x
    acc = np.zeros_like(x) + bd
    for ky in range(3):
        for kx in range(3):
            acc = acc + xp[:, ky:ky + H, kx:kx + W] * wd[:, 0, ky, kx]
    y = leaky(acc)
    y = leaky(y @ wp[:, :, 0, 0].T + bp)
    return (y @ wf[:, :, 0, 0].T + bf).astype(f)


BN_ONE_VAR = np.float32(1.0) - np.float32(arch.BN_EPS)      # running_var with fl32(var + eps) == 1 (asserted by the CPU test): gamma 1 folds to factor 1


def head_keys(hd):
    n = "head_det_%d" % hd
    return [("%s.%d.convs.0" % (n, j), "%s.%d.convs.1" % (n, j)) for j in (2, 3)] + [(n + ".4", None)]


def selection_layers(C):
    """folded weights of the steered tail: layer .2 the centre tap, layer .3 the identity, layer .4 column n reads channel n mod 96; the bias
    of a column carries the offset (STEER_BIAS)"""
    nc = A * (5 + C)
    wd = np.zeros((NECK, 1, 3, 3), np.float32); wd[:, 0, 1, 1] = 1
    wp = np.zeros((NECK, NECK, 1, 1), np.float32); wp[np.arange(NECK), np.arange(NECK)] = 1
    wf = np.zeros((nc, NECK, 1, 1), np.float32); wf[np.arange(nc), np.arange(nc) % NECK] = 1
    return wd, np.zeros(NECK, np.float32), wp, np.zeros(NECK, np.float32), wf, steer_bias(C)


def steer_bias(C):
    """-60 on every column: activations in [0, 120] in steps of 1/8 give raw values in [-60, 60].  Two class columns of every anchor sit
    2**-17 and 2**-16 lower (e = 0.9999924 and 0.9999847 against an equal activation: just inside and just outside the general path's
    window); the box columns sit at -58 (box logits around 0)"""
    b = np.full(A * (5 + C), -60.0, np.float32)
    b[:A] = -60.125                                         # objectness: levels 0, 0.125, 0.25 give -60.125, -60, -59.875
    for a in range(A):
        if C >= 3:
            b[A + a * C + 1] = -60.0 - 2.0 ** -17
            b[A + a * C + 2] = -60.0 - 2.0 ** -16
    b[A * (1 + C):] = -58.0
    return b


def steered_state_dict(sd, C):
    """sd with the layers .2, .3, .4 of the three heads replaced by selection_layers (BatchNorm folded to the identity)"""
    sd = dict(sd)
    wd, bd, wp, bp, wf, bf = selection_layers(C)
    for hd in (1, 2, 3):
        for (conv, bn), w, b in zip(head_keys(hd), (wd, wp, wf), (bd, bp, bf)):
            sd[conv + ".weight"], sd[conv + ".bias"] = w.copy(), b.copy()
            if bn:
                sd[bn + ".weight"] = np.ones(NECK, np.float32); sd[bn + ".bias"] = np.zeros(NECK, np.float32)
                sd[bn + ".running_mean"] = np.zeros(NECK, np.float32); sd[bn + ".running_var"] = np.full(NECK, BN_ONE_VAR, np.float32)
    return sd


# =====================================================================================================================================
# case tables
# =====================================================================================================================================
DECODE_C = (1, 3, 16, 17, 20, 32, 33, 80, 81, 256, 257)     # both sides of every KMAX boundary
DECODE_S = (96, 64)                                         # maps 12 / 6 / 3 (N = 567: 35 full 16-candidate blocks + a partial one) and 8 / 4 / 2
DECODE_CASES = {"d-c%d-s%d" % (C, S): (C, S) for C in DECODE_C for S in DECODE_S}
CONF_RANDOM, CONF_STEERED = 0.25, 0.001                     # random: objectness ~ N(0, 2) spans logit(0.25) = -1.1; steered: even 1 / 257 passes

HEAD_TAIL_C = (80, 20, 16, 37)                              # head_tail_group_kernel<5> + <2,5>; <1,2>; <1,1>; <1,5> with Npad = 128
HEAD_TAIL_CASES = {"t-c%d-s%d" % (C, S): (C, S) for C in HEAD_TAIL_C for S in DECODE_S}

NEAR = math.log(0.99999)
OBJ_EDGES = (-59.875, -60.0, -60.125, -104.0, 40.0)
TWH = (-104.0, -88.0, 0.0, 88.0, 89.0, 104.0)
TXY = (-104.0, -20.0, 0.0, 20.0, 104.0)
MARGIN_OBJ = -6.9140625                                     # between logit(0.001) - 0.01 = -6.91675 and logit(0.001) = -6.90675
BELOW_OBJ = -8.0


def _frac(rs, lo, hi, *shape):
    """exact binary fractions: multiples of 1/8 in [lo, hi]"""
    return rs.randint(int(lo * 8), int(hi * 8) + 1, size=shape).astype(np.float32) / np.float32(8)


@functools.lru_cache(maxsize=None)
def random_heads(C, S, seed=7):
    """normal logits; objectness ~ N(0, 2) spans both sides of logit(CONF_RANDOM); class logits ~ N(0, 2); box logits ~ N(0, 1)"""
    rs = np.random.RandomState(seed + 1000 * C + S)
    N = num_pred(S)
    obj = (2.0 * rs.standard_normal((B, N))).astype(np.float32)
    cls = (2.0 * rs.standard_normal((B, N, C))).astype(np.float32)
    box = rs.standard_normal((B, N, 4)).astype(np.float32)
    return pack_heads(obj, cls, box, S)


def _class_recipes(C):
    """[(name, f(rs) -> class logits [C])]: what one candidate's class slice can be steered to"""
    hi = np.float32(2.0)

    def base(rs):
        return np.minimum(_frac(rs, -4, 1, C), np.float32(1.0))

    def tie(idx):
        def f(rs):
            v = base(rs)
            v[list(idx)] = hi
            return v
        return f

    def near(delta):
        def f(rs):
            v = base(rs)
            v[0 if C < 3 else C // 2] = hi
            v[C - 1] = hi + np.float32(delta)
            return v
        return f

    def one_finite(rs):
        v = np.full(C, -np.inf, np.float32)
        v[C // 3] = np.float32(1.5)
        return v

    def far(rs):
        v = np.where(rs.randint(0, 2, C) > 0, np.float32(80), np.float32(-80)).astype(np.float32)
        v[0], v[C - 1] = np.float32(-80), np.float32(80)
        return v

    rec = [("ordinary", base), ("all_equal", lambda rs: np.full(C, 0.5, np.float32))]
    if C >= 2:
        rec += [("tie_first_last", tie((0, C - 1))), ("tie_diff_lane", tie((C - 2, C - 1))), ("near_at", near(NEAR)), ("near_inside", near(0.5 * NEAR)),
                ("near_outside", near(2.0 * NEAR)), ("one_finite", one_finite), ("far", far)]
    if C > 16:
        rec.append(("tie_same_lane", tie(tuple(C - 1 - 16 * k for k in range(min(3, (C - 1) // 16 + 1))))))
    return rec


@functools.lru_cache(maxsize=None)
def steered_heads(C, S):
    """exact binary fractions (but for the three near-tie deltas) placed to hit each regime of REGIMES.  Image 0: candidate n takes class recipe
    n mod R (R is odd, so every wavefront mixes recipes) and a random objectness edge; its box logits walk TXY x TWH, first on the
    cells of the first and last row and column.  Image 1: ordinary classes; the objectness of wavefront q puts (0, 1, 3, 4, 2)[q mod 5]
    candidates below logit(conf) - 0.01, one candidate of every seventh wavefront inside the 0.01 margin, a NaN in every eleventh."""
    rs = np.random.RandomState(11 + 1000 * C + S)
    N = num_pred(S)
    rec = _class_recipes(C)
    R = len(rec) if len(rec) % 2 else len(rec) + 1
    obj = _frac(rs, -3, 3, B, N)
    cls = np.empty((B, N, C), np.float32)
    box = _frac(rs, -2, 2, B, N, 4)
    obj_cycle = OBJ_EDGES + (1.0, 40.0, 2.5)
    for n in range(N):
        cls[0, n] = rec[n % R % len(rec)][1](rs)
        obj[0, n] = obj_cycle[rs.randint(len(obj_cycle))]
        cls[1, n] = rec[0][1](rs)
    # boxes: every (tx, tw) pair on the edge cells of every scale and anchor
    sc, gx, gy, an = geometry(S)
    w = np.asarray(maps(S))[sc]
    edge = (gx == 0) | (gy == 0) | (gx == w - 1) | (gy == w - 1)
    for s_ in range(3):
        for a_ in range(A):
            j = 0
            for n in np.nonzero(edge & (sc == s_) & (an == a_))[0]:
                for b in range(B):
                    box[b, n] = (TXY[j % 5], TXY[(j + 2) % 5], TWH[j % 6], TWH[(j + 3) % 6])
                    j += 1
    # image 1: skip mixes per wavefront of the flat index i = N + n
    counts = (0, 1, 3, 4, 2)
    for i in range(N, 2 * N):
        q, lane = i // 4, i % 4
        if (lane + q) % 4 < counts[q % 5]:
            obj[1, i - N] = BELOW_OBJ
        if q % 7 == 0 and lane == 0:
            obj[1, i - N] = MARGIN_OBJ
        if q % 11 == 3 and lane == 1:
            obj[1, i - N] = np.nan
    return pack_heads(obj, cls, box, S)


REGIMES = ("tie_same_lane", "tie_diff_lane", "tie_first_last", "all_equal", "near_at", "near_inside", "near_outside", "one_finite", "far",
           "obj_-59.875", "obj_-60", "obj_-60.125", "obj_-104", "obj_40", "obj_below_-60_not_skipped", "nan_with_three_ordinary",
           "skip_0", "skip_1", "skip_3", "skip_4", "margin", "general_wave", "fast_wave",
           "box_twh", "box_txy", "box_edges", "clamp_0", "clamp_1")


def regimes(r64, S, C, conf, groups):
    """name -> boolean mask [B * N] of the candidates in that regime, from the float64 reference r64 of raw heads; `groups` = wave_groups(...).
    A regime that needs more classes than C has is absent from the dict."""
    x, p = r64["x"].reshape(-1, C), r64["p"].reshape(-1, C)
    obj_raw = r64["obj_raw"].reshape(-1)
    cls = r64["cls"].reshape(-1, C)
    t = r64["t"].reshape(-1, 4)
    n_all = len(obj_raw)
    with np.errstate(all="ignore"):
        e = np.exp(x)
    top = x == 0
    ntop = top.sum(-1)
    lanes = np.arange(C) % 16
    lane_cnt = np.stack([(top & (lanes == l)).sum(-1) for l in range(16)], -1)           # tied classes per lane
    second = np.where(top, -np.inf, e).max(-1) if C > 1 else np.zeros(n_all)
    L = skip_logit(conf)
    below = obj_raw < L - 1e-4
    not_below = obj_raw > L + 1e-4
    ok = groups >= 0
    gid = np.where(ok, groups, groups.max() + 1)
    n_in = np.bincount(gid)[gid]
    n_below = np.bincount(gid, weights=below)[gid]
    n_nan = np.bincount(gid, weights=np.isnan(obj_raw))[gid]
    full = ok & (n_in == 4)
    window = ((e < 1.0 - 2e-7) & (e > 0.99999 + 2e-7)).any(-1) | (obj_raw < -60.0)       # what sends a wavefront down the general path, with a float margin
    clear = ~(((e < 1.0) & (e > 0.99999 - 2e-7)).any(-1)) & (obj_raw >= -60.0)
    n_window = np.bincount(gid, weights=window)[gid]                                     # (a skipping candidate of a wavefront that does not skip votes too)
    n_clear = np.bincount(gid, weights=clear | below)[gid]
    m = {}
    if C > 16:
        m["tie_same_lane"] = (lane_cnt >= 2).any(-1)
    if C >= 2:
        m["tie_diff_lane"] = ((lane_cnt >= 1).sum(-1) >= 2)
        m["tie_first_last"] = top[:, 0] & top[:, C - 1]
        m["near_at"] = np.abs(second - 0.99999) < 1e-7
        m["near_inside"] = (second > 0.99999 + 2e-6) & (second < 1.0 - 2e-6)
        m["near_outside"] = (second < 0.99999 - 2e-6) & (second > 0.9999)
        m["one_finite"] = np.isfinite(cls).sum(-1) == 1
        m["far"] = (np.abs(cls) >= 80).all(-1) & (cls.max(-1) - cls.min(-1) > 104)
    m["all_equal"] = ntop == C
    for v in OBJ_EDGES:
        m["obj_%g" % v] = obj_raw == v
    m["obj_below_-60_not_skipped"] = full & (obj_raw < -60.0) & (n_below < 4)
    m["nan_with_three_ordinary"] = full & np.isnan(obj_raw) & (n_nan == 1) & (n_below == 0)
    for k in (0, 1, 3, 4):
        m["skip_%d" % k] = full & (n_below == k) & (n_nan == 0)
    m["margin"] = (obj_raw > L + 1e-4) & (obj_raw < L + 0.01 - 1e-4)
    m["general_wave"] = full & (n_below < 4) & (n_window >= 1) & clear & ~below         # a fast-path candidate carried down the general path by a neighbour
    m["fast_wave"] = full & (n_clear == 4) & (n_below < 4) & (n_nan == 0)
    sc, gx, gy, an = geometry(S)
    w = np.asarray(maps(S))[sc]
    edge = np.tile((gx == 0) | (gy == 0) | (gx == w - 1) | (gy == w - 1), B)
    m["box_twh"] = edge & np.isin(t[:, 2], TWH) & np.isin(t[:, 3], TWH)
    m["box_txy"] = edge & np.isin(t[:, 0], TXY) & np.isin(t[:, 1], TXY)
    m["box_edges"] = m["box_twh"] & m["box_txy"]
    pre = r64["pre_clamp"].reshape(-1, 4)
    m["clamp_0"] = (pre < -1e-3).any(-1)
    m["clamp_1"] = (pre > 1 + 1e-3).any(-1)
    return m


def box_coverage(r64, S):
    """the steered box logits: every value of TWH and TXY on an edge cell of every (scale, anchor), and all four borders of every scale"""
    t = r64["t"].reshape(B, -1, 4)
    sc, gx, gy, an = geometry(S)
    w = np.asarray(maps(S))[sc]
    missing = []
    for s in range(3):
        for a in range(A):
            m = (sc == s) & (an == a) & ((gx == 0) | (gy == 0) | (gx == w - 1) | (gy == w - 1))
            for name, col, vals in (("tx", 0, TXY), ("ty", 1, TXY), ("tw", 2, TWH), ("th", 3, TWH)):
                for v in vals:
                    if not (t[:, m, col] == v).any():
                        missing.append((s, a, name, v))
        for name, m in (("col0", gx == 0), ("row0", gy == 0), ("colw", gx == w - 1), ("roww", gy == w - 1)):
            mm = m & (sc == s)
            if not np.isin(t[:, mm, 2], TWH).any():
                missing.append((s, name))
    return missing


# ---- the head tail's inputs -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_acts(S, seed=5):
    """the 96-channel activations layers .2 read: normal, scaled so that the objectness of the random-weight heads spans both sides of the threshold"""
    rs = np.random.RandomState(seed + S)
    return [(1.5 * rs.standard_normal((B, w, w, NECK))).astype(np.float32) for w in maps(S)]


@functools.lru_cache(maxsize=None)
def steered_acts(C, S):
    """activations in [0, 120] in steps of 1/8: through selection_layers raw = activation[n mod 96] + bias[n] exactly.  Channel values are
    drawn per pixel from a few levels (many exact ties between the classes that read them, equal activations under the 2**-17 / 2**-16 lower
    biases for the near ties), channels 0..2 (the objectness of the three anchors, and whatever class columns share them) from the
    objectness edges + 60, with runs of pixels far below the threshold so that wavefronts of 0, 1, 3 and 4 skipping candidates occur in
    every grouping."""
    rs = np.random.RandomState(13 + 1000 * C + S)
    out = []
    levels = np.asarray([56.0, 58.0, 60.0, 60.5, 61.0, 61.0, 61.0], np.float32)
    obj_levels = np.asarray([0.0, 0.125, 0.25, 50.0, 57.0, 58.0, 59.0, 60.0, 61.0, 62.0, 63.0, 100.0], np.float32)   # raw = level - 60.125
    for w in maps(S):
        x = levels[rs.randint(0, len(levels), size=(B, w, w, NECK))]
        some = rs.randint(0, 4, size=(B, w, w, 1)) == 0
        x = np.where(some, _frac(rs, 50, 62, B, w, w, NECK), x)
        x[..., :A] = obj_levels[rs.randint(0, len(obj_levels), size=(B, w, w, A))]
        # runs: the first rows of image 1 all far below, the last row all well above
        x[1, : max(1, w // 3), :, :A] = np.float32(10.0)
        x[1, -1, :, :A] = np.float32(62.0)
        out.append(np.ascontiguousarray(x, dtype=np.float32))
    return out


HEAD_TAIL_REGIMES = ("tie_same_lane", "tie_diff_lane", "near_inside", "near_outside", "obj_-59.875", "obj_-60", "obj_below_-60_not_skipped",
                     "skip_0", "skip_1", "skip_3", "skip_4", "general_wave", "fast_wave", "clamp_0", "clamp_1")
WAVE_REGIMES = ("obj_below_-60_not_skipped", "nan_with_three_ordinary", "skip_0", "skip_1", "skip_3", "skip_4", "general_wave", "fast_wave")


def folded_tail_layers(sd, hd):
    """layers .2, .3, .4 of head hd (1..3) of a state dict, BatchNorm folded in float32 the way fold_pack_kernel does (utils/fuse_conv_bn.py:17-21)"""
    out = []
    for conv, bn in head_keys(hd):
        w, b = sd[conv + ".weight"].astype(np.float32), sd[conv + ".bias"].astype(np.float32)
        if bn:
            f = sd[bn + ".weight"] / np.sqrt(sd[bn + ".running_var"] + np.float32(arch.BN_EPS))
            w, b = w * f.reshape(-1, 1, 1, 1), (b - sd[bn + ".running_mean"]) * f + sd[bn + ".bias"]
        out += [w.astype(np.float32), b.astype(np.float32)]
    return out


@functools.lru_cache(maxsize=None)
def random_state_dict(C):
    from yolo_nano_amd import weights
    return weights.make_state_dict("1.0x", C, A, seed=3)


@functools.lru_cache(maxsize=None)
def random_tail_heads(C, S):
    """the raw heads of the random head-tail case, evaluated in float32 on the CPU (the near-tie count; the GPU test takes the device's own)"""
    sd = random_state_dict(C)
    return [tail_ref(x, *folded_tail_layers(sd, hd + 1), dtype=np.float32) for hd, x in enumerate(random_acts(S))]


def score_bar(r64, r32):
    """what f64_bar.bar allows an element of all_class: 4 e32 + 4 ulp"""
    a64, a32 = np.nan_to_num(r64["all_class"], nan=0.0), np.nan_to_num(r32["all_class"].astype(np.float64), nan=0.0)
    e32 = float(np.abs(a32 - a64).max())
    ulp = float(np.spacing(np.float32(np.abs(a64).max())))
    return 4 * e32 + 4 * ulp


def near_tie_mask(r64, r32):
    """[B, N] the candidates whose two largest float64 class scores lie within twice score_bar of each other (each may move by one bar): the class
    check excuses them.  Bit-equal maxima are no near-ties: there the class must be the lowest tied index."""
    a = r64["all_class"]
    if a.shape[-1] < 2:
        return np.zeros(a.shape[:2], bool)
    top = np.sort(np.nan_to_num(a, nan=0.0), -1)
    gap = top[..., -1] - top[..., -2]
    tied = (r64["x"] == 0).sum(-1) >= 2
    return (gap <= 2 * score_bar(r64, r32)) & ~tied & ~np.isnan(r64["obj_raw"])


def tail_round_mixes(r64, S, conf):
    """head_tail_block runs pass A on three candidates per 16-lane group and round (wavefront w of a tile takes the tile's groups q with q mod 4 = w,
    three per round: q // 12 is the round) and skips the class statistics only when all three of a round skip: the number of rounds, over the whole
    batch, in which some of the three wavefront-quartets skip and some do not"""
    ids = wave_groups("head_tail", S)
    below = r64["obj_raw"].reshape(-1) < skip_logit(conf) - 1e-4
    ok = ids >= 0
    rel = ids[ok] % (1 << 20)
    key = (ids[ok] >> 20) * (1 << 20) + (rel // 24) * 8 + (rel % 24 % 4) * 2 + (rel % 24) // 12      # (scale, tile, wavefront, round)
    quartet = ids[ok]
    uq, inv = np.unique(quartet, return_inverse=True)
    all_below = np.bincount(inv, weights=below[ok]) == 4
    kq = np.zeros(len(uq), np.int64); kq[inv] = key
    uk, kinv = np.unique(kq, return_inverse=True)
    n = np.bincount(kinv)
    nb = np.bincount(kinv, weights=all_below)
    return int(((nb > 0) & (nb < n)).sum())
