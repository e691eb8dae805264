"""What tests/test_gpu_rect.py and tests/test_rect_cases_cpu.py share: rectangular grids (yn_set_grid_rect) restated in Python.

The convention.  A rectangular grid is a WINDOW OF A LETTERBOXED SQUARE: the canvas is H x W (multiples of 32), its top-left pixel sits at
(left, top) of a side x side square.  Raw heads are NHWC [B, H/st, W/st, A (5 + C)]; candidate n of an image = off[scale] + cell * A + anchor,
cell = gy * (W/st) + gx.  A box is normalised to the square, not to the canvas: with p the canvas pixel coordinate as decode_cases.decode_ref
computes it, v = (p + off) / side, clipped to [0, 1], off = left for x1 / x2 and top for y1 / y2.  rect_ref is decode_cases.decode_ref with that
one change; on the whole square (H = W = side, left = top = 0) it IS decode_ref (tests/test_rect_cases_cpu.py).
"""
import functools

import numpy as np

import decode_cases as dc
from yolo_nano_amd import arch

A, B = dc.A, dc.B


def maps(H, W):
    return [(H // s, W // s) for s in arch.STRIDES]


def num_pred(H, W):
    return sum(A * h * w for h, w in maps(H, W))


def default_window(H, W):
    """yn_set_grid_rect's side = 0: the smallest square, the window centred -> (side, left, top)"""
    side = max(H, W)
    return side, (side - W) // 2, (side - H) // 2


@functools.lru_cache(maxsize=None)
def geometry(H, W):
    """per candidate of one image: scale, gx, gy, anchor (int arrays [N])"""
    sc, gx, gy, an = [], [], [], []
    for s, (h, w) in enumerate(maps(H, W)):
        cell = np.repeat(np.arange(h * w), A)
        sc.append(np.full(h * w * A, s)); gx.append(cell % w); gy.append(cell // w); an.append(np.tile(np.arange(A), h * w))
    return tuple(np.concatenate(v) for v in (sc, gx, gy, an))


def unpack_heads(heads, C):
    """three raw heads [B, h, w, A (5 + C)] -> obj [B, N], cls [B, N, C], box [B, N, 4] in candidate order"""
    o, c, t = [], [], []
    for hd in heads:
        Bn, h, w = hd.shape[:3]
        r = hd.reshape(Bn, h * w, A * (5 + C))
        o.append(r[:, :, :A].reshape(Bn, h * w * A))
        c.append(r[:, :, A:A * (1 + C)].reshape(Bn, h * w * A, C))
        t.append(r[:, :, A * (1 + C):].reshape(Bn, h * w * A, 4))
    return np.concatenate(o, 1), np.concatenate(c, 1), np.concatenate(t, 1)


def pack_heads(obj, cls, box, H, W):
    """the inverse of unpack_heads"""
    Bn, N, C = cls.shape
    heads, off = [], 0
    for h, w in maps(H, W):
        n = h * w * A
        r = np.concatenate([obj[:, off:off + n].reshape(Bn, h * w, A), cls[:, off:off + n].reshape(Bn, h * w, A * C),
                            box[:, off:off + n].reshape(Bn, h * w, A * 4)], -1)
        heads.append(np.ascontiguousarray(r.reshape(Bn, h, w, A * (5 + C)), dtype=np.float32))
        off += n
    return heads


def rect_ref(heads, H, W, side, left, top, C, dtype=np.float64):
    """decode_cases.decode_ref for the H x W window at (left, top) of a side x side square: the same dict, every operation in `dtype`"""
    f = dtype
    obj_raw, cls, t = (v.astype(f) for v in unpack_heads(heads, C))
    sc, gx, gy, an = geometry(H, W)
    assert obj_raw.shape[1] == len(sc), (obj_raw.shape, len(sc))
    with np.errstate(all="ignore"):
        x = cls - cls.max(-1, keepdims=True)
        e = np.exp(x)
        p = e / e.sum(-1, keepdims=True)
        obj = f(1) / (f(1) + np.exp(-obj_raw))
        all_class = p * obj[..., None]
        stride = np.asarray(arch.STRIDES, dtype=f)[sc]
        anc = dc.ANCHORS.astype(f)[sc, an]                                               # [N, 2]
        cxy = (f(1) / (f(1) + np.exp(-t[..., :2])) + np.stack([gx, gy], -1).astype(f)) * stride[:, None]
        wh = np.exp(t[..., 2:]) * anc
        pix = np.concatenate([cxy - wh / f(2), cxy + wh / f(2)], -1)                     # canvas pixels: what yn_decode_boxes returns
        box = (pix + np.asarray([left, top, left, top], dtype=f)) / f(side)              # one normaliser for both axes
        pre = box.copy()
        box = np.clip(box, f(0), f(1))
    key = np.where(np.isnan(all_class), -np.inf, all_class)
    best = key.argmax(-1)
    score = np.take_along_axis(all_class, best[..., None], -1)[..., 0]
    return dict(all_bbox=box, pre_clamp=pre, pixels=pix, all_class=all_class, best=best, score=score, x=x, p=p, obj=obj, obj_raw=obj_raw, cls=cls, t=t)


def window_of_square(heads, S, H, W, left, top):
    """the raw heads of the cells an H x W window at (left, top) - whole cells of every scale: multiples of 32 - cuts out of S x S heads"""
    assert left % 32 == 0 and top % 32 == 0 and left + W <= S and top + H <= S
    return [np.ascontiguousarray(hd[:, top // s:(top + H) // s, left // s:(left + W) // s]) for hd, s in zip(heads, arch.STRIDES)]


def window_candidates(S, H, W, left, top):
    """[N_window] the square grid's candidate index of every candidate of the window, in the window's candidate order"""
    idx, off = [], 0
    for s in arch.STRIDES:
        w = S // s
        gy, gx = np.meshgrid(np.arange(top // s, (top + H) // s), np.arange(left // s, (left + W) // s), indexing="ij")
        cell = (gy * w + gx).reshape(-1)
        idx.append(off + (cell[:, None] * A + np.arange(A)[None]).reshape(-1))
        off += w * w * A
    return np.concatenate(idx)


# =====================================================================================================================================
# data: decode_cases.random_heads / steered_heads on an H x W canvas
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def random_heads(C, H, W, seed=7):
    """as decode_cases.random_heads: objectness ~ N(0, 2) on both sides of logit(CONF_RANDOM), class logits ~ N(0, 2), box logits ~ N(0, 1)"""
    rs = np.random.RandomState(seed + 1000 * C + 31 * H + W)
    N = num_pred(H, W)
    obj = (2.0 * rs.standard_normal((B, N))).astype(np.float32)
    cls = (2.0 * rs.standard_normal((B, N, C))).astype(np.float32)
    box = rs.standard_normal((B, N, 4)).astype(np.float32)
    return pack_heads(obj, cls, box, H, W)


@functools.lru_cache(maxsize=None)
def steered_heads(C, H, W):
    """as decode_cases.steered_heads (its class recipes, objectness edges and box logit tables): image 0 walks the recipes and puts every (tx, tw)
    pair on the border cells of every scale and anchor - the cells where a window's offset meets the clamp; image 1 mixes skipping and live
    candidates per wavefront of the flat index, with a candidate inside the 0.01 margin and a NaN objectness now and then"""
    rs = np.random.RandomState(11 + 1000 * C + 31 * H + W)
    N = num_pred(H, W)
    rec = dc._class_recipes(C)
    R = len(rec) if len(rec) % 2 else len(rec) + 1
    obj = dc._frac(rs, -3, 3, B, N)
    cls = np.empty((B, N, C), np.float32)
    box = dc._frac(rs, -2, 2, B, N, 4)
    obj_cycle = dc.OBJ_EDGES + (1.0, 40.0, 2.5)
    for n in range(N):
        cls[0, n] = rec[n % R % len(rec)][1](rs)
        obj[0, n] = obj_cycle[rs.randint(len(obj_cycle))]
        cls[1, n] = rec[0][1](rs)
    sc, gx, gy, an = geometry(H, W)
    hh = np.asarray([m[0] for m in maps(H, W)])[sc]
    ww = np.asarray([m[1] for m in maps(H, W)])[sc]
    edge = (gx == 0) | (gy == 0) | (gx == ww - 1) | (gy == hh - 1)
    for s_ in range(3):
        for a_ in range(A):
            j = 0
            for n in np.nonzero(edge & (sc == s_) & (an == a_))[0]:
                for b in range(B):
                    box[b, n] = (dc.TXY[j % 5], dc.TXY[(j + 2) % 5], dc.TWH[j % 6], dc.TWH[(j + 3) % 6])
                    j += 1
    counts = (0, 1, 3, 4, 2)
    for i in range(N, 2 * N):
        q, lane = i // 4, i % 4
        if (lane + q) % 4 < counts[q % 5]:
            obj[1, i - N] = dc.BELOW_OBJ
        if q % 7 == 0 and lane == 0:
            obj[1, i - N] = dc.MARGIN_OBJ
        if q % 11 == 3 and lane == 1:
            obj[1, i - N] = np.nan
    return pack_heads(obj, cls, box, H, W)


# =====================================================================================================================================
# case tables of tests/test_gpu_rect.py
# =====================================================================================================================================
NET_BACKBONES = (("1.0x", 20), ("0.5x", 80))
# a one-cell-high and a one-cell-wide stride-32 map, tiles that end mid-row and mid-image, 0.5x stage 2 at width 76 > BM; both orientations
NET_SHAPES = ((32, 96, 3), (96, 32, 3), (64, 160, 2), (160, 64, 2), (128, 224, 3), (64, 608, 3), (608, 64, 1))
FORM_SHAPES = ((128, 224, 3), (64, 608, 3))
DECODE_C = (20, 80)
DECODE_GRIDS = ((32, 96), (96, 32), (64, 160))


def decode_windows(H, W):
    """name -> (side, left, top): the default window, one off the cell raster inside a 192 square, and the one that touches the square's far
    corner (the whole-square window exists for H = W only: WHOLE_SQUARE)"""
    side, left, top = default_window(H, W)
    return {"default": (side, left, top), "s192": (192, 13, 71), "corner": (192, 192 - W, 192 - H)}


WHOLE_SQUARE = 96                                           # yn_set_grid_rect(96, 96, 96, 0, 0) is yn_set_grid(96)

FRAMES_16_9 = ((90, 160), (72, 128), (45, 80))             # (h0, w0): at side 160 all three letterbox to 160 x 90 at (0, 35)


def make_input(batch, H, W, seed=0):
    """weights.make_input on an H x W canvas: x ~ N(0, 1) float32 [B, 3, H, W] from the same generator"""
    rs = np.random.RandomState(1000003 * seed + 17)
    return rs.standard_normal((batch, 3, H, W)).astype(np.float32)


# ---- the head tail's inputs (decode_cases.random_acts / steered_acts on an H x W canvas) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_acts(H, W, seed=5):
    rs = np.random.RandomState(seed + 31 * H + W)
    return [(1.5 * rs.standard_normal((B, h, w, dc.NECK))).astype(np.float32) for h, w in maps(H, W)]


@functools.lru_cache(maxsize=None)
def steered_acts(C, H, W):
    rs = np.random.RandomState(13 + 1000 * C + 31 * H + W)
    out = []
    levels = np.asarray([56.0, 58.0, 60.0, 60.5, 61.0, 61.0, 61.0], np.float32)
    obj_levels = np.asarray([0.0, 0.125, 0.25, 50.0, 57.0, 58.0, 59.0, 60.0, 61.0, 62.0, 63.0, 100.0], np.float32)   # raw = level - 60.125
    for h, w in maps(H, W):
        x = levels[rs.randint(0, len(levels), size=(B, h, w, dc.NECK))]
        some = rs.randint(0, 4, size=(B, h, w, 1)) == 0
        x = np.where(some, dc._frac(rs, 50, 62, B, h, w, dc.NECK), x)
        x[..., :A] = obj_levels[rs.randint(0, len(obj_levels), size=(B, h, w, A))]
        x[1, : max(1, h // 3), :, :A] = np.float32(10.0)     # the first rows of image 1 far below the threshold, the last row well above
        x[1, -1, :, :A] = np.float32(62.0)
        out.append(np.ascontiguousarray(x, dtype=np.float32))
    return out


def front_end(C, H, W, tail, fuse, group):
    """decode_cases.front_end with the size rule of head_fuse_all on an H x W canvas: B (H/8)(W/8) rows of the stride-8 head"""
    fuse_all = fuse != 0 and dc.head_decode_supported(C)
    tail_possible = fuse_all and tail and group and C > 32 and 128 < dc.npad(C) <= 256
    if fuse != 2 and B * (H // 8) * (W // 8) < 8192 and not tail_possible:
        fuse_all = False
    if not fuse_all:
        return [dc.decode_kernel(C, False)]
    if group and tail and dc.head_tail_ok(C):
        return ["head_tail_group_kernel<5>"]
    if group:
        return ["head_decode_group_kernel<%d,%d>" % dc.head_decode_variant(C)]
    return ["head_decode_kernel<%d,%d>" % dc.head_decode_variant(C)] * 3


# the stage_pipe_kernel forms the FORM_SHAPES must take (stage_pipe_form, csrc/yn_stage_form.h: W + 1 <= BM, LDS of two workgroups per CU or one):
# (backbone, H, W) -> kernel name prefixes.  1.0x stage 3 (bf 116: 32-row tiles of four wavefronts, 64 of eight): W = 14 fits the first, W = 38
# needs the second (as 608 x 608 does); 0.5x stage 2 (bf 24: 64-row tiles of four wavefronts, 128 of eight): W = 28 fits the first, W = 76 > 64
# only the second - the width rule; 0.5x stage 3 (bf 48): 64-row tiles hold W = 14 and W = 38.
STAGE_FORMS = {
    ("1.0x", 128, 224): ("stage_pipe_kernel<116,4,",),
    ("1.0x", 64, 608): ("stage_pipe_kernel<116,8,",),
    ("0.5x", 128, 224): ("stage_pipe_kernel<24,4,", "stage_pipe_kernel<48,4,"),
    ("0.5x", 64, 608): ("stage_pipe_kernel<24,8,", "stage_pipe_kernel<48,4,"),
}
