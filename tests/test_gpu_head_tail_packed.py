"""head_tail_group_kernel<5> with its tiles packed from the run list (csrc/yn_head_tile_map.h): a workgroup is eight consecutive runs of four
x-consecutive pixels - an 8 x 4 block where the eight are aligned, other shapes at band ends, image ends and the level's end, tiles that straddle
bands and images, and a last tile that is part empty.  Which candidates share a wavefront of the decode passes follows from that order, and nothing
the kernel writes may depend on it.

On an 80-class handle, for maps whose levels are 12/6/3, 20/10/5, 28/14/7 and 52/26/13 wide and one rectangular window (20 x 28, 10 x 14, 5 x 7), with
1, 2 or 3 images: all B x N boxes, scores and classes of yn_op_head_tail are bit-identical to the same call with yn_tail_fuse off and to
yn_op_decode_cand on raw heads computed layer by layer from the same activations.  Inputs: random activations under random weights, and the steered
selection weights of tests/decode_cases.py (raw = activation + bias exactly: ties, near ties inside and outside the general path's window, objectness
edges) with runs of far-below objectness laid out in the PACKED order, so that wavefront quartets skip, rounds of three quartets skip in part and in
whole, and fast and general wavefronts occur - counted here with the packed grouping restated in Python."""
import numpy as np
import pytest
import torch

import decode_cases as dc
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu

C = 80
A = dc.A
BMAX = 3
# name: (H, W, B): image sizes; the levels are H / 8, H / 16, H / 32 high
CASES = {"s96-b1": (96, 96, 1), "s96-b3": (96, 96, 3), "s160-b1": (160, 160, 1), "s160-b3": (160, 160, 3), "s224-b1": (224, 224, 1),
         "s224-b3": (224, 224, 3), "s416-b2": (416, 416, 2), "r160x224-b3": (160, 224, 3), "r224x96-b1": (224, 96, 1)}


def _levels(H, W):
    return [(H // s, W // s) for s in arch.STRIDES]


# ---- the packed order, restated: run list -> tiles -> tile rows -> candidates -> wavefront quartets and rounds -----------------------------------
def packed_slots(B, h, w):
    """int array [tiles, 32, 4]: (image, y, x, inside) of every tile row of a level, tile row = slot * 4 + pixel of the run"""
    runs = []
    for b in range(B):
        for y0 in range(0, h, 4):
            for col in range((w + 3) // 4):
                for y in range(y0, min(y0 + 4, h)):
                    runs.append((b, y, 4 * col))
    runs += [(0, 0, -8)] * (-len(runs) % 8)                    # the last tile's empty slots
    r = np.asarray(runs, np.int64)
    x = r[:, None, 2] + np.arange(4)
    inside = (x >= 0) & (x < w)
    rows = np.stack([np.broadcast_to(r[:, None, 0], x.shape), np.broadcast_to(r[:, None, 1], x.shape), np.where(inside, x, 0), inside.astype(np.int64)], -1)
    return rows.reshape(-1, 32, 4)


def packed_quartets(per_cand, B, h, w, fill):
    """per_cand [B, h, w, A] -> [tiles, round 2, u 3, wavefront 4, 4]: pass A takes candidate c = row * A + anchor of a tile in quartets q = c // 4,
    wavefront q % 4, three quartets (u) per round; rows outside the map hold `fill`.  Also [tiles] whether all 32 rows of the tile are inside."""
    s = packed_slots(B, h, w)
    v = np.where(s[..., 3:4] > 0, per_cand[s[..., 0], s[..., 1], s[..., 2]], fill)             # [tiles, 32, A]
    q = v.reshape(len(s), 24, 4)                                                                # quartet q
    return q.reshape(len(s), 2, 3, 4, 4), s[..., 3].all(-1)


def _steered_acts(B, H, W):
    """dc.steered_acts for any batch and map: levels of exact binary fractions with many ties, objectness from the edge levels - and, in the packed
    order, slots 0 1 4 5 of every third tile and slots 0 - 3 of the tiles after them far below the threshold"""
    rs = np.random.RandomState(17 + H + 7 * W + 1000 * B)
    levels = np.asarray([56.0, 58.0, 60.0, 60.5, 61.0, 61.0, 61.0], np.float32)
    obj_levels = np.asarray([0.0, 0.125, 0.25, 50.0, 57.0, 58.0, 59.0, 60.0, 61.0, 62.0, 63.0, 100.0], np.float32)
    out = []
    for h, w in _levels(H, W):
        x = levels[rs.randint(0, len(levels), size=(B, h, w, dc.NECK))]
        some = rs.randint(0, 4, size=(B, h, w, 1)) == 0
        x = np.where(some, dc._frac(rs, 50, 62, B, h, w, dc.NECK), x)
        x[..., :A] = obj_levels[rs.randint(0, len(obj_levels), size=(B, h, w, A))]
        s = packed_slots(B, h, w)
        tile, slot = np.arange(len(s))[:, None] % 3, np.arange(32)[None, :] // 4
        low = (s[..., 3] > 0) & (((tile == 0) & np.isin(slot, (0, 1, 4, 5))) | ((tile == 1) & (slot < 4)))
        x[s[low][:, 0], s[low][:, 1], s[low][:, 2], :A] = np.float32(10.0)
        out.append(np.ascontiguousarray(x, dtype=np.float32))
    return out


def _random_acts(B, H, W):
    rs = np.random.RandomState(5 + H + 7 * W + 1000 * B)
    return [(1.5 * rs.standard_normal((B, h, w, dc.NECK))).astype(np.float32) for h, w in _levels(H, W)]


# ---- the device -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_handle():
    from yolo_nano_amd import capi
    cache = {}

    def get(kind):
        if kind not in cache:
            sd, conf = dc.random_state_dict(C), dc.CONF_RANDOM
            if kind == "steered":
                sd, conf = dc.steered_state_dict(sd, C), dc.CONF_STEERED
            h = capi.Handle(96, C, arch.MULTI_ANCHOR_SIZE, conf_thresh=conf, max_batch=BMAX)
            h.autotune(False)
            h.load_state_dict(sd)
            h.fold_bn()
            cache[kind] = (h, conf)
        return cache[kind]
    yield get
    for h, _ in cache.values():
        h.close()


def _ran(h, fn):
    h.profile_enable(True)
    try:
        y = fn()
        torch.cuda.synchronize()
        names = [r[1] for r in h.profile_records()]
    finally:
        h.profile_enable(False)
    return [t.cpu().numpy() for t in y], names


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    ia, ib = a.view(np.int32), b.view(np.int32)
    if not np.array_equal(ia, ib):
        bad = np.argwhere(ia != ib)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r against %r" % (what, len(bad), a.size, i, a[i], b[i]))


def _steering_reached(tag, raw_np, B, H, W, conf):
    """what the steered data must make the packed wavefronts do, from the device's raw heads (exact: activation + bias)"""
    L = dc.skip_logit(conf)
    seen = dict(part=0, whole=0, none=0, q1=0, q3=0, fast=0, general=0, tie=0, straddle=0)
    for raw, (h, w) in zip(raw_np, _levels(H, W)):
        r = raw.astype(np.float64)
        obj = r[..., :A]
        cls = r[..., A:A * (1 + C)].reshape(B, h, w, A, C)
        x = cls - cls.max(-1, keepdims=True)
        e = np.exp(x)
        window = (((e < 1.0 - 2e-7) & (e > 0.99999 + 2e-7)).any(-1) | (obj < -60.0)).astype(np.float64)
        seen["tie"] += int(((x == 0).sum(-1) >= 2).sum())
        below, full = packed_quartets((obj < L - 1e-4).astype(np.float64), B, h, w, 1.0)
        win, _ = packed_quartets(window, B, h, w, 0.0)
        nb = below.sum(-1)                                    # [tiles, round, u, wavefront]: candidates of the quartet that skip
        allb = (nb == 4)[full]
        k = allb.sum(2)                                      # [tiles, round, wavefront]: quartets of the round's three that skip whole
        seen["part"] += int(((k > 0) & (k < 3)).sum()); seen["whole"] += int((k == 3).sum()); seen["none"] += int((k == 0).sum())
        seen["q1"] += int((nb[full] == 1).sum()); seen["q3"] += int((nb[full] == 3).sum())
        live = nb[full] < 4
        seen["general"] += int((live & (win.sum(-1)[full] > 0)).sum()); seen["fast"] += int((live & (win.sum(-1)[full] == 0)).sum())
        s = packed_slots(B, h, w)
        inside = s[..., 3] > 0
        img_lo, img_hi = np.where(inside, s[..., 0], B).min(-1), np.where(inside, s[..., 0], -1).max(-1)
        seen["straddle"] += int((img_hi > img_lo).sum())
    want = [k for k in seen if k != "straddle" or B > 1]
    assert all(seen[k] > 0 for k in want), (tag, seen)


@pytest.mark.parametrize("kind", ["random", "steered"])
@pytest.mark.parametrize("case", list(CASES))
def test_packed_head_tail_is_bit_identical(tail_handle, case, kind):
    H, W, B = CASES[case]
    h, conf = tail_handle(kind)
    if H == W:
        h.set_grid(H)
    else:
        h.set_grid_rect(H, W)
    lv = _levels(H, W)
    assert h.N == sum(A * a * b for a, b in lv)
    # the shapes are here for their tiles: a part-empty last tile on some level, tiles that straddle images where B > 1
    runs = [B * a * ((b + 3) // 4) for a, b in lv]
    assert any(r % 8 for r in runs), runs
    acts = _random_acts(B, H, W) if kind == "random" else _steered_acts(B, H, W)
    xs = [torch.from_numpy(x).cuda() for x in acts]
    tag = "%s %s" % (case, kind)
    shapes = ((dc.NECK, 1, 3, 3), (dc.NECK, dc.NECK, 1, 1), (A * (5 + C), dc.NECK, 1, 1))
    raws = []
    for hd, x in enumerate(xs):
        lay = [h.get_folded(conv, shp) for (conv, _), shp in zip(dc.head_keys(hd + 1), shapes)]
        (wd, bd), (wp, bp), (wf, bf) = [(torch.from_numpy(w_).cuda(), torch.from_numpy(b_).cuda()) for w_, b_ in lay]
        raws.append(h.op_pwconv(h.op_pwconv(h.op_dwconv3x3(x, wd, bd, 1, 2), wp, bp, 2), wf, bf, 0))
    (rb, rs, rcl), names = _ran(h, lambda: h.op_decode_cand(raws, conf))
    assert names == [dc.decode_kernel(C, False)], names
    try:
        h.tail_fuse(False)
        (ub, us, ucl), names = _ran(h, lambda: h.op_head_tail(xs))
        assert not any(n.startswith("head_tail") for n in names), names
        h.tail_fuse(True)
        (boxes, scores, cls), names = _ran(h, lambda: h.op_head_tail(xs))
        assert [n for n in names if dc.is_decode_kernel(n)] == ["head_tail_group_kernel<5>"], names
    finally:
        h.tail_fuse(True)
    assert boxes.shape == (B, h.N, 4) and scores.shape == (B, h.N) and cls.shape == (B, h.N)
    for what, ref in (("yn_tail_fuse off", (ub, us, ucl)), ("op_decode_cand on the raw heads", (rb, rs, rcl))):
        _bits_equal(boxes, ref[0], "%s boxes against %s" % (tag, what))
        _bits_equal(scores, ref[1], "%s scores against %s" % (tag, what))
        assert np.array_equal(cls, ref[2]), (tag, what)
    if kind == "steered":
        assert (cls >= 0).any() and (cls < 0).any(), tag      # both sides of the threshold
        _steering_reached(tag, [r.cpu().numpy() for r in raws], B, H, W, conf)
