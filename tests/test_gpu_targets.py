"""GPU parity of the training label assigner (tools.multi_gt_creator, tools.py:97-216):
yn_make_targets against the reference's own outputs (tests/golden/targets.npz) and against the oracle at BASELINE
configs[2]'s size.  Everything is integer / exactly-rounded float64 arithmetic and must match BIT-EXACTLY, except
tw/th = log(box/anchor): the device's float64 log may differ from libm's in the last bit, which can move the float32
result by one ulp — those two fields get 1 float32 ulp."""
import numpy as np
import pytest
import torch

from oracle import targets as otg
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu


def _check(got, ref):
    assert got.shape == ref.shape
    for f in (0, 1, 2, 3, 6, 7, 8, 9, 10):
        np.testing.assert_array_equal(got[..., f], ref[..., f], err_msg="field %d" % f)
    for f in (4, 5):
        ulp = np.spacing(np.abs(ref[..., f]).astype(np.float32))
        assert (np.abs(got[..., f] - ref[..., f]) <= ulp).all(), "field %d" % f


def test_targets_match_reference_fixture(golden):
    from yolo_nano_amd import capi
    g = golden("targets.npz")
    for ci in range(4):
        S, C, B, coco = (int(v) for v in g["case%d_meta" % ci])
        anchors = arch.MULTI_ANCHOR_SIZE_COCO if coco else arch.MULTI_ANCHOR_SIZE
        labels = otg.labels_from_flat(g["case%d_labels" % ci], B)
        h = capi.Handle(S, C, anchors, "1.0x", max_batch=B)
        got = h.make_targets(labels, anchors).cpu().numpy()
        _check(got, g["case%d_target" % ci])
        h.close()


def test_targets_config3_size_vs_oracle_and_shim():
    """608x608, 32 images x 40 objects (+ an empty image): vs the oracle; the module-level shim with the reference's
    signature gives the same tensor; a reused output buffer is fully overwritten."""
    import yolo_nano_amd
    from yolo_nano_amd import capi
    S, C, B = 608, 80, 32
    rs = np.random.RandomState(9)
    labels = []
    for b in range(B):
        n = 0 if b == 5 else 40
        cxy = rs.uniform(0.05, 0.95, (n, 2))
        wh = np.exp(rs.uniform(np.log(0.004), np.log(0.9), (n, 2)))
        box = np.clip(np.concatenate([cxy - wh / 2, cxy + wh / 2], 1), 0, 1).astype(np.float32).astype(np.float64)
        labels.append(np.concatenate([box, rs.randint(0, C, (n, 1)).astype(np.float64)], 1).tolist())
    ref = otg.multi_gt_creator(S, list(arch.STRIDES), labels, arch.MULTI_ANCHOR_SIZE_COCO)
    h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE_COCO, "1.0x", max_batch=B)
    out = torch.full((B, h.N, 11), 7.0, dtype=torch.float32, device="cuda")
    got = h.make_targets(labels, arch.MULTI_ANCHOR_SIZE_COCO, out=out)
    assert got.data_ptr() == out.data_ptr()
    _check(got.cpu().numpy(), ref)
    t2 = yolo_nano_amd.multi_gt_creator(S, [8, 16, 32], labels, arch.MULTI_ANCHOR_SIZE_COCO)
    assert t2.is_cuda and torch.equal(t2, got)
    # the assigned targets drive a training step end to end
    losses = None
    from yolo_nano_amd import weights
    h.load_state_dict(weights.make_state_dict("1.0x", C))
    h.train_bind()
    x = torch.as_tensor(weights.make_input(2, S, seed=3)).cuda()
    losses = h.train_step(x, got[:2].contiguous(), lr=1e-4)
    assert torch.isfinite(losses).all()
    h.close()


# ---- more than 64 objects per image: targets_kernel takes an image's objects 64 at a time and replays each chunk's records before it evaluates
#      the next one (the LDS records are reused, one barrier pair per chunk) ----
def _shape_for(anchors, S, best, also_above=None):
    """(w, h) in pixels of a box whose best anchor is `best` and, when asked, whose IoU with `also_above` exceeds the ignore threshold too."""
    aw = [(float(a[0]), float(a[1])) for a in anchors]
    for bw in range(4, int(0.9 * S), 2):
        for bh in range(4, int(0.9 * S), 2):
            iou = otg.shape_iou(aw, float(bw), float(bh))
            if int(np.argmax(iou)) != best:
                continue
            if also_above is None or (also_above != best and iou[also_above] > otg.IGNORE_THRESH):
                return float(bw), float(bh)
    return None


def _chunk_labels(S, C, anchors, rs):
    """Images of 0, 64, 65, 128 and 130 objects whose overwrite order crosses a chunk boundary; -> labels, [(image, slot, expected obj, expected cls)]."""
    pair = None
    for k in range(9):
        for k2 in range(9):
            if k2 != k and pair is None:
                p, q = _shape_for(anchors, S, k), _shape_for(anchors, S, k2, also_above=k)
                if p and q:
                    pair = (k, p, q)
    assert pair is not None, "no box shape is positive on one anchor and above the ignore threshold on another at this size"
    k, pos_wh, ign_wh = pair
    si, ab = k // 3, k % 3
    s, ws = arch.STRIDES[si], S // arch.STRIDES[si]
    off = sum(3 * (S // t) ** 2 for t in arch.STRIDES[:si])

    def box(cx, cy, wh, cls):                               # centre in pixels; exact in float32 so that the float64 labels are what a loader yields
        v = np.array([(cx - wh[0] / 2) / S, (cy - wh[1] / 2) / S, (cx + wh[0] / 2) / S, (cy + wh[1] / 2) / S], np.float32).astype(np.float64)
        assert 0.0 <= v.min() and v.max() <= 1.0
        return v.tolist() + [float(cls)]

    def slot(cx, cy):
        return off + (int(cy / s) * ws + int(cx / s)) * 3 + ab

    labels, expect = [], []
    for b, n in enumerate((0, 64, 65, 128, 130)):
        cxy = rs.uniform(0.05, 0.95, (n, 2))
        wh = np.exp(rs.uniform(np.log(0.02), np.log(0.9), (n, 2)))
        bx = np.clip(np.concatenate([cxy - wh / 2, cxy + wh / 2], 1), 0, 1).astype(np.float32).astype(np.float64)
        ls = np.concatenate([bx, rs.randint(0, C, (n, 1)).astype(np.float64)], 1).tolist()
        c = S / 2 + s / 2                                     # the middle of a cell at every stride
        if n == 65:        # objects 63 and 64: positives of one (cell, anchor) slot on either side of the boundary, the later one stays
            ls[63], ls[64] = box(c - 1, c, pos_wh, 3), box(c + 1, c - 1, pos_wh, 4)
            expect.append((b, slot(c, c), 1.0, 4.0))
        if n == 128:       # a positive of the first chunk (object 10), then an ignore write from the second (object 127) on its slot
            ls[10], ls[127] = box(c, c, pos_wh, 5), box(c, c, ign_wh, 6)
            expect.append((b, slot(c, c), -1.0, 5.0))
        if n == 130:       # an ignore write of the first chunk (object 5), then a positive of the last chunk (object 129) on its slot
            ls[5], ls[129] = box(c, c, ign_wh, 7), box(c, c, pos_wh, 8)
            expect.append((b, slot(c, c), 1.0, 8.0))
        if n >= 65:        # nothing else may touch the engineered slot: move the other objects whose centre lies in that cell (at any stride it is inside the top-level cell)
            keep = {63, 64} if n == 65 else ({10, 127} if n == 128 else {5, 129})
            for i, l in enumerate(ls):
                if i not in keep and abs((l[0] + l[2]) / 2 * S - c) < 32 and abs((l[1] + l[3]) / 2 * S - c) < 32:
                    ls[i] = box(S * 0.15, S * 0.15, (0.2 * S, 0.2 * S), 0)
        labels.append(ls)
    return labels, expect


@pytest.mark.parametrize("S", [128, 416])
@pytest.mark.parametrize("coco", [0, 1])
def test_targets_beyond_one_chunk_of_objects(S, coco):
    """0 / 64 / 65 / 128 / 130 objects per image against the oracle, field by field as _check: the loop over 64-object chunks runs zero, one, two and
    three times, with a full and a ragged last chunk.  Three slots are engineered (anchor-shaped boxes on one centre, as gen_golden.gen_targets) so
    that the overwrite order crosses a chunk boundary; the oracle's own output is checked for those collisions first."""
    from yolo_nano_amd import capi
    anchors, C = (arch.MULTI_ANCHOR_SIZE_COCO, 80) if coco else (arch.MULTI_ANCHOR_SIZE, 20)
    labels, expect = _chunk_labels(S, C, anchors, np.random.RandomState(5 + S + coco))
    ref = otg.multi_gt_creator(S, list(arch.STRIDES), labels, anchors)
    assert len(expect) == 3
    for b, sl, obj, cls in expect:
        assert ref[b, sl, 0] == obj and ref[b, sl, 1] == cls, "the oracle's slot (%d, %d) holds obj %g cls %g: no collision" % (b, sl, ref[b, sl, 0], ref[b, sl, 1])
        assert (ref[b, sl, 6] == -1.0) if obj < 0 else (ref[b, sl, 6] > 0), "an ignore write leaves weight -1, a positive its box weight"
    assert not ref[0].any() and (ref[1:, :, 0] > 0).any() and (ref[1:, :, 0] < 0).any()
    h = capi.Handle(S, C, anchors, "1.0x", max_batch=len(labels))
    got = h.make_targets(labels, anchors).cpu().numpy()
    h.close()
    _check(got, ref)
