"""Host restatement of the batched test-time augmentation (yn_tta_*, kernels_tta.hip) in numpy float32: the bilinear resize exactly as
include/yolonano_hip.h specifies it, the horizontal flip (utils/misc.py:120), the un-mirror of the flipped forward's boxes (:126) and
the list building (:114-130).  The merge itself is oracle.tta_merge (utils/misc.py:132-146), called once per image.

The resize, per axis with scale = float32(S0) / float32(s):
    src = max(fmaf(scale, d + 0.5, -0.5), 0)   - the product of two float32 is exact in float64 (48 bits) and so is the subtraction of
                                                 0.5 from it (a multiple of the product's last bit, the result no larger), so
                                                 "float64, then round once to float32" IS the fused multiply-add
    i0 = int(src), i1 = i0 + (i0 < S0 - 1), l1 = src - i0, l0 = 1 - l1
    v = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)   - numpy rounds every ufunc call on its own: no contraction
s == S0 is the identity (the reference hands x itself to the model, utils/misc.py:106-107)."""
import numpy as np

F32 = np.float32


def axis_taps(S0, s):
    """-> (i0, i1 int64 [s], l0, l1 float32 [s]) of one axis"""
    scale = F32(S0) / F32(s)
    d = np.arange(s, dtype=np.float32) + F32(0.5)
    src = (np.float64(scale) * d.astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, F32(0))
    i0 = np.minimum(src.astype(np.int64), S0 - 1)
    i1 = i0 + (i0 < S0 - 1)
    l1 = src - i0.astype(np.float32)
    l0 = F32(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0, l1


def taps(x, s):
    """The four taps a, b, c, d [B,3,s,s] (top-left, top-right, bottom-left, bottom-right) and the weights of resize(x, s)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    S0 = x.shape[-1]
    assert x.shape[-2] == S0
    i0, i1, l0, l1 = axis_taps(S0, s)
    a = x[:, :, i0[:, None], i0[None, :]]
    b = x[:, :, i0[:, None], i1[None, :]]
    c = x[:, :, i1[:, None], i0[None, :]]
    d = x[:, :, i1[:, None], i1[None, :]]
    return (a, b, c, d), (l0, l1)


def resize(x, s):
    """x float32 [B,3,S0,S0] -> [B,3,s,s]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.shape[-1] == s:
        return x.copy()
    (a, b, c, d), (l0, l1) = taps(x, s)
    l0w, l1w = l0[None, None, None, :], l1[None, None, None, :]
    l0h, l1h = l0[None, None, :, None], l1[None, None, :, None]
    top = l0w * a + l1w * b
    bot = l0w * c + l1w * d
    v = l0h * top + l1h * bot
    assert v.dtype == np.float32
    return v


def flip_pairs(r):
    """[B,3,s,s] -> [2B,3,s,s]: image 2b = r[b], image 2b + 1 = its horizontal mirror (torch.flip(x, [-1]))"""
    out = np.empty((2 * r.shape[0],) + r.shape[1:], dtype=np.float32)
    out[0::2] = r
    out[1::2] = r[..., ::-1]
    return out


def unmirror(boxes):
    """utils/misc.py:126 on a float32 [K,4] array: bboxes[:, 0::2] = 1.0 - bboxes[:, 2::-2]"""
    b = np.array(boxes, dtype=np.float32, copy=True)
    b[:, 0::2] = 1.0 - b[:, 2::-2]
    assert b.dtype == np.float32
    return b


def build_list(per_forward):
    """per_forward = [(boxes, scores, labels), ...] of ONE image in call order (scale 0 plain, scale 0 flipped, scale 1 plain, ...)
    -> (boxes [n,4] f32, scores [n] f32, labels [n] i64, start [forwards] = where each forward's rows begin): the reference's
    concatenation (utils/misc.py:132-134), odd forwards un-mirrored."""
    bb, sc, lb, start, n = [], [], [], [], 0
    for i, (b, s, l) in enumerate(per_forward):
        b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        bb.append(unmirror(b) if i & 1 else b.copy())
        sc.append(np.asarray(s, dtype=np.float32))
        lb.append(np.asarray(l, dtype=np.int64))
        start.append(n)
        n += len(b)
    return np.concatenate(bb), np.concatenate(sc), np.concatenate(lb), np.array(start, dtype=np.int64)
