"""Case tables and references of tests/test_gpu_train_tail_ops.py (csrc/kernels_train.hip: loss_kernel in its three instantiations with
loss_reduce_kernel, grad_finite_kernel, sgd_kernel, ema_kernel), importable without a GPU; tests/test_train_tail_cases_cpu.py shows that each
case has the property it claims.

loss64 restates models/yolo_nano.py:332-358 and tools.loss in torch at a chosen dtype (float64: the reference; float32: what the reference's own
arithmetic gives, the e32 of f64_bar.bar), gradients from autograd of the sum of the four losses.  It shares no formula with loss_kernel or with
oracle/loss.py, which both derive the gradients by hand.

Out of scope for the loss cases: |tw| or |th| large enough that fp32 exp overflows, or that an area underflows.  There the reference's own fp32
gives inf / NaN, and the kernel's "0/0 carries no gradient" rule is a choice of this project, not parity.  The inputs stay away from this
(tw, th within [-8, 8]); the CPU file asserts that no case's float64 or float32 reference holds a NaN or Inf.
"""
import numpy as np
import torch
import torch.nn.functional as F

from yolo_nano_amd import arch

A = 3
TIE_ANCHORS = [[8, 12], [16, 8], [12, 20], [24, 16], [20, 32], [32, 24], [48, 40], [40, 56], [60, 52]]   # even integers: t = 0 decodes to k / 64 exactly


# ---------------------------------------------------------------------------------------------------------------------------------------
# candidate geometry (models/yolo_nano.py:82-112): level by level, cell by cell (row-major), anchor by anchor
# ---------------------------------------------------------------------------------------------------------------------------------------
def candidates(S, anchors):
    """-> float64 arrays over the N candidates of one image: gx, gy, stride, aw, ah, and the level of each"""
    an = np.asarray(anchors, dtype=np.float64).reshape(3, A, 2)
    gx, gy, st, aw, ah, lv = [], [], [], [], [], []
    for s, stride in enumerate(arch.STRIDES):
        w = S // stride
        yy, xx = np.meshgrid(np.arange(w), np.arange(w), indexing="ij")
        gx.append(np.repeat(xx.reshape(-1), A)); gy.append(np.repeat(yy.reshape(-1), A))
        st.append(np.full(w * w * A, float(stride)))
        aw.append(np.tile(an[s, :, 0], w * w)); ah.append(np.tile(an[s, :, 1], w * w))
        lv.append(np.full(w * w * A, s))
    return tuple(np.concatenate(v).astype(np.float64) for v in (gx, gy, st, aw, ah)) + (np.concatenate(lv),)


def decode(t, S, anchors, dtype=torch.float64):
    """txtytwth [B,N,4] -> x1y1x2y2 / S [B,N,4], unclamped (models/yolo_nano.py:120-156, :336), in `dtype`"""
    gx, gy, st, aw, ah = (torch.as_tensor(v).to(dtype) for v in candidates(S, anchors)[:5])
    t = (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.array(t))).to(dtype)
    cxy = (torch.sigmoid(t[..., :2]) + torch.stack([gx, gy], -1)) * st[:, None]
    wh = torch.exp(t[..., 2:]) * torch.stack([aw, ah], -1)
    return torch.cat([cxy - wh / 2, cxy + wh / 2], -1) / S


def loss64(conf, cls, t, target, S, anchors, dtype=torch.float64):
    """conf [B,N], cls [B,N,C], t [B,N,4], target [B,N,11] -> dict: losses [4] (dtype), terms [4][B,N] (the per-candidate summands of each loss, / B
    included), g_conf, g_cls, g_t (autograd of the sum of the four losses), iou [B,N]"""
    conf, cls, t = (torch.as_tensor(np.array(v)).to(dtype).requires_grad_(True) for v in (conf, cls, t))
    target = torch.as_tensor(np.array(target)).to(dtype)
    B, N, C = cls.shape
    obj, gcls, gt_t, wgt, gt_box = target[..., 0], target[..., 1].long(), target[..., 2:6], target[..., 6], target[..., 7:11]
    box = decode(t, S, anchors, dtype)
    tl, br = torch.max(box[..., :2], gt_box[..., :2]), torch.min(box[..., 2:], gt_box[..., 2:])
    area_a, area_b = torch.prod(box[..., 2:] - box[..., :2], -1), torch.prod(gt_box[..., 2:] - gt_box[..., :2], -1)
    en = (tl < br).to(dtype).prod(-1)
    area_i = torch.prod(br - tl, -1) * en
    iou = area_i / (area_a + area_b - area_i)
    pos, neg, mask = (obj == 1).to(dtype), (obj == 0).to(dtype), (obj > 0).to(dtype)
    sg = torch.sigmoid(conf)
    terms = [
        (5.0 * pos * (sg - iou.detach()) ** 2 + neg * sg ** 2) / B,
        F.cross_entropy(cls.reshape(B * N, C), gcls.reshape(B * N), reduction="none").reshape(B, N) * mask / B,
        (F.binary_cross_entropy_with_logits(t[..., :2], gt_t[..., :2], reduction="none").sum(-1) * wgt * mask
         + F.mse_loss(t[..., 2:], gt_t[..., 2:], reduction="none").sum(-1) * wgt * mask) / B,
        F.smooth_l1_loss(iou, mask, reduction="none") / B,
    ]
    losses = torch.stack([v.sum() for v in terms])
    g_conf, g_cls, g_t = torch.autograd.grad(losses.sum(), [conf, cls, t])
    return {"losses": losses.detach(), "terms": [v.detach() for v in terms], "g_conf": g_conf, "g_cls": g_cls, "g_t": g_t, "iou": iou.detach(), "en": en}


def to_heads(conf, cls, t, S):
    """the split layout -> the three dense raw heads [B, S/s, S/s, A(5+C)] (models/yolo_nano.py:308-330 backwards)"""
    conf, cls, t = (torch.as_tensor(np.array(v)) for v in (conf, cls, t))
    B, N, C = cls.shape
    heads, off = [], 0
    for s in arch.STRIDES:
        w = S // s
        sl = slice(off, off + w * w * A)
        hd = torch.cat([conf[:, sl].reshape(B, w * w, A), cls[:, sl].reshape(B, w * w, A * C), t[:, sl].reshape(B, w * w, A * 4)], -1)
        heads.append(hd.reshape(B, w, w, A * (5 + C)).contiguous())
        off += w * w * A
    return heads


def from_heads(heads, C):
    """three [B, S/s, S/s, A(5+C)] tensors -> (conf [B,N], cls [B,N,C], t [B,N,4])"""
    conf, cls, t = [], [], []
    for hd in heads:
        B, w = hd.shape[0], hd.shape[1]
        hd = hd.reshape(B, w * w, A * (5 + C))
        conf.append(hd[:, :, :A].reshape(B, w * w * A))
        cls.append(hd[:, :, A:A + A * C].reshape(B, w * w * A, C))
        t.append(hd[:, :, A + A * C:].reshape(B, w * w * A, 4))
    return torch.cat(conf, 1), torch.cat(cls, 1), torch.cat(t, 1)


def loss_blocks(S, B):
    """workgroups of loss_kernel = partials of loss_reduce_kernel (loss_num_blocks)"""
    return (B * arch.num_predictions(S) + 255) // 256


def head_row(C):
    """(dense, physical) width of a raw-head row of the fp16 step: A(5+C) rounded up to a multiple of 8"""
    hc = A * (5 + C)
    return hc, (hc + 7) & ~7


# ---------------------------------------------------------------------------------------------------------------------------------------
# loss cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def _logits(rs, S, C, B):
    N = arch.num_predictions(S)
    return (rs.standard_normal((B, N)).astype(np.float32), rs.standard_normal((B, N, C)).astype(np.float32),
            (rs.standard_normal((B, N, 4)) * 0.5).astype(np.float32), np.zeros((B, N, 11), np.float32))


def _near(rs, box):
    """a ground-truth box that overlaps the decoded `box` [n,4]: every edge moved by up to 30 % of the box's size"""
    wh = np.concatenate([box[:, 2:] - box[:, :2]] * 2, -1)
    return box + rs.uniform(-0.3, 0.3, box.shape) * wh


def _fill(rs, target, b, idx, C, box):
    n = len(idx)
    target[b, idx, 0] = 1.0
    target[b, idx, 1] = rs.randint(0, C, n)
    target[b, idx, 2:4] = rs.uniform(0, 1, (n, 2))
    target[b, idx, 4:6] = rs.standard_normal((n, 2)) * 0.3
    target[b, idx, 6] = rs.uniform(1.0, 2.0, n)
    target[b, idx, 7:11] = box


def _ignore(target, b, idx):
    target[b, idx, 0] = -1.0                                  # tools.py:206-207: the ignore write touches obj and weight, nothing else
    target[b, idx, 6] = -1.0


def _random(rs, S, C, B, anchors, n_pos, n_ign, n_ign_box=0, skip_images=()):
    """n_pos positives per image with boxes near their prediction, n_ign ignored slots with an all-zero box (what multi_gt_creator writes into
    an untouched slot), n_ign_box ignored slots that still carry a positive's class and box"""
    conf, cls, t, target = _logits(rs, S, C, B)
    N = conf.shape[1]
    pred = decode(t, S, anchors).numpy()
    for b in range(B):
        idx = rs.choice(N, n_pos + n_ign + n_ign_box, replace=False)
        p, i0, i1 = idx[:n_pos], idx[n_pos:n_pos + n_ign], idx[n_pos + n_ign:]
        if b in skip_images:
            p = p[:0]
        _fill(rs, target, b, p, C, _near(rs, pred[b, p]))
        _fill(rs, target, b, i1, C, _near(rs, pred[b, i1]))
        _ignore(target, b, i1)
        _ignore(target, b, i0)
    return conf, cls, t, target


def _build_random(n_pos, n_ign, **kw):
    return lambda rs, S, C, B, anchors: _random(rs, S, C, B, anchors, n_pos, n_ign, **kw)


TIE_SHARED = (0, 1, 2, 3, 4)
TIE_PER_COUNT = 9                                           # 45 positives, 15 per image


def _build_ties(rs, S, C, B, anchors):
    conf, cls, t, target = _random(rs, S, C, B, anchors, 0, 4)
    N = conf.shape[1]
    counts = np.repeat(TIE_SHARED, TIE_PER_COUNT)
    rs.shuffle(counts)
    per = len(counts) // B
    for b in range(B):
        free = np.flatnonzero(target[b, :, 0] == 0)
        idx = rs.choice(free, per, replace=False)
        t[b, idx] = 0.0                                       # sigmoid 0.5, exp 1: the decoded box is (integers) / 64
        box = decode(t, S, anchors).numpy()[b, idx]
        gt = box.copy()
        for k, shared in enumerate(counts[b * per:(b + 1) * per]):
            moved = rs.permutation(4)[shared:]                # the edges that do NOT coincide: by 1..3 / 64, inward or outward
            gt[k, moved] += rs.choice([-3, -2, -1, 1, 2, 3], len(moved)) / 64.0
        _fill(rs, target, b, idx, C, gt)
    return conf, cls, t, target


def tie_slots(target, t):
    """the positives of the `ties` case: those whose prediction is all zero"""
    return (np.asarray(target)[..., 0] == 1) & (np.asarray(t) == 0).all(-1)


def _build_miss(rs, S, C, B, anchors):
    conf, cls, t, target = _random(rs, S, C, B, anchors, 3, 3)
    N = conf.shape[1]
    for b in range(B):
        free = np.flatnonzero(target[b, :, 0] == 0)
        idx = rs.choice(free, 4, replace=False)
        t[b, idx, 2:] = -3.0
        box = decode(t, S, anchors).numpy()[b, idx]
        c = (box[:, :2] + box[:, 2:]) / 2
        far = np.where(c < 0.5, 0.8, 0.2) + rs.uniform(-0.05, 0.05, c.shape)      # the far side of the image, in x and in y
        wh = rs.uniform(0.05, 0.12, c.shape)
        _fill(rs, target, b, idx, C, np.concatenate([far - wh / 2, far + wh / 2], -1))
    return conf, cls, t, target


def miss_slots(target, t):
    return (np.asarray(target)[..., 0] == 1) & (np.asarray(t)[..., 2] == -3.0) & (np.asarray(t)[..., 3] == -3.0)


def _build_dense(rs, S, C, B, anchors):
    conf, cls, t, target = _random(rs, S, C, B, anchors, 5, 3)
    N = conf.shape[1]
    b = 1
    target[b] = 0.0
    _fill(rs, target, b, np.arange(N), C, _near(rs, decode(t, S, anchors).numpy()[b]))
    return conf, cls, t, target


def _build_saturated(rs, S, C, B, anchors):
    conf, cls, t, _ = _logits(rs, S, C, B)
    N = conf.shape[1]
    conf[:] = rs.choice([-100.0, -50.0, -20.0, 20.0, 50.0, 100.0], conf.shape)
    sat = rs.uniform(size=(B, N)) < 0.3                       # on negatives and positives alike
    t[..., :2] = np.where(sat[..., None], rs.choice([-60.0, 60.0], (B, N, 2)), t[..., :2])
    wide = rs.uniform(size=(B, N)) < 0.3
    t[..., 2:] = np.where(wide[..., None], rs.uniform(-8.0, 8.0, (B, N, 2)), t[..., 2:])
    target = np.zeros((B, N, 11), np.float32)
    pred = decode(t, S, anchors).numpy()
    for b in range(B):
        idx = rs.choice(N, 24, replace=False)
        p, i0, i1 = idx[:16], idx[16:20], idx[20:]
        _fill(rs, target, b, p, C, _near(rs, pred[b, p]))
        _fill(rs, target, b, i1, C, _near(rs, pred[b, i1]))
        _ignore(target, b, i1)
        _ignore(target, b, i0)
        cls[b, p[:8]] *= 40.0                                 # the log-sum-exp spread
    return conf, cls, t, target


VOC, COCO = arch.MULTI_ANCHOR_SIZE, arch.MULTI_ANCHOR_SIZE_COCO
# id, S, C, B, anchors, builder, seed
LOSS_CASES = [
    ("s32-b1-c1", 32, 1, 1, VOC, _build_random(6, 3, n_ign_box=2), 101),
    ("s64-b3-c20", 64, 20, 3, VOC, _build_random(12, 6, n_ign_box=4), 102),
    ("s64-b64-c20", 64, 20, 64, VOC, _build_random(6, 3, n_ign_box=2), 103),
    ("s128-b66-c20", 128, 20, 66, VOC, _build_random(8, 4, n_ign_box=2), 104),
    ("s64-b2-c80", 64, 80, 2, COCO, _build_random(12, 6, n_ign_box=4), 105),
    ("ties", 64, 20, 3, TIE_ANCHORS, _build_ties, 106),
    ("ignored-box", 64, 20, 3, VOC, _build_random(8, 2, n_ign_box=4), 107),
    ("miss", 64, 20, 3, VOC, _build_miss, 108),
    ("none", 64, 20, 3, VOC, _build_random(0, 4, n_ign_box=3), 109),
    ("none-one", 64, 20, 3, VOC, _build_random(8, 4, n_ign_box=3, skip_images=(1,)), 110),
    ("dense", 64, 20, 3, VOC, _build_dense, 111),
    ("saturated", 64, 20, 3, VOC, _build_saturated, 112),
]
LOSS_IDS = [c[0] for c in LOSS_CASES]
LOSS_BLOCKS = {"s32-b1-c1": 1, "s64-b3-c20": 3, "s64-b64-c20": 63, "s128-b66-c20": 260}
_built = {}


def loss_case(cid, fp16_inputs=False):
    """-> dict: S, C, B, anchors, conf, cls, t, target (float32 numpy, never modified), ref64 / ref32 (loss64 at both dtypes, computed once).
    fp16_inputs: the predictions rounded to fp16 first (what the fp16 route sees), a case of its own."""
    key = (cid, fp16_inputs)
    if key not in _built:
        _, S, C, B, anchors, builder, seed = LOSS_CASES[LOSS_IDS.index(cid)]
        conf, cls, t, target = builder(np.random.RandomState(seed), S, C, B, anchors)
        if fp16_inputs:
            conf, cls, t = (v.astype(np.float16).astype(np.float32) for v in (conf, cls, t))
        c = {"id": cid, "S": S, "C": C, "B": B, "anchors": anchors, "conf": conf, "cls": cls, "t": t, "target": target}
        c["ref64"] = loss64(conf, cls, t, target, S, anchors, torch.float64)
        c["ref32"] = loss64(conf, cls, t, target, S, anchors, torch.float32)
        for v in (conf, cls, t, target):
            v.setflags(write=False)
        _built[key] = c
    return _built[key]


def groups(target):
    """the three kinds of candidate, as boolean [B,N] arrays: positives, negatives, ignored slots"""
    obj = np.asarray(target)[..., 0]
    return {"pos": obj == 1, "neg": obj == 0, "ign": obj == -1}


def loss_value_bar(ref64, ref32):
    """[4] bars of the loss values.  Every term is non-negative; a block's sum is an fp32 tree of depth 8 (six shuffle steps, two LDS steps), the sum
    over blocks is double: |L - L64| <= 8 * 2**-24 * L64 + 4 * sum |term32 - term64|"""
    return [8 * 2.0 ** -24 * float(a.sum()) + 4 * float((b.double() - a).abs().sum()) for a, b in zip(ref64["terms"], ref32["terms"])]


# ---------------------------------------------------------------------------------------------------------------------------------------
# SGD, the finite scan, EMA
# ---------------------------------------------------------------------------------------------------------------------------------------
SGD_GRID_CAP = 2048                                         # launch_sgd: at most 2048 workgroups of 256 threads, four elements a thread
SGD_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 1023, 1025, 5003, 2097152 + 3075]
SGD_EXACT = dict(lr=2.0 ** -3, momentum=0.5, weight_decay=2.0 ** -4, grad_scale=0.5)
SGD_REFERENCE = dict(lr=1e-3, momentum=0.9, weight_decay=5e-4)          # train.py:167-171
SCAN_LENGTHS = [5003, 600001]
SCAN_VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
FLT_MAX = float(np.finfo(np.float32).max)


def sgd_blocks(n):
    return max(1, min(SGD_GRID_CAP, ((n >> 2) + 255) // 256))


def sgd_trips(n):
    """trips of sgd_kernel's grid-stride loop over the float4 body"""
    per = sgd_blocks(n) * 256
    return ((n >> 2) + per - 1) // per


def scan_stride(n):
    """elements grad_finite_kernel covers per trip: min(the SGD grid, 512) workgroups of 256 threads, one element a thread"""
    return min(sgd_blocks(n), 512) * 256


def scan_placements(n):
    """where the non-finite element sits: name -> index"""
    st = scan_stride(n)
    k = (n - 1) // st
    late = k * st + 5 if k * st + 5 < n else (k - 1) * st + 5
    return {"first": 0, "last": n - 1, "tail": n & ~3, "late-stride": late}


def sgd64(p, g, buf, lr, momentum, weight_decay, grad_scale, first):
    """one step of torch.optim.SGD(momentum, weight_decay), dampening 0, on float64 tensors -> (p, buf)"""
    d = g * grad_scale + weight_decay * p
    buf = d if first else momentum * buf + d
    return p - lr * buf, buf


EMA_LENGTHS = [1, 257, 524288 + 257]                       # launch_ema: at most 2048 workgroups of 256 threads, one element a thread
EMA_DECAYS = {"zero": 0.0, "ramp-first": 0.9999 * (1.0 - np.exp(-1.0 / 2000.0)), "late": 0.9999}      # utils/misc.py:72-86


def ema32(v, m, decay):
    """ModelEMA.update with torch's three float32 roundings: fl(fl(v * d) + fl((1 - d) * m)), d and 1 - d rounded to float32 first"""
    d, omd = np.float32(decay), np.float32(1.0 - decay)
    return (v.astype(np.float32) * d).astype(np.float32) + (omd * m.astype(np.float32)).astype(np.float32)
