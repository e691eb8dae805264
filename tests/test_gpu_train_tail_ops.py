"""The kernels every training step ends in (csrc/kernels_train.hip) on their own against float64: loss_kernel<false, float> (Handle.loss),
loss_kernel<true, float> (Handle.loss_heads), loss_kernel<true, fp16> (Handle.op_h16_loss, the fp16 step's), each with loss_reduce_kernel;
grad_finite_kernel and sgd_kernel (Handle.sgd_step); ema_kernel (Handle.ema_update).  The case tables and the references are
tests/train_tail_cases.py; tests/test_train_tail_cases_cpu.py shows without a GPU that each case has the property it claims.

Which case reaches what (every loss case runs in the split layout, in the heads layout and through op_h16_loss at loss scale 1 and 1024):
  s32-b1-c1      one workgroup whose last wave is not full (63 candidates); C = 1: class loss exactly 0.0, g_cls exactly 0
  s64-b3-c20     three workgroups, the last ragged (756 candidates); image and level boundaries inside workgroups
  s64-b64-c20    63 full workgroups, no ragged one
  s128-b66-c20   260 partials: loss_reduce_kernel's loop takes a second trip; also the ensure_loss regrow (B = 1, 66, 1 on one handle against fresh ones)
  s64-b2-c80     dense head rows of 255 floats (odd stride); physical fp16 rows of 256
  ties           45 positives with t = 0 and integer anchors: decoded boxes are k / 64 exactly; target boxes share 0..4 edges with them, the others moved
                 by 1..3 / 64 inward and outward: the 0.5 tie weights of torch.max / torch.min, and iou == 1 (needs expf(0) == 1 and 1 / (1 + 1) == 0.5)
  ignored-box    slots with obj -1, weight -1 that still carry a class and an overlapping box: an IoU term and an IoU gradient, nothing else
                 (every random case carries a few such slots as well)
  miss           positives with tw = th = -3 whose box lies on the far side of the image: en == 0, the |d| == 1 seam of SmoothL1, 0.5 / B each
  none, none-one no image / one image of three has a positive; class and box loss are exactly 0.0 in `none`
  dense          every candidate of one image is a positive
  saturated      conf in +-{20, 50, 100} (expf(-v) overflows in sigmoid_t), class rows * 40 (the log-sum-exp spread), tx / ty = +-60, tw / th in [-8, 8]
  SGD            n = 0 (refused before this suite: now a step that does nothing), 1, 2, 3, 4, 5, 7 (no float4 body / every tail), 1023, 1025, 5003, and
                 2 097 152 + 3075: a second trip of the grid-stride loop (the grid is capped at 2048 workgroups) with a tail of 3; first_step 0 and 1, three
                 steps each; sentinel elements behind every bucket
  scan           one NaN / +Inf / -Inf at the first element, the last, the first tail element n & ~3 and in the scan's fourth trip or later, n = 5003 and
                 600 001: parameters and momentum unchanged bit for bit, skipped_steps() + 1, a clean step afterwards applies.  +-FLT_MAX with grad_scale
                 2**-126 is a normal step: grad_finite_kernel tested |v| <= 3.0e38 and skipped finite gradients in (3.0e38, FLT_MAX]; it now tests <= FLT_MAX
  EMA            n = 1, 257, 524 288 + 257 (past the 2048-workgroup cap) at decay 0, the ramp's first value and 0.9999, two updates each, bit for bit

Bars.  Gradients: f64_bar.bar (4 * e32 + 4 ulp, e32 = loss64 in float32 on the CPU against loss64 in float64, both autograd), taken separately for g_conf,
g_cls, g_t and for positives, negatives and ignored slots.  Loss values: |L - L64| <= 8 * 2**-24 * L64 + 4 * sum |term32 - term64| (all terms are non-negative;
a workgroup's sum is an fp32 tree of depth 8, the sum over workgroups is double).  fp16 route: losses bit-identical to loss_heads on the same fp16-rounded
heads; gradients equal (fp32 gradient * scale) rounded once to fp16 in every bit but the sign of a zero; f64_bar.bar16 against float64; pad count 0.
Exact on top: g_cls == g_t == 0 where obj is 0 and the box is zero, g_conf == g_cls == 0 on ignored slots, split and heads layouts bit-identical, the same
losses without gradients, gradient buffers pre-filled with NaN come back finite.

Measured on an MI355X: the worst (error / bar) of each output over all cases, with the case.  149 tests, 5.3 s.
  g_conf   0.250  saturated, positives     g_cls    0.174  s128-b66-c20, positives   g_t      0.251  saturated, ignored slots
  L conf   0.224  saturated                L cls    0.130  ignored-box               L box    0.241  dense               L iou  0.219  saturated
  fp16 g_conf  0.995  s64-b64-c20, negatives   fp16 g_cls  0.997  s64-b64-c20, positives   fp16 g_t  0.994  s128-b66-c20, positives
           (an fp16-stored value sits just under 1.0 by nature: a correctly rounded value is up to half a spacing away)
  sgd p    0.139  n 2 100 227              sgd buf  0.250  n 1
Every exact statement held, `ties` included.  One finding, stated rather than changed: two of the fp16 kernel's stores (the objectness gradient is one) are
compiled into v_fma_mixlo_f16 (gradient * scale + 0 -> fp16), so a product of -0 (a positive whose sigmoid underflowed to 0: conf = -100 in `saturated`, 2 of
14 400 elements of head 0) is stored as +0 where the rounded fp32 product is -0.  Every other bit pattern, infinities included, is identical.

The cases notice.  Tried once with deliberately wrong libraries in a scratch copy (arithmetic and strides only, no access outside a buffer), 149 tests each:
  tie weights 1.0 for 0.5, the fp16 rows read with stride A(5+C) for the physical one, the SGD tail dropped, the scan started at index 1: 68 fail.
  The tie weights fail test_loss_gradients[ties] alone among the fp32 loss tests (and both fp16 ties tests); the stride fails all 24 test_loss_h16 and no fp32
  test; the dropped tail fails test_sgd_exact and test_sgd_random at every n with n % 4 != 0 and the FLT_MAX step (n = 0 and 4 rightly pass); the scan fails
  the six `first` placements and no other (`tail` and `late-stride` rightly pass).
  the IoU term dropped for obj -1, the last thread of a ragged workgroup skipped: 70 fail.  s64-b64-c20 has no ragged workgroup: there the gradient bar of the
  ignored slots (g_t error 1.1e-02 against 2.4e-08), the IoU loss value and the fp16 tests fail, the exact statements and the layout comparison rightly
  pass; in the other eleven cases the skipped thread leaves the NaN of the pre-filled g_conf in place (test_loss_gradients), breaks the exact statements
  and the split-against-heads comparison (yn_loss_heads zeroes its buffers, yn_loss does not zero g_conf).  The regrow, SGD and EMA tests pass.
"""
import numpy as np
import pytest
import torch

import train_tail_cases as tc
from f64_bar import bar, bar16
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu
GRADS = ("g_conf", "g_cls", "g_t")
LOSSES = ("conf", "cls", "box", "iou")


def dev(a):
    return torch.as_tensor(np.array(a)).cuda()                # (a copy: the cases' arrays are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    """bit for bit, signs of zero included"""
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, (what, a.shape, b.shape)
    if not torch.equal(_bits(a), _bits(b)):
        bad = (_bits(a) != _bits(b)).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r against %r" % (what, len(bad), a.numel(), i, float(a[i]), float(b[i])))


def _handle(S, C, anchors):
    from yolo_nano_amd import capi
    return capi.Handle(S, C, anchors)


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(c):
        key = (c["S"], c["C"], repr(c["anchors"]))
        if key not in made:
            made[key] = _handle(c["S"], c["C"], c["anchors"])
        return made[key]
    yield get
    for h in made.values():
        h.close()


def _nan_like(shape):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device="cuda")


def _split(h, c, B=None):
    """Handle.loss into NaN-filled gradient buffers -> (losses, g_conf, g_cls, g_t) on the CPU"""
    conf, cls, t, target = (dev(c[k][:B]) for k in ("conf", "cls", "t", "target"))
    out = (_nan_like(conf.shape), _nan_like(cls.shape), _nan_like(t.shape))
    losses, g = h.loss(conf, cls, t, target, out=out)
    return (losses.cpu(),) + tuple(v.cpu() for v in g)


def _heads(h, c, B=None):
    """Handle.loss_heads into NaN-filled gradient buffers -> (losses, g_conf, g_cls, g_t) on the CPU, back in the split layout"""
    heads = [v.cuda() for v in tc.to_heads(c["conf"][:B], c["cls"][:B], c["t"][:B], c["S"])]
    losses, g = h.loss_heads(heads, dev(c["target"][:B]), out=[_nan_like(v.shape) for v in heads])
    return (losses.cpu(),) + tuple(v.contiguous() for v in tc.from_heads([v.cpu() for v in g], c["C"]))


_ran = {}


def _run(handles, cid):
    """both fp32 layouts of a case, once"""
    if cid not in _ran:
        c = tc.loss_case(cid)
        h = handles(c)
        _ran[cid] = (_split(h, c), _heads(h, c))
    return _ran[cid]


# ---------------------------------------------------------------------------------------------------------------------------------------
# loss, fp32
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", tc.LOSS_IDS)
def test_loss_gradients(handles, cid):
    """g_conf, g_cls, g_t of both layouts against float64 autograd: 4 * e32 + 4 ulp, taken separately over positives, negatives and ignored slots"""
    c = tc.loss_case(cid)
    for layout, got in zip(("split", "heads"), _run(handles, cid)):
        for name, g in zip(GRADS, got[1:]):
            assert bool(torch.isfinite(g).all()), "%s %s: a NaN of the pre-filled buffer survived, or a non-finite gradient" % (layout, name)
            for grp, keep in tc.groups(c["target"]).items():
                if keep.any():
                    k = torch.from_numpy(keep)
                    bar(name, "%s %s %s" % (cid, layout, grp), g[k], c["ref64"][name][k], c["ref32"][name][k])


@pytest.mark.parametrize("cid", tc.LOSS_IDS)
def test_loss_exact_statements(handles, cid):
    c = tc.loss_case(cid)
    target, grp = c["target"], tc.groups(c["target"])
    untouched = torch.from_numpy(grp["neg"] & (target[..., 7:11] == 0).all(-1))
    ign = torch.from_numpy(grp["ign"])
    for layout, (losses, g_conf, g_cls, g_t) in zip(("split", "heads"), _run(handles, cid)):
        assert not g_cls[untouched].any() and not g_t[untouched].any(), "%s: a candidate with obj 0 and a zero box has a class / box gradient" % layout
        assert not g_conf[ign].any() and not g_cls[ign].any(), "%s: an ignored slot has an objectness / class gradient" % layout
        if c["C"] == 1:
            assert not g_cls.any() and float(losses[1]) == 0.0
        if cid == "none":
            assert float(losses[1]) == 0.0 and float(losses[2]) == 0.0
        if cid == "miss":                                     # the float64 gradient there is the box-regression term alone (shown in the CPU file)
            miss = torch.from_numpy(tc.miss_slots(target, c["t"]))
            bar("g_t", "%s %s missed" % (cid, layout), g_t[miss], c["ref64"]["g_t"][miss], c["ref32"]["g_t"][miss])
    if cid == "ignored-box":
        k = torch.from_numpy(grp["ign"] & (target[..., 7:11] != 0).any(-1))
        assert int(k.sum()) >= 10 and bool((c["ref64"]["g_t"][k].abs().sum(-1) > 0).all())
        for layout, got in zip(("split", "heads"), _run(handles, cid)):
            assert bool((got[3][k].abs().sum(-1) > 0).all()), "%s: an ignored slot with a box lost its IoU gradient" % layout


@pytest.mark.parametrize("cid", tc.LOSS_IDS)
def test_loss_layouts_identical_and_forward_only(handles, cid):
    c = tc.loss_case(cid)
    h = handles(c)
    split, heads = _run(handles, cid)
    for name, a, b in zip(("losses",) + GRADS, split, heads):
        _same(a, b, "%s: %s, split against heads" % (cid, name))
    l1, none1 = h.loss(dev(c["conf"]), dev(c["cls"]), dev(c["t"]), dev(c["target"]), grads=False)
    l2, none2 = h.loss_heads([v.cuda() for v in tc.to_heads(c["conf"], c["cls"], c["t"], c["S"])], dev(c["target"]), grads=False)
    assert none1 is None and none2 is None
    _same(l1.cpu(), split[0], "%s: losses without gradients, split" % cid)
    _same(l2.cpu(), split[0], "%s: losses without gradients, heads" % cid)


@pytest.mark.parametrize("cid", tc.LOSS_IDS)
def test_loss_values(handles, cid):
    """|L - L64| <= 8 * 2**-24 * L64 + 4 * sum |term32 - term64| (train_tail_cases.loss_value_bar)"""
    c = tc.loss_case(cid)
    losses = _run(handles, cid)[0][0].double()
    bars = tc.loss_value_bar(c["ref64"], c["ref32"])
    worst = []
    for k, name in enumerate(LOSSES):
        err = abs(float(losses[k]) - float(c["ref64"]["losses"][k]))
        ratio = err / bars[k] if bars[k] > 0 else (0.0 if err == 0 else float("inf"))
        print("RATIO loss-%-4s %-14s L64 %.9e  err %.3e  bar %.3e  err/bar %.3f" % (name, cid, float(c["ref64"]["losses"][k]), err, bars[k], ratio))
        worst.append((ratio, name, err, bars[k]))
    for ratio, name, err, b in worst:
        assert ratio <= 1.0, "%s loss of %s: error %.3e against %.3e" % (name, cid, err, b)


def test_loss_partials_regrow():
    """one handle at B = 1, then 66 (ensure_loss grows the partials: 4 -> 260 workgroups), then 1 again: each result is a fresh handle's, bit for bit"""
    c = tc.loss_case("s128-b66-c20")
    assert tc.loss_blocks(c["S"], 1) == 4 and tc.loss_blocks(c["S"], 66) == 260
    h = _handle(c["S"], c["C"], c["anchors"])
    try:
        for B in (1, 66, 1):
            fresh = _handle(c["S"], c["C"], c["anchors"])
            try:
                want = _split(fresh, c, B) + _heads(fresh, c, B)
            finally:
                fresh.close()
            got = _split(h, c, B) + _heads(h, c, B)
            for k, (a, b) in enumerate(zip(got, want)):
                _same(a, b, "B = %d, output %d" % (B, k))
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# loss, the fp16 step's instantiation
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1024.0])
@pytest.mark.parametrize("cid", tc.LOSS_IDS)
def test_loss_h16(handles, cid, scale):
    c = tc.loss_case(cid, fp16_inputs=True)                  # rounded by the test: both routes see the same numbers
    h = handles(c)
    hc, hcp = tc.head_row(c["C"])
    assert hcp != hc
    heads = [v.cuda() for v in tc.to_heads(c["conf"], c["cls"], c["t"], c["S"])]
    target = dev(c["target"])
    l32, g32 = h.loss_heads(heads, target)
    l16, g16, pad = h.op_h16_loss(heads, target, scale=scale)
    l16n, none, _ = h.op_h16_loss(heads, target, scale=scale, grads=False)
    assert none is None
    _same(l16.cpu(), l32.cpu(), "%s: losses, fp16 rows against fp32 heads" % cid)
    _same(l16n.cpu(), l32.cpu(), "%s: losses without gradients" % cid)
    assert pad == 0, "%d elements of the pad columns of the fp16 gradient rows were written" % pad
    want = [(g * scale).to(torch.float16).float().cpu() for g in g32]          # the fp32 product rounded once
    for k, (a, b) in enumerate(zip(g16, want)):
        # every bit but the sign of a zero: the compiler fuses two of the kernel's stores into fma(gradient, scale, +0) -> fp16 (v_fma_mixlo_f16),
        # which stores the product -0 as +0 (a positive whose sigmoid underflowed to 0: `saturated`)
        _same(a.cpu() + 0.0, b + 0.0, "%s scale %g: gradient of head %d against (fp32 gradient * scale) rounded to fp16" % (cid, scale, k))
    got = [v.contiguous() for v in tc.from_heads([v.cpu() for v in g16], c["C"])]
    fin = [v.contiguous() for v in tc.from_heads([torch.isfinite(v) for v in want], c["C"])]
    for name, g, f in zip(GRADS, got, fin):
        for grp, keep in tc.groups(c["target"]).items():
            k = torch.from_numpy(keep)
            if k.any():
                bar16(name, "%s x%g %s" % (cid, scale, grp), g[k], c["ref64"][name][k] * scale, c["ref32"][name][k].double() * scale, keep=f[k])


# ---------------------------------------------------------------------------------------------------------------------------------------
# SGD and the finite scan
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hop():
    h = _handle(64, 20, arch.MULTI_ANCHOR_SIZE)
    yield h
    h.close()


GUARD = 8


def _guarded(v):
    """v on the device with GUARD sentinel elements behind it -> (the whole buffer, the view of v's length)"""
    full = torch.cat([torch.as_tensor(v, dtype=torch.float32), torch.full((GUARD,), 77.0)]).cuda()
    return full, full[:len(v)]


def _guards_intact(*fulls):
    for f in fulls:
        assert bool((f[-GUARD:] == 77.0).all()), "an element behind the bucket was written"


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n", tc.SGD_LENGTHS)
def test_sgd_exact(hop, n, first):
    """integers in {-3..3}, lr 2**-3, momentum 0.5, weight decay 2**-4, grad_scale 0.5: every operation is exact in fp32 (shown in the CPU file)"""
    rs = np.random.RandomState(1000 + n % 997)
    p0, b0 = (rs.randint(-3, 4, n).astype(np.float32) for _ in range(2))
    skipped = hop.skipped_steps()
    pf, p = _guarded(p0)
    bf, buf = _guarded(np.full(n, np.nan, np.float32) if first else b0)      # a first step never reads the momentum
    p64, b64 = torch.from_numpy(p0).double(), torch.from_numpy(b0).double()
    for step in range(3):
        g0 = rs.randint(-3, 4, n).astype(np.float32)
        gf, g = _guarded(g0)
        hop.sgd_step(p, g, buf, first_step=bool(first) and step == 0, **tc.SGD_EXACT)
        p64, b64 = tc.sgd64(p64, torch.from_numpy(g0).double(), b64, first=bool(first) and step == 0, **tc.SGD_EXACT)
        assert torch.equal(p.cpu().double(), p64) and torch.equal(buf.cpu().double(), b64), "n = %d, step %d" % (n, step)
        assert torch.equal(g.cpu(), torch.from_numpy(g0))
        _guards_intact(pf, bf, gf)
    assert hop.skipped_steps() == skipped


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n", tc.SGD_LENGTHS[1:])
def test_sgd_random(hop, n, first):
    """the reference's lr, momentum and weight decay on normal data against float64; e32 from torch.optim.SGD in fp32 on the CPU"""
    rs = np.random.RandomState(2000 + n % 997)
    p0, b0 = (rs.standard_normal(n).astype(np.float32) for _ in range(2))
    world = 8                                                 # the bucket holds the sum over 8 ranks: grad_scale 1/8 (exact)
    pf, p = _guarded(p0)
    bf, buf = _guarded(np.full(n, np.nan, np.float32) if first else b0)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([ref], **tc.SGD_REFERENCE)
    if not first:
        opt.state[ref]["momentum_buffer"] = torch.from_numpy(b0.copy())
    p64, b64 = torch.from_numpy(p0).double(), torch.from_numpy(b0).double()
    for step in range(3):
        g0 = rs.standard_normal(n).astype(np.float32)
        hop.sgd_step(p, dev(g0 * world), buf, grad_scale=1.0 / world, first_step=bool(first) and step == 0, **tc.SGD_REFERENCE)
        ref.grad = torch.from_numpy(g0.copy())
        opt.step()
        p64, b64 = tc.sgd64(p64, torch.from_numpy(g0).double(), b64, tc.SGD_REFERENCE["lr"], tc.SGD_REFERENCE["momentum"],
                            tc.SGD_REFERENCE["weight_decay"], 1.0, bool(first) and step == 0)
        bar("sgd p", "n %d first %d step %d" % (n, first, step), p.cpu(), p64, ref.detach())
        bar("sgd buf", "n %d first %d step %d" % (n, first, step), buf.cpu(), b64, opt.state[ref]["momentum_buffer"])
    _guards_intact(pf, bf)


@pytest.mark.parametrize("value", sorted(tc.SCAN_VALUES))
@pytest.mark.parametrize("place", ["first", "last", "tail", "late-stride"])
@pytest.mark.parametrize("n", tc.SCAN_LENGTHS)
def test_sgd_skips_a_bucket_with_one_non_finite_element(hop, n, place, value):
    rs = np.random.RandomState(3000 + n % 997)
    p0, b0, g0 = (rs.standard_normal(n).astype(np.float32) for _ in range(3))
    bad = g0.copy()
    bad[tc.scan_placements(n)[place]] = tc.SCAN_VALUES[value]
    p, buf = dev(p0), dev(b0)
    before = hop.skipped_steps()
    hop.sgd_step(p, dev(bad), buf, first_step=False, **tc.SGD_REFERENCE)
    _same(p.cpu(), torch.from_numpy(p0), "parameters after a skipped step")
    _same(buf.cpu(), torch.from_numpy(b0), "momentum after a skipped step")
    assert hop.skipped_steps() == before + 1
    hop.sgd_step(p, dev(g0), buf, first_step=False, **tc.SGD_REFERENCE)              # a clean step afterwards applies
    p2, buf2 = dev(p0), dev(b0)
    hop.sgd_step(p2, dev(g0), buf2, first_step=False, **tc.SGD_REFERENCE)
    assert hop.skipped_steps() == before + 1
    _same(p.cpu(), p2.cpu(), "the clean step after a skipped one")
    _same(buf.cpu(), buf2.cpu(), "the clean step's momentum")
    assert not torch.equal(p.cpu(), torch.from_numpy(p0))


def test_sgd_takes_a_finite_bucket_of_flt_max(hop):
    """"a NaN or Inf" skips; +-FLT_MAX is finite: with grad_scale 2**-126 it is the gradient +-(4 - 2**-22), a normal (here exact) step"""
    n = 5003
    rs = np.random.RandomState(7)
    g0 = rs.choice([-tc.FLT_MAX, 0.0, tc.FLT_MAX], n).astype(np.float32)
    g0[[0, n - 1, n & ~3]] = tc.FLT_MAX
    p, buf = dev(np.zeros(n, np.float32)), dev(np.full(n, np.nan, np.float32))
    before = hop.skipped_steps()
    hop.sgd_step(p, dev(g0), buf, lr=2.0 ** -3, momentum=0.5, weight_decay=0.0, grad_scale=2.0 ** -126, first_step=True)
    assert hop.skipped_steps() == before
    p64, b64 = tc.sgd64(torch.zeros(n, dtype=torch.float64), torch.from_numpy(g0).double(), torch.zeros(n, dtype=torch.float64), 2.0 ** -3, 0.5, 0.0, 2.0 ** -126, True)
    assert float(b64.abs().max()) == 4.0 - 2.0 ** -22
    assert torch.equal(p.cpu().double(), p64) and torch.equal(buf.cpu().double(), b64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# EMA
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", sorted(tc.EMA_DECAYS))
@pytest.mark.parametrize("n", tc.EMA_LENGTHS)
def test_ema_bit_exact(hop, n, decay):
    rs = np.random.RandomState(4000 + n % 997)
    v0, m0 = (rs.standard_normal(n).astype(np.float32) for _ in range(2))
    vf, v = _guarded(v0)
    mf, m = _guarded(m0)
    for _ in range(2):
        hop.ema_update(v, m, tc.EMA_DECAYS[decay])
        v0 = tc.ema32(v0, m0, tc.EMA_DECAYS[decay])
        assert np.array_equal(v.cpu().numpy().view(np.int32), v0.view(np.int32)), "n = %d, decay %s" % (n, decay)
    assert torch.equal(m.cpu(), torch.from_numpy(m0))
    _guards_intact(vf, mf)
