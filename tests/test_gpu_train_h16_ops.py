"""Every kernel of the fp16 training step (csrc/kernels_h16.hip) on its own against float64 torch on the CPU, through the single-operator
entries of csrc/yn_train_h16_ops.inc (fp32 tensors in and out, staged to fp16 where the step stores fp16).  The case tables and the restated
dispatch rules are tests/h16_op_cases.py; tests/test_h16_ops_cases_cpu.py shows without a GPU that they reach every variant.  Each case first
asserts the kernels the profile recorded (in order: forward, dx, dbias, dw, the slot combine), then the values.

Two kinds of case per shape.
  EXACT   every operand is a small integer (an fp16 number).  Asserted per case before comparing: the float64 reference run on the absolute values
          stays below 2**24 (every fp32 sum is then an exact integer in any order: MFMA chains, LDS combines, float atomics, the slot combine) and
          every value a kernel stores as fp16 has |ref| <= 2048 (stored exactly).  Then y, dx (with and without prior contents, the channels outside
          a dx view included), dw, dbias, the forward statistics sums, pooled values, window positions, pool dx, resample and gather results equal
          float64 bit for bit.  The statistics cases use operands in {-1, 0, 1}: sum y^2 is taken in fp32 over a 128-row tile / a workgroup's runs.
  RANDOM  standard-normal data, rounded to fp16 where the device stages it.  Element-wise, with d = 4 * e32 + 4 ulp (f64_bar.bar: e32 = torch fp32
          on the CPU against float64 on the same rounded operands):   fp16-stored outputs  |got - ref64| <= u16(|ref64| + d) / 2 + d   (f64_bar.bar16:
          the one rounding the kernel adds);   fp32 outputs (dw, dbias, dgamma, dbeta, mean, invstd, the sums)  |got - ref64| <= d.
          Two documented exceptions, both arithmetic the kernels state:  hgemm_kernel with accumulate rounds the conv result to fp16 BEFORE adding the
          prior value (its epilogue tile is fp16), so the dx bar of those cases carries that second rounding, u16(|conv| + d) / 2;  hstem_wgrad_kernel
          splits its fp32 patch values into hi + lo * 2**-11 fp16 pairs, 2**-22 relative per product, so its bar carries 2**-22 * sum |terms| (float64).
Activation signs (BatchNorm dy / dgamma / dbeta, the backward statistics sums, the fused stem) follow tests/test_gpu_train_ops.py: elements whose
float64 pre-activation is below 1e-5 in magnitude are left out of dy (at most 0.5 % of a case, asserted) and what they could add to a channel's sums is
added to that channel's bound.  The backward statistics sums are compared on the dx the kernel itself stored (they are taken from those fp16 values).

The fused stem (hstem_apply_pool_kernel, hstem_bwd_kernel<0 / 1>) is compared with the separate kernels (hbn_apply -> hmaxpool_idx; hmaxpool_bwd ->
hcol_reduce<2> + hbn_bwd): pooled values, window positions, mean and invstd are asserted equal bit for bit; dy, dgamma, dbeta of both are compared
against float64.  The two backward forms are NOT bit-equal and cannot be asserted so: they batch their fp32 partial sums over different pixels (four
rows of one lane against four pixels of an 85-pixel walk).  Measured over the ten fused cases: dbeta equal in all 24 channels every time, dgamma
different in its last bits in 3 to 12 of the 24 channels, dy different in 0 to 2 of up to 18 432 elements (one fp16 neighbour).  On normal data two window elements can round to the same
fp16 value, so the float64 arg-max is not the kernel's: the reference routes the pooled gradient by the recorded positions, after asserting that each
recorded position holds a maximum of its window up to twice the element bar and is the first of the window's elements with exactly its float64 value.

Not exact by nature, so random only: BatchNorm (its arithmetic divides) and the backward statistics sums (xhat is no integer).
hdw_run_kernel<0> with NR > 1 is not reached (h16_op_cases.UNREACHED: 33.6 M elements); dw of a depthwise conv, dbias and BatchNorm above 256 padded
channels are refused by the entries (asserted): hdw_wgrad_kernel, hcol_reduce_kernel and the hbn kernels combine at most 32 octet lanes / keep 256
channel constants, which the 1.0x and 0.5x backbones never exceed.  The step had no such limit of its own: yn_train_precision now refuses fp16 for the
1.5x / 2.0x backbones (bf = 352 / 488) with a message (test_fp16_step_refuses_backbones_above_256_padded_channels); they train in fp32.

Measured on an MI355X: the worst (error / bar) of each output family over the random cases, with the case (and for fp32 outputs its error / e32).
Every exact case matched bit for bit.  An fp16-stored output sits just under 1.0 by nature: a correctly rounded value is up to half a spacing away.
  conv y       0.996  dw232g-s2-cap        conv dx      0.996  dws232g-bwd-relu-nr2     pool dx     0.999  pool-9x11-b3      resample  0.999  mode 3, 4<->2
  bn z         0.997  bn-5x14-act1         bn dy        0.996  unit-2000x14-act1        stem pooled 0.996  pool-17x15-b3 act2
  conv dw      0.320  c3-96-96-m399        3.2e-05 / 1.8e-05        conv dbias   0.133  c3-96-96-m1353   8.1e-06 / 7.6e-06
  bn dgamma    0.175  bn-3x116-act2        5.6e-07 / 5.6e-07        bn dbeta     0.083  unit-2000x14-act1   1.9e-06 / 1.9e-06
  bn mean      0.076  bn-500x58-act1       3.3e-09 / 3.3e-09        bn invstd    0.098  bn-1x14-act2     1.7e-05 / 1.3e-05
  stem mean    0.083  pool-9x11-b3         7.4e-09 / 7.4e-09        stem invstd  0.078  pool-16x16-b1    6.5e-08 / 9.0e-08
  sum y        0.047  gs116g-58            2.1e-06 / 3.8e-06        sum y^2      0.142  dws58-fwd        2.4e-04 / 1.9e-04
  sum d        0.273  dws24-bwd-leaky      1.0e-05 / 5.3e-06        sum d xhat   0.142  dws24-bwd-leaky  7.9e-06 / 1.0e-05
  undecided activation signs: at most 1.5e-04 of a case's elements.
One finding, fixed in the kernels: test_bn[1-14-2] (one row, LeakyReLU) returned dy = 2.3e-06 where float64 and fp32 give exactly 0 - 76 times the bar.
hbn_bwd_kernel (and hstem_bwd_kernel<1>) had the product dz * 0.1 contracted into the subtraction of the batch mean of that product, i.e. the unrounded
product minus the rounded one, times gamma * invstd = 316 at zero variance; the product is now formed with contraction off (act_grad2_rounded).

The cases notice.  Tried once with deliberately wrong libraries (arithmetic only, no address changed), 174 tests each:
  all five mistakes at once: 89 fail.  The last row pair of an M slice masked off in hwgrad2_kernel fails dw of every pointwise / dense case that runs hwgrad2,
  exact and random (the hwgrad_kernel cases pw24-58-m1, pw58-58-m7, pw58-24-m7, pw58-58-plane, c3-16-24 rightly pass dw); row 0 counted twice in
  hcol_reduce_kernel<3> fails dbias of every case that asks for it (dw352-s1-w5, dw232g-s2-g66 and the statistics entries do not: they pass); the image's
  last column masked in hdw_run_kernel's partial last run fails y of every stride-1 depthwise case with W % 4 != 0, the statistics cases included
  (dw58-s1-w4, dw232g-s1-w8 and dws96-bwd-none have no partial run, dw352-s1-w5 runs hdw_kernel<1>: they rightly pass); >= for > in hmaxpool_idx_kernel
  fails the window positions of all five test_maxpool cases and "fused against separate" in eight of the ten fused cases (pool-9x11 under LeakyReLU has
  no tied window: it rightly passes); every gemm_statistics, bn, stem, resample, gather and grad_finish case passes.
  without the two mistakes that come first in a conv case's order of assertions: 39 fail.  accumulate ignoring the prior value in hgemm_kernel fails
  dx (accumulate 1) of the four pointwise / dense cases that accumulate (pw116-116-m297, pw96-96-m297, pw58-58-plane, c3-96-96-b2), exact and random;
  the depthwise accumulate cases (other kernels) pass.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import h16_op_cases as hoc
from f64_bar import bar, bar16, ints, normal, u16
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu
AMBIGUOUS = 1e-5


@pytest.fixture(scope="module")
def hop():
    from yolo_nano_amd import capi
    h = capi.Handle(64, 20, arch.MULTI_ANCHOR_SIZE)
    yield h
    h.close()


def _ran(h, fn):
    """fn() under the handle's profile: its result and the kernel symbols its bracketed launches recorded, in order"""
    h.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [r[1] for r in h.profile_records()]
    finally:
        h.profile_enable(False)
    return out, names


def _q(t):
    """fp16 rounding as the device stages it, in float64"""
    return torch.as_tensor(t).to(torch.float16).to(torch.float64)


def _lim(lim):
    return lambda rs, *shape: torch.from_numpy(rs.randint(-lim, lim + 1, size=shape).astype(np.float32))


def _same(got, ref64, what):
    """bit for bit: the float32 result, widened, is the float64 one"""
    got, ref64 = torch.as_tensor(got), torch.as_tensor(ref64)
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    if not torch.equal(got.double(), ref64.double()):
        bad = (got.double() != ref64.double()).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r against %r" % (what, len(bad), got.numel(), i, float(got[i]), float(ref64[i])))


def _exact_sums(v, what):
    assert float(v.abs().max()) + 3.0 < 2 ** 24, (what, float(v.abs().max()))


def _stored(v, what):
    assert float(v.abs().max()) <= 2048.0, (what, float(v.abs().max()))


def _d(ref64, ref32):
    """what f64_bar.bar allows an fp32 result"""
    e32 = float((ref32.double() - ref64.double()).abs().max())
    return 4 * e32 + 4 * float(np.spacing(np.float32(float(ref64.abs().max()))))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _act(t, act):
    return F.relu(t) if act == 1 else (F.leaky_relu(t, 0.1) if act == 2 else t)


# =====================================================================================================================================
# convolutions: forward, input gradient, weight gradient, bias gradient
# =====================================================================================================================================
def _conv_data(case, kind_of_data):
    """fp32 tensors as the entry takes them, and the values the kernels see (float64: rounded to fp16 where the device stages them)"""
    kind, cin, cout, stride, (B, H, W), opt = hoc.CONV_CASES[case]
    g = hoc.conv_geometry(case)
    exact = kind_of_data == "exact"
    gen = _lim(opt.get("lim", 3)) if exact else normal
    rs = np.random.RandomState(211 if exact else 212)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    wshape = {hoc.PW: (cout, cin, 1, 1), hoc.DW: (cout, 1, 3, 3), hoc.C3: (cout, cin, 3, 3)}[kind]
    d = {"x": gen(rs, B, H, W, g["x_ld"]), "w": gen(rs, *wshape), "bias": gen(rs, cout) if opt.get("bias") else None, "dy": gen(rs, B, Ho, Wo, cout),
         "prior": gen(rs, B, H, W, g["x_ld"])}
    seen = {"x": _q(d["x"]), "w": d["w"].double() if kind == hoc.DW else _q(d["w"]),                 # depthwise taps and every bias stay fp32
            "bias": d["bias"].double() if d["bias"] is not None else torch.zeros(cout, dtype=torch.float64), "dy": _q(d["dy"]), "prior": _q(d["prior"])}
    return d, seen


def _conv_ref(case, seen, dtype, absolute=False):
    kind, cin, cout, stride, _, _ = hoc.CONV_CASES[case]
    x_off = hoc.conv_geometry(case)["x_off"]
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    xs = f(_nchw(seen["x"][..., x_off:x_off + cin])).to(dtype).clone().requires_grad_(True)
    w = f(seen["w"]).to(dtype).clone().requires_grad_(True)
    b = f(seen["bias"]).to(dtype).clone().requires_grad_(True)
    y = F.conv2d(xs, w, b, stride=stride, padding=0 if kind == hoc.PW else 1, groups=cin if kind == hoc.DW else 1)
    y.backward(_nchw(f(seen["dy"])).to(dtype))
    return {"y": _nhwc(y.detach()), "dx": _nhwc(xs.grad), "dw": w.grad, "dbias": b.grad}


def _dx_expected(case, seen, ref_dx, accumulate, dtype, absolute=False):
    """the whole dx tensor: the conv's channels written (or added to), every other channel as it was"""
    cin, x_off = hoc.CONV_CASES[case][1], hoc.conv_geometry(case)["x_off"]
    e = (seen["prior"].abs() if absolute else seen["prior"]).to(dtype).clone()
    e[..., x_off:x_off + cin] = e[..., x_off:x_off + cin] + ref_dx if accumulate else ref_dx
    return e


def _conv_run(hop, case, d, accumulate):
    kind, cin, cout, stride, _, opt = hoc.CONV_CASES[case]
    g = hoc.conv_geometry(case)
    want = opt.get("want", ("dx", "dw", "dbias"))
    dx = d["prior"].cuda() if "dx" in want else None
    bias = d["bias"].cuda() if d["bias"] is not None else None
    out, names = _ran(hop, lambda: hop.op_h16_conv2(kind, d["x"].cuda(), d["w"].cuda(), bias, stride=stride, dy=d["dy"].cuda(), gapped=opt.get("gapped", 0),
                                                    x_off=g["x_off"], cin=cin, dx=dx, dx_off=g["x_off"], accumulate=accumulate, partial_cap=g["cap"], want=want))
    assert names == hoc.conv_kernels(case), (names, hoc.conv_kernels(case))
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("case", list(hoc.CONV_CASES))
def test_conv_exact(hop, case):
    """Integer data: y, dx (the whole tensor of a view), dw, dbias equal the float64 results bit for bit."""
    kind, cin, cout, _, _, opt = hoc.CONV_CASES[case]
    d, seen = _conv_data(case, "exact")
    ref, mag = _conv_ref(case, seen, torch.float64), _conv_ref(case, seen, torch.float64, absolute=True)
    for k, v in mag.items():                                 # the exactness claim, part one: every sum of magnitudes stays below 2**24
        _exact_sums(v, k)
    _stored(ref["y"], "y")                                   # part two: what is stored as fp16 is an integer up to 2048
    for accumulate in opt.get("acc", (0,)):
        dxe = _dx_expected(case, seen, ref["dx"], accumulate, torch.float64)
        _exact_sums(_dx_expected(case, seen, mag["dx"], accumulate, torch.float64, absolute=True), "dx")
        _stored(dxe, "dx")
        _stored(ref["dx"], "dx before the prior contents are added")
        got = _conv_run(hop, case, d, accumulate)
        _same(got["y"], ref["y"], "y")
        for k in ("dw", "dbias"):
            if k in got:
                _same(got[k], ref[k], k)
        if "dx" in got:
            _same(got["dx"], dxe, "dx (accumulate %d)" % accumulate)


@pytest.mark.parametrize("case", list(hoc.CONV_CASES))
def test_conv_random(hop, case):
    """Standard-normal data: fp16-stored outputs within u16 / 2 + d of float64, fp32 outputs within d, element by element."""
    kind, cin, cout, _, _, opt = hoc.CONV_CASES[case]
    d, seen = _conv_data(case, "random")
    r64, r32 = _conv_ref(case, seen, torch.float64), _conv_ref(case, seen, torch.float32)
    for accumulate in opt.get("acc", (0,)):
        got = _conv_run(hop, case, d, accumulate)
        tag = "%s acc%d" % (case, accumulate)
        bar16("y", tag, got["y"], r64["y"], r32["y"])
        if "dw" in got:
            bar("dw", tag, got["dw"], r64["dw"], r32["dw"])
        if "dbias" in got:
            bar("dbias", tag, got["dbias"], r64["dbias"], r32["dbias"])
        if "dx" in got:
            slack = None
            if accumulate and kind != hoc.DW:                # hgemm_kernel's epilogue tile is fp16: the conv result is rounded before the prior value is added
                g = hoc.conv_geometry(case)
                slack = torch.zeros_like(seen["prior"])
                slack[..., g["x_off"]:g["x_off"] + cin] = u16(r64["dx"].abs() + _d(r64["dx"], r32["dx"])) / 2
            bar16("dx", tag, got["dx"], _dx_expected(case, seen, r64["dx"], accumulate, torch.float64),
                  _dx_expected(case, seen, r32["dx"], accumulate, torch.float32), slack=slack)


def test_entries_refuse_what_the_kernels_cannot_read(hop):
    """Slices off a 16-byte boundary, odd two-plane tensors, more octet lanes than the reducing kernels combine: an error with a message, not a wrong answer."""
    from yolo_nano_amd import capi
    rs = np.random.RandomState(1)
    x116, w58, dy58 = ints(rs, 1, 4, 4, 116).cuda(), ints(rs, 58, 58, 1, 1).cuda(), ints(rs, 1, 4, 4, 58).cuda()
    refused = lambda fn, word: word in str(pytest.raises(capi.YnError, fn).value)
    assert refused(lambda: hop.op_h16_conv2(hoc.PW, x116, w58, x_off=20, cin=58), "16-byte")                       # a slice that is no plane
    assert refused(lambda: hop.op_h16_conv2(hoc.PW, x116, w58, dy=dy58, x_off=58, cin=58, dx=torch.zeros(1, 4, 4, 100).cuda()), "dx is the whole row")
    assert refused(lambda: hop.op_h16_conv2(hoc.PW, ints(rs, 1, 4, 4, 57).cuda(), ints(rs, 8, 57, 1, 1).cuda(), gapped=True), "even channel count")
    assert refused(lambda: hop.op_h16_conv2(hoc.PW, x116, ints(rs, 58, 116, 1, 1).cuda(), stride=2), "stride")
    x352, w352, dy352 = ints(rs, 1, 4, 4, 352).cuda(), ints(rs, 352, 1, 3, 3).cuda(), ints(rs, 1, 4, 4, 352).cuda()
    assert refused(lambda: hop.op_h16_conv2(hoc.DW, x352, w352, dy=dy352, want=("dw",)), "32 octet lanes")
    assert refused(lambda: hop.op_h16_conv2(hoc.DW, x352, w352, dy=dy352, want=("dbias",)), "32 octet lanes")
    assert refused(lambda: hop.op_h16_conv2(hoc.DW, x352, w352, stat=1), "statistics")
    assert refused(lambda: hop.op_h16_conv2(hoc.PW, x116[..., :58].contiguous(), w58, stat=1), "statistics")
    x58, wd58 = ints(rs, 1, 4, 4, 58).cuda(), ints(rs, 58, 1, 3, 3).cuda()
    below = (x58, torch.zeros(58).cuda(), torch.ones(58).cuda(), torch.ones(58).cuda(), torch.zeros(58).cuda(), 1)
    assert refused(lambda: hop.op_h16_conv2(hoc.DW, x58, wd58, dy=dy58, stat=2, below=below, accumulate=True, want=("dx",)), "complete, dense dx")
    assert refused(lambda: hop.op_h16_conv2(hoc.PW, x58, w58, dy=dy58, partial_cap=64 * 64 - 1), "partial_cap")
    assert refused(lambda: hop.op_h16_maxpool(ints(rs, 1, 4, 4, 12).cuda()), "multiple of 8")
    assert refused(lambda: hop.op_h16_resample(0, ints(rs, 1, 5, 4, 8).cuda(), ints(rs, 1, 2, 2, 8).cuda()), "even")
    assert refused(lambda: hop.op_h16_resample(2, ints(rs, 1, 4, 3, 8).cuda(), out=ints(rs, 1, 2, 1, 8).cuda()), "even")
    src, dst = ints(rs, 3, 128).cuda(), ints(rs, 3, 64).cuda()
    assert refused(lambda: hop.op_h16_gather(src, dst, 58, 64, src_cs=2, src_half=58, src_gap=6, dst_off=1), "destination")
    assert refused(lambda: hop.op_h16_gather(src, dst, 64, 64, src_cs=2, src_half=58, src_gap=6, src_off=3), "source")
    assert refused(lambda: hop.op_h16_bn(ints(rs, 4, 264).cuda(), torch.ones(264).cuda(), torch.zeros(264).cuda()), "256")


def test_fp16_step_refuses_backbones_above_256_padded_channels():
    """The reducing and BatchNorm kernels of the fp16 step serve at most 256 padded channels (what the entries above refuse one kernel at a time): the step
    itself says so when fp16 is selected for the 1.5x / 2.0x backbones (bf = 352 / 488) and keeps serving them in fp32."""
    from yolo_nano_amd import capi
    for backbone, fits in (("0.5x", True), ("1.0x", True), ("1.5x", False), ("2.0x", False)):
        h = capi.Handle(64, 20, arch.MULTI_ANCHOR_SIZE, backbone=backbone)
        try:
            if fits:
                h.train_precision("f16")
            else:
                msg = str(pytest.raises(capi.YnError, lambda: h.train_precision("f16")).value)
                assert "256 padded channels" in msg and "fp32" in msg, msg
            h.train_precision("f32")
        finally:
            h.close()


# =====================================================================================================================================
# the statistics epilogues: forward sums of the stored output, BatchNorm-backward sums of the layer below
# =====================================================================================================================================
def _below_data(rs, B, H, W, C):
    """the layer below: its pre-BN output (fp16 values), the float32 statistics the step would have saved, gamma, beta"""
    yb = 1.5 * normal(rs, B, H, W, C) + 0.3
    ybq = _q(yb).reshape(-1, C)
    mean = ybq.mean(0).float()
    invstd = (1.0 / torch.sqrt(ybq.var(0, unbiased=False) + arch.BN_EPS)).float()
    gamma, beta = 1.0 + 0.1 * normal(rs, C), 0.1 * normal(rs, C)
    return yb, mean, invstd, gamma, beta


def _sums_bwd_check(tag, sums, dx_stored, yb, mean, invstd, gamma, beta, act):
    """sum d and sum d * xhat, d = dx * act'(BN(y_below)), on the dx the kernel stored: float64 against torch fp32, the undecided signs added to the bound"""
    C = yb.shape[-1]

    def ref(dtype):
        y2, dxs = _q(yb).reshape(-1, C).to(dtype), dx_stored.reshape(-1, C).to(dtype)
        xh = (y2 - mean.to(dtype)) * invstd.to(dtype)
        z = xh * gamma.to(dtype) + beta.to(dtype)
        slope = {0: 1.0, 1: 0.0, 2: 0.1}[act]
        dd = dxs * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
        return torch.stack([dd.sum(0), (dd * xh).sum(0)]), z, xh
    r64, z64, xh64 = ref(torch.float64)
    r32, _, _ = ref(torch.float32)
    amb = (z64.abs() < AMBIGUOUS) if act else torch.zeros_like(z64, dtype=torch.bool)
    share = float(amb.double().mean())
    print("RATIO ambiguous %-26s share %.2e" % (tag, share))
    assert share <= 0.005
    step = (1.0 if act == 1 else 0.9) * dx_stored.reshape(-1, C).double().abs() * amb
    slack = torch.stack([step.sum(0), (step * xh64.abs()).sum(0)])
    got = torch.as_tensor(sums)
    bar("sum d", tag, got[0], r64[0], r32[0], slack=slack[0])
    bar("sum d xh", tag, got[1], r64[1], r32[1], slack=slack[1])


@pytest.mark.parametrize("case", list(hoc.DW_STAT_CASES))
def test_depthwise_statistics(hop, case):
    """hdw_run_kernel<1> / <2>: exact on {-1, 0, 1} (forward sums), and on normal data under the bars."""
    C, gapped, (B, H, W), stat, act = hoc.DW_STAT_CASES[case]
    Cp = hoc.chan_map(C, gapped)[2]
    kernel, NR = hoc.hdw_choice(Cp, 1, B, H, W, stat)
    conv = lambda x, w, b, dtype: _nhwc(F.conv2d(_nchw(x).to(dtype), w.to(dtype), b.to(dtype) if b is not None else None, padding=1, groups=C))
    if stat == 1:
        rs = np.random.RandomState(221)
        x, w, b = _lim(1)(rs, B, H, W, C), _lim(1)(rs, C, 1, 3, 3), _lim(1)(rs, C)
        y64 = conv(x, w, b, torch.float64)
        per_group = max(NR, 1) * (256 // (Cp >> 3)) * hoc.DW_R                                # output pixels of one workgroup: its fp32 sums
        assert float((y64 * y64).max()) * per_group < 2 ** 24 and float(y64.abs().max()) <= 2048.0
        out, names = _ran(hop, lambda: hop.op_h16_conv2(hoc.DW, x.cuda(), w.cuda(), b.cuda(), gapped=gapped, stat=1))
        assert names == [kernel], names
        _same(out["y"].cpu(), y64, "y")
        _same(out["sums_fwd"][0], y64.reshape(-1, C).sum(0), "sum y")
        _same(out["sums_fwd"][1], (y64 * y64).reshape(-1, C).sum(0), "sum y^2")
        rs = np.random.RandomState(222)
        x, w, b = normal(rs, B, H, W, C), normal(rs, C, 1, 3, 3), normal(rs, C)
        out, names = _ran(hop, lambda: hop.op_h16_conv2(hoc.DW, x.cuda(), w.cuda(), b.cuda(), gapped=gapped, stat=1))
        assert names == [kernel], names
        bar16("y", case, out["y"].cpu(), conv(_q(x), w, b, torch.float64), conv(_q(x), w, b, torch.float32))
        ys = out["y"].cpu().reshape(-1, C)                                                    # the stored values: what the epilogue summed
        bar("sum y", case, torch.as_tensor(out["sums_fwd"][0]), ys.double().sum(0), ys.sum(0))
        bar("sum y^2", case, torch.as_tensor(out["sums_fwd"][1]), (ys.double() ** 2).sum(0), (ys * ys).sum(0))
        return
    rs = np.random.RandomState(223)
    x, w, dy = normal(rs, B, H, W, C), normal(rs, C, 1, 3, 3), normal(rs, B, H, W, C)
    yb, mean, invstd, gamma, beta = _below_data(rs, B, H, W, C)
    below = (yb.cuda(), mean.cuda(), invstd.cuda(), gamma.cuda(), beta.cuda(), act)
    out, names = _ran(hop, lambda: hop.op_h16_conv2(hoc.DW, x.cuda(), w.cuda(), dy=dy.cuda(), gapped=gapped, stat=2, below=below, want=("dx",)))
    assert names == [hoc.hdw_choice(Cp, 1, B, H, W, 0)[0], kernel], names

    def dxref(dtype):
        xs = _nchw(_q(x)).to(dtype).clone().requires_grad_(True)
        F.conv2d(xs, w.to(dtype), None, padding=1, groups=C).backward(_nchw(_q(dy)).to(dtype))
        return _nhwc(xs.grad)
    dx = out["dx"].cpu()
    bar16("dx", case, dx, dxref(torch.float64), dxref(torch.float32))
    _sums_bwd_check(case, out["sums_bwd"], dx, yb, mean, invstd, gamma, beta, act)


@pytest.mark.parametrize("case", list(hoc.GEMM_STAT_CASES))
def test_gemm_statistics(hop, case):
    """hgemm_kernel<NT, taps, 1> / <NT, taps, 2>: y and the forward sums exact on {-1, 0, 1}; on normal data y, dx and all four sums under the bars."""
    kind, cin, cout, gapped, (B, H, W), act = hoc.GEMM_STAT_CASES[case]
    k = 3 if kind == hoc.C3 else 1
    want = hoc.gemm_stat_kernels(case)
    conv = lambda x, w, dtype: _nhwc(F.conv2d(_nchw(x).to(dtype), w.to(dtype), None, padding=k // 2))
    rs = np.random.RandomState(231)
    x, w = _lim(1)(rs, B, H, W, cin), _lim(1)(rs, cout, cin, k, k)
    y64 = conv(x, w, torch.float64).reshape(-1, cout)
    pad = torch.zeros((-len(y64)) % hoc.GEMM_TILE_ROWS, cout, dtype=torch.float64)
    tiles = torch.cat([y64, pad]).reshape(-1, hoc.GEMM_TILE_ROWS, cout)                      # the fp32 sums are taken per 128-row tile
    assert float((tiles * tiles).sum(1).max()) < 2 ** 24 and float(y64.abs().max()) <= 2048.0
    (y, sf, _, _), names = _ran(hop, lambda: hop.op_h16_gemm_stats(kind, x.cuda(), w.cuda(), gapped))
    assert names == want[:1], names
    _same(y.cpu().reshape(-1, cout), y64, "y")
    _same(sf[0], y64.sum(0), "sum y")
    _same(sf[1], (y64 * y64).sum(0), "sum y^2")
    rs = np.random.RandomState(232)
    x, w, dy = normal(rs, B, H, W, cin), 0.2 * normal(rs, cout, cin, k, k), normal(rs, B, H, W, cout)
    yb, mean, invstd, gamma, beta = _below_data(rs, B, H, W, cin)
    cu = lambda t: t.cuda()
    (y, sf, dx, sb), names = _ran(hop, lambda: hop.op_h16_gemm_stats(kind, cu(x), cu(w), gapped, cu(dy), cu(yb), cu(mean), cu(invstd), cu(gamma), cu(beta), act))
    assert names == want, names
    bar16("y", case, y.cpu(), conv(_q(x), _q(w), torch.float64), conv(_q(x), _q(w), torch.float32))
    ys = y.cpu().reshape(-1, cout)
    bar("sum y", case, torch.as_tensor(sf[0]), ys.double().sum(0), ys.sum(0))
    bar("sum y^2", case, torch.as_tensor(sf[1]), (ys.double() ** 2).sum(0), (ys * ys).sum(0))

    def dxref(dtype):
        xs = _nchw(_q(x)).to(dtype).clone().requires_grad_(True)
        F.conv2d(xs, _q(w).to(dtype), None, padding=k // 2).backward(_nchw(_q(dy)).to(dtype))
        return _nhwc(xs.grad)
    bar16("dx", case, dx.cpu(), dxref(torch.float64), dxref(torch.float32))
    _sums_bwd_check(case, sb, dx.cpu(), yb, mean, invstd, gamma, beta, act)


# =====================================================================================================================================
# stem conv and its weight gradient
# =====================================================================================================================================
def _stem_ref(x, w, b, dy, dtype, absolute=False):
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    wv = f(w).to(dtype).clone().requires_grad_(True)
    y = F.conv2d(f(x).to(dtype), wv, f(b).to(dtype), stride=2, padding=1)
    y.backward(_nchw(f(dy)).to(dtype))
    return _nhwc(y.detach()), wv.grad


@pytest.mark.parametrize("case", list(hoc.STEM_CASES))
def test_stem(hop, case):
    """hstem_kernel and hstem_wgrad_kernel: the input and the weights stay fp32, y and dy are fp16."""
    B, H, W = hoc.STEM_CASES[case]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rs = np.random.RandomState(241)
    x, w, b, dy = ints(rs, B, 3, H, W), ints(rs, 24, 3, 3, 3), ints(rs, 24), ints(rs, B, Ho, Wo, 24)
    y64, dw64 = _stem_ref(x, w, b, dy, torch.float64)
    for v in _stem_ref(x, w, b, dy, torch.float64, absolute=True):
        _exact_sums(v, case)
    _stored(y64, "y")
    (y, dw), names = _ran(hop, lambda: hop.op_h16_stem(x.cuda(), w.cuda(), b.cuda(), dy.cuda()))
    assert names == ["hstem_kernel", "hstem_wgrad_kernel", "hgrad_finish_kernel"], names
    _same(y.cpu(), y64, "y")
    _same(dw.cpu(), dw64, "dw")
    rs = np.random.RandomState(242)
    x, w, b, dy = normal(rs, B, 3, H, W), normal(rs, 24, 3, 3, 3), normal(rs, 24), normal(rs, B, Ho, Wo, 24)
    (y, dw), _ = _ran(hop, lambda: hop.op_h16_stem(x.cuda(), w.cuda(), b.cuda(), dy.cuda()))
    r64, r32 = _stem_ref(x, w, b, _q(dy), torch.float64), _stem_ref(x, w, b, _q(dy), torch.float32)
    bar16("y", case, y.cpu(), r64[0], r32[0])
    terms = _stem_ref(x, w, b, _q(dy), torch.float64, absolute=True)[1]                       # sum |dy| |patch| per weight: the hi / lo split loses 2**-22 of each product
    bar("dw", case, dw.cpu(), r64[1], r32[1], slack=2.0 ** -22 * terms)


# =====================================================================================================================================
# max pool with the recorded window position; the fused stem BatchNorm + activation + max pool
# =====================================================================================================================================
def _window_position(idx64, H, W):
    """torch's flat input index of the maximum -> the position ky * 3 + kx inside its 3x3 stride-2 pad-1 window"""
    B, C, Ho, Wo = idx64.shape
    iy, ix = idx64 // W, idx64 % W
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    return _nhwc((iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))).to(torch.uint8)


def _flat_index(pos, H, W):
    """the inverse: window positions [B,Ho,Wo,C] -> flat input indices [B,C,Ho,Wo]"""
    p = _nchw(pos.long())
    _, _, Ho, Wo = p.shape
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    return (2 * oy - 1 + p // 3) * W + (2 * ox - 1 + p % 3)


@pytest.mark.parametrize("case", list(hoc.POOL_CASES))
def test_maxpool(hop, case):
    """hmaxpool_idx_kernel / hmaxpool_bwd_kernel on post-ReLU integers (ties are the common case: the first maximum in window order wins, as torch's) bit for
    bit, and on normal data: values and positions still bit for bit (a maximum of fp16 numbers), dx under the fp16 bar."""
    B, H, W = hoc.POOL_CASES[case]
    C, Ho, Wo = 24, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for kind_of_data in ("exact", "random"):
        rs = np.random.RandomState(251 if kind_of_data == "exact" else 252)
        if kind_of_data == "exact":
            x, dy = ints(rs, B, H, W, C).clamp_min(0.0), ints(rs, B, Ho, Wo, C)
            assert 0.35 < float((x == 0).double().mean()) < 0.75
        else:
            x, dy = normal(rs, B, H, W, C), normal(rs, B, Ho, Wo, C)
        xn = _nchw(_q(x)).clone().requires_grad_(True)
        y64, idx64 = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
        y64.backward(_nchw(_q(dy)))
        (y, idx, dx), names = _ran(hop, lambda: hop.op_h16_maxpool(x.cuda(), dy.cuda()))
        assert names == ["hmaxpool_idx_kernel", "hmaxpool_bwd_kernel"], names
        _same(y.cpu(), _nhwc(y64.detach()), "y")
        assert torch.equal(idx.cpu(), _window_position(idx64, H, W)), "window positions"
        if kind_of_data == "exact":
            _stored(_nhwc(xn.grad), "dx")                                                     # at most four windows add into a pixel
            _same(dx.cpu(), _nhwc(xn.grad), "dx")
        else:
            x32 = _nchw(_q(x)).float().clone().requires_grad_(True)
            F.max_pool2d(x32, 3, 2, 1).backward(_nchw(_q(dy)).float())
            bar16("pool dx", case, dx.cpu(), _nhwc(xn.grad), _nhwc(x32.grad))


def _bn_ref(yq, dzq, gamma, beta, act, dtype):
    """train-mode BatchNorm + activation and its backward over [M, C] in `dtype`"""
    y = yq.to(dtype).clone().requires_grad_(True)
    g, b = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    pre, mean, invstd = torch.native_batch_norm(y, g, b, None, None, True, 0.1, arch.BN_EPS)
    z = _act(pre, act)
    out = {"pre": pre.detach(), "z": z.detach(), "mean": mean.detach(), "invstd": invstd.detach()}
    if dzq is not None:
        z.backward(dzq.to(dtype))
        out.update(dy=y.grad, dgamma=g.grad, dbeta=b.grad)
    return out


def _bn_backward_check(tag, got, yq, dzq, gamma, act, r64, r32):
    """dy (fp16) / dgamma / dbeta (fp32) against float64, the undecided activation signs as tests/test_gpu_train_ops.py treats them"""
    M = yq.shape[0]
    amb = (r64["pre"].abs() < AMBIGUOUS) if act else torch.zeros_like(r64["pre"], dtype=torch.bool)
    share = float(amb.double().mean())
    print("RATIO ambiguous %-26s share %.2e" % (tag, share))
    assert share <= 0.005
    step = (1.0 if act == 1 else 0.9) * dzq.abs() * amb                                       # |dz| * |act'(+) - act'(-)| per undecided element
    xhat = (yq - r64["mean"]) * r64["invstd"]
    s_beta, s_gamma = step.sum(0), (step * xhat.abs()).sum(0)
    worst = {"dbeta": bar("dbeta", tag, got["dbeta"], r64["dbeta"], r32["dbeta"], slack=s_beta),
             "dgamma": bar("dgamma", tag, got["dgamma"], r64["dgamma"], r32["dgamma"], slack=s_gamma)}
    k = (gamma.double() * r64["invstd"]).abs()
    clean = ~amb.any(0)                                                                       # e32 of dy from the channels no undecided element touches
    worst["dy"] = bar16("dy", tag, got["dy"], r64["dy"], torch.where(clean[None, :], r32["dy"].double(), r64["dy"]),
                        slack=k[None, :] * (s_beta[None, :] + xhat.abs() * s_gamma[None, :]) / M, keep=~amb)
    return worst


@pytest.mark.parametrize("case", list(hoc.POOL_CASES))
@pytest.mark.parametrize("act", [1, 2])
def test_fused_stem_equals_the_separate_kernels_and_float64(hop, case, act):
    B, H, W = hoc.POOL_CASES[case]
    C, Ho, Wo = 24, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rs = np.random.RandomState(261 + act)
    y, g1 = normal(rs, B, H, W, C), normal(rs, B, Ho, Wo, C)
    gamma, beta = 1.0 + 0.1 * normal(rs, C), 0.1 * normal(rs, C)
    fused, names = _ran(hop, lambda: hop.op_h16_stem_pool(y.cuda(), gamma.cuda(), beta.cuda(), act, g1.cuda()))
    assert names == ["hcol_reduce_kernel<0>", "hstem_apply_pool_kernel", "hstem_bwd_kernel<0>+hstem_bwd_kernel<1>"], names
    fused = {k: v.cpu() for k, v in fused.items()}
    # ---- the separate launches: BatchNorm apply -> pool; pool backward -> BatchNorm backward
    y2 = y.reshape(-1, C).cuda()
    (z, _, _, _, smean, sinvstd), n1 = _ran(hop, lambda: hop.op_h16_bn2(y2, gamma.cuda(), beta.cuda(), act))
    (p, pidx, dz), n2 = _ran(hop, lambda: hop.op_h16_maxpool(z.reshape(B, H, W, C), g1.cuda()))
    (_, dy, dg, db), n3 = _ran(hop, lambda: hop.op_h16_bn(y2, gamma.cuda(), beta.cuda(), act, dz.reshape(-1, C)))
    assert n1 == ["hcol_reduce_kernel<0>", "hbn_apply_kernel"] and n2 == ["hmaxpool_idx_kernel", "hmaxpool_bwd_kernel"] and \
        n3 == ["hcol_reduce_kernel<0>", "hbn_apply_kernel", "hcol_reduce_kernel<2>+hbn_bwd_kernel"], (n1, n2, n3)
    _same(fused["out"], p.cpu(), "pooled values: fused against separate")
    assert torch.equal(fused["idx"], pidx.cpu()), "window positions: fused against separate"
    _same(fused["mean"], smean.cpu(), "mean: fused against separate")
    _same(fused["invstd"], sinvstd.cpu(), "invstd: fused against separate")
    print("RATIO fused-vs-separate %-14s act%d elements that differ: dy %d of %d, dgamma %d, dbeta %d of %d" % (
        case, act, int((fused["dy"].reshape(-1, C) != dy.cpu()).sum()), dy.numel(), int((fused["dgamma"] != dg.cpu()).sum()), int((fused["dbeta"] != db.cpu()).sum()), C))
    # ---- float64
    yq, M = _q(y).reshape(-1, C), B * H * W
    f64, f32 = _bn_ref(yq, None, gamma, beta, act, torch.float64), _bn_ref(yq, None, gamma, beta, act, torch.float32)
    bar("mean", case, fused["mean"], f64["mean"], f32["mean"])
    bar("invstd", case, fused["invstd"], f64["invstd"], f32["invstd"])
    z64, z32 = _nchw(f64["z"].reshape(B, H, W, C)), _nchw(f32["z"].reshape(B, H, W, C))
    p64, p32 = _nhwc(F.max_pool2d(z64, 3, 2, 1)), _nhwc(F.max_pool2d(z32, 3, 2, 1))
    bar16("pooled", "%s act%d" % (case, act), fused["out"], p64, p32)
    # the recorded positions: inside the image, holding a maximum of the window up to twice the element bar, the first of their exact value
    flat = _flat_index(fused["idx"], H, W)
    iy, ix = _nchw(fused["idx"].long()) // 3 + 2 * torch.arange(Ho).view(1, 1, Ho, 1) - 1, _nchw(fused["idx"].long()) % 3 + 2 * torch.arange(Wo).view(1, 1, 1, Wo) - 1
    assert bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).all())
    chosen = z64.reshape(B, C, H * W).gather(2, flat.reshape(B, C, -1)).reshape(B, C, Ho, Wo)
    allowed = 2 * (u16(_nchw(p64).abs() + _d(p64, p32)) / 2 + _d(p64, p32))
    assert bool((_nchw(p64) - chosen <= allowed).all()), float((_nchw(p64) - chosen - allowed).max())
    win = F.unfold(F.pad(z64, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(B, C, 9, Ho, Wo)
    first = (win == chosen.unsqueeze(2)).double().argmax(2)
    assert torch.equal(first, _nchw(fused["idx"].long())), "the first of equal window elements wins"
    # the pooled gradient routed by those positions, rounded to fp16 where the kernels form the stored gradient of the full-resolution tensor
    dz64 = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, flat.reshape(B, C, -1), _nchw(_q(g1)).reshape(B, C, -1))
    dzq = _q(_nhwc(dz64.reshape(B, C, H, W)).reshape(-1, C))
    _same(dz.cpu().reshape(-1, C), dzq, "the separate pool backward is that gradient")
    r64, r32 = _bn_ref(yq, dzq, gamma, beta, act, torch.float64), _bn_ref(yq, dzq, gamma, beta, act, torch.float32)
    for tag, got in (("fused", {"dy": fused["dy"].reshape(-1, C), "dgamma": fused["dgamma"], "dbeta": fused["dbeta"]}),
                     ("separate", {"dy": dy.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()})):
        _bn_backward_check("%s act%d %s" % (case, act, tag), got, yq, dzq, gamma, act, r64, r32)


# =====================================================================================================================================
# BatchNorm (train mode) + activation, plain and as the last layer of a ShuffleV2 unit
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _bn_problem(M, C, act, seed):
    rs = np.random.RandomState(seed)
    d = {"y": normal(rs, M, C), "gamma": 1.0 + 0.1 * normal(rs, C), "beta": 0.1 * normal(rs, C), "dz": normal(rs, M, C)}
    yq, dzq = _q(d["y"]), _q(d["dz"])
    return d, yq, dzq, _bn_ref(yq, dzq, d["gamma"], d["beta"], act, torch.float64), _bn_ref(yq, dzq, d["gamma"], d["beta"], act, torch.float32)


@pytest.mark.parametrize("M,C,act", hoc.BN_CASES)
def test_bn(hop, M, C, act):
    """hcol_reduce_kernel<0>, hbn_apply_kernel, hcol_reduce_kernel<2>, hbn_bwd_kernel: element-wise, where tests/test_gpu_train_h16.py compares norms."""
    d, yq, dzq, r64, r32 = _bn_problem(M, C, act, 271)
    tag = "bn-%dx%d-act%d" % (M, C, act)
    (z, dy, dg, db, mean, invstd), names = _ran(hop, lambda: hop.op_h16_bn2(d["y"].cuda(), d["gamma"].cuda(), d["beta"].cuda(), act, d["dz"].cuda()))
    assert names == ["hcol_reduce_kernel<0>", "hbn_apply_kernel", "hcol_reduce_kernel<2>+hbn_bwd_kernel"], names
    bar("mean", tag, mean.cpu(), r64["mean"], r32["mean"])
    bar("invstd", tag, invstd.cpu(), r64["invstd"], r32["invstd"])
    bar16("z", tag, z.cpu(), r64["z"], r32["z"])
    _bn_backward_check(tag, {"dy": dy.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}, yq, dzq, d["gamma"], act, r64, r32)


@pytest.mark.parametrize("M,C,act", hoc.BN_UNIT_CASES)
def test_bn_as_the_last_layer_of_a_unit(hop, M, C, act):
    """The unit form: the pass-through half and the even half of the gradient are exact copies of fp16 values; z, dy, dgamma, dbeta under the bars."""
    d, yq, dzq, r64, r32 = _bn_problem(M, C, act, 272)
    tag = "unit-%dx%d-act%d" % (M, C, act)
    rs = np.random.RandomState(273)
    pas, dev = normal(rs, M, C), normal(rs, M, C)
    dunit = torch.stack([dev, d["dz"]], 2).reshape(M, 2 * C)                                  # dunit[:, 2c] = dev, dunit[:, 2c + 1] = dz
    (unit, dy, deven, dg, db), names = _ran(hop, lambda: hop.op_h16_bn_unit(d["y"].cuda(), pas.cuda(), d["gamma"].cuda(), d["beta"].cuda(), act, dunit.cuda()))
    assert names == ["hcol_reduce_kernel<0>", "hbn_apply_kernel", "hcol_reduce_kernel<2>+hbn_bwd_kernel"], names
    unit = unit.cpu()
    _same(unit[:, 0::2], _q(pas), "pass-through half of the unit output")
    _same(deven.cpu(), _q(dev), "even channels of the unit gradient")
    bar16("z", tag, unit[:, 1::2], r64["z"], r32["z"])
    _bn_backward_check(tag, {"dy": dy.cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu()}, yq, dzq, d["gamma"], act, r64, r32)


# =====================================================================================================================================
# FPN / PAN adds, channel gathers, the end of a backward pass
# =====================================================================================================================================
def _resample_ref(mode, a, b, prior, dtype):
    n = lambda t: _nchw(t).to(dtype)
    if mode == 0:
        return _nhwc(n(a) + F.interpolate(n(b), scale_factor=2, mode="nearest"))
    if mode == 1:
        return _nhwc(n(a) + F.interpolate(n(b), scale_factor=0.5, mode="nearest"))
    B, H, W, C = a.shape
    src = torch.zeros((B, C, H // 2, W // 2) if mode == 2 else (B, C, 2 * H, 2 * W), dtype=dtype, requires_grad=True)
    F.interpolate(src, scale_factor=2 if mode == 2 else 0.5, mode="nearest").backward(n(a))
    return prior.to(dtype) + _nhwc(src.grad)


@pytest.mark.parametrize("gen", ["ints", "normal"])
@pytest.mark.parametrize("mode", hoc.RESAMPLE_MODES)
@pytest.mark.parametrize("hi,lo", hoc.RESAMPLE_SIZES)
def test_resample(hop, hi, lo, mode, gen):
    """hresample_kernel: out = a + up2(b), out = a + down(b) and their accumulating backwards (non-zero prior contents) against F.interpolate + autograd."""
    B, C = 2, 96
    rs = np.random.RandomState(281 + mode)
    g = ints if gen == "ints" else normal
    big, small = (hi, hi + 2), (lo, lo + 1)                                                   # (H, W) of the two maps, W != H
    (ha, wa), (hb, wb) = (big, small) if mode in (0, 2) else (small, big)
    a, b, prior = g(rs, B, ha, wa, C), g(rs, B, hb, wb, C), g(rs, B, hb, wb, C)
    out, names = _ran(hop, lambda: hop.op_h16_resample(mode, a.cuda(), b.cuda() if mode <= 1 else None, out=prior.cuda() if mode >= 2 else None))
    assert names == ["hresample_kernel"], names
    r64 = _resample_ref(mode, _q(a), _q(b), _q(prior), torch.float64)
    assert out.shape == r64.shape
    if gen == "ints":
        _stored(r64, "out")
        _same(out.cpu(), r64, "mode %d" % mode)
    else:
        bar16("resample", "mode%d %d<->%d" % (mode, hi, lo), out.cpu(), r64, _resample_ref(mode, _q(a), _q(b), _q(prior), torch.float32))


@pytest.mark.parametrize("case", list(hoc.GATHER_CASES))
def test_gather(hop, case):
    """hgather_kernel with the maps of the step's three uses: the mapped channels are copied, the pads of the destination's first npad channels zeroed,
    everything else in the destination row (the second plane of a unit gradient) is left as it was."""
    use, bf, M = hoc.GATHER_CASES[case]
    a = hoc.gather_args(use, bf)
    rs = np.random.RandomState(291)
    src = ints(rs, M, a["src_ld"]) + 10.0                                                     # no zeros, the source's pads included: a wrong channel shows
    dst = torch.full((M, a["dst_ld"]), 77.0)
    exp = dst.clone()
    phys = lambda l, half, gap: l + (gap if l >= half else 0)
    for j in range(a["npad"]):
        dp = phys(a["dst_off"] + j * a["dst_cs"], a["dst_half"], a["dst_gap"])
        exp[:, dp] = src[:, phys(a["src_off"] + j * a["src_cs"], a["src_half"], a["src_gap"])] if j < a["n"] else 0.0
    kw = {k: v for k, v in a.items() if k not in ("src_ld", "dst_ld", "n", "npad")}
    out, names = _ran(hop, lambda: hop.op_h16_gather(src.cuda(), dst.cuda(), a["n"], a["npad"], **kw))
    assert names == ["hgather_kernel"], names
    _same(out.cpu(), exp, case)
    assert int((exp == 77.0).sum()) == M * (a["dst_ld"] - a["npad"]) and int((exp == 0.0).sum()) == M * (a["npad"] - a["n"])


def _state(S, clean=0.0, flag=0, pending=0.0):
    st = np.array([S, 1.0 / S, clean, 0.0, pending], np.float32)
    st.view(np.uint32)[3] = flag
    return st


def _flag(st):
    return int(st.view(np.uint32)[3])


@pytest.mark.parametrize("n", hoc.FINISH_SIZES)
def test_grad_finish_and_scale_update(hop, n):
    """hgrad_finish_kernel: g = (g + the eight slot copies) / S exactly on integers with S a power of two, the overflow flag for one Inf / NaN anywhere;
    hscale_update_kernel: halve on overflow (floor 1), count clean steps, double after the 2000th (cap 65536), from the local or the bucket-wide flag."""
    rs = np.random.RandomState(301)
    g0, slots = ints(rs, n), ints(rs, hoc.GRAD_SLOTS, n)
    exp = (g0.double() + slots.double().sum(0)) / 4.0
    g = g0.cuda()
    st, names = _ran(hop, lambda: hop.op_h16_grad_finish(g, slots.cuda(), _state(4.0, clean=5.0)))
    assert names == ["hgrad_finish_kernel"], names
    _same(g.cpu(), exp, "g")
    assert (float(st[0]), float(st[1]), float(st[2]), _flag(st), float(st[4])) == (4.0, 0.25, 5.0, 0, 1.0)          # untouched, and pending
    for update, gflag in ((1, 0), (2, 0)):                                                    # a clean step settles: counter + 1
        g = g0.cuda()
        st, names = _ran(hop, lambda: hop.op_h16_grad_finish(g, slots.cuda(), _state(4.0, clean=5.0), update, gflag))
        assert names == ["hgrad_finish_kernel", "hscale_update_kernel"], names
        _same(g.cpu(), exp, "g")
        assert (float(st[0]), float(st[1]), float(st[2]), _flag(st), float(st[4])) == (4.0, 0.25, 6.0, 0, 0.0)
    for bad in (float("inf"), float("nan")):
        for pos in sorted({0, n // 2, n - 1}):
            gb = g0.clone()
            gb[pos] = bad
            st = hop.op_h16_grad_finish(gb.cuda(), slots.cuda(), _state(4.0, clean=5.0))
            assert _flag(st) == 1 and float(st[4]) == 1.0 and float(st[0]) == 4.0, (bad, pos)                      # raised, pending, the scale not yet moved
            st = hop.op_h16_grad_finish(gb.cuda(), slots.cuda(), _state(4.0, clean=5.0), 1)
            assert (float(st[0]), float(st[1]), float(st[2]), _flag(st), float(st[4])) == (2.0, 0.5, 0.0, 0, 0.0), (bad, pos)
            sb = slots.clone()
            sb[hoc.GRAD_SLOTS - 1, pos] = bad                                                                       # in a slot copy instead
            st = hop.op_h16_grad_finish(g0.cuda(), sb.cuda(), _state(1.0, clean=5.0), 1)
            assert (float(st[0]), float(st[1]), float(st[2]), _flag(st), float(st[4])) == (1.0, 1.0, 0.0, 0, 0.0), (bad, pos)      # the floor
    if n == hoc.FINISH_SIZES[0]:
        mk = lambda **kw: hop.op_h16_grad_finish(g0.cuda(), slots.cuda(), _state(**kw["state"]), kw["update"], kw.get("gflag", 0))
        st = mk(state=dict(S=4.0, clean=1999.0), update=1)                                    # the 2000th clean step doubles
        assert (float(st[0]), float(st[1]), float(st[2])) == (8.0, 0.125, 0.0)
        st = mk(state=dict(S=4.0, clean=1998.0), update=1)
        assert (float(st[0]), float(st[2])) == (4.0, 1999.0)
        st = mk(state=dict(S=65536.0, clean=1999.0), update=2)                                # the cap
        assert (float(st[0]), float(st[2])) == (65536.0, 0.0)
        st = mk(state=dict(S=4.0, clean=7.0), update=2, gflag=1)                              # another rank overflowed: the bucket-wide flag decides
        assert (float(st[0]), float(st[2]), _flag(st), float(st[4])) == (2.0, 0.0, 0, 0.0)
        gb = g0.clone()
        gb[0] = float("inf")
        st = hop.op_h16_grad_finish(gb.cuda(), slots.cuda(), _state(4.0, clean=7.0), 2, 0)    # ... and only it: a local flag is cleared, the step counts as clean
        assert (float(st[0]), float(st[2]), _flag(st), float(st[4])) == (4.0, 8.0, 0, 0.0)
        st = hop.op_h16_grad_finish(g0.cuda(), slots.cuda(), _state(4.0, clean=7.0, flag=1), 1)      # a flag raised earlier in the pass (the loss kernel's) survives the combine
        assert (float(st[0]), float(st[2]), _flag(st)) == (2.0, 0.0, 0)
