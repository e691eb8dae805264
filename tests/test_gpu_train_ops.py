"""Every kernel of the fp32 training step on its own against float64 torch on the CPU (yn_op_f32_conv / _bn / _maxpool / _resample: the
step's own per-layer launch code, csrc/yn_train.inc, on one synthetic layer).

Two kinds of case per shape.
  EXACT   x, w, dy, bias (and the prior contents of an accumulated dx) are integers in {-3..3}: every product and every partial sum is an
          integer below 2**24 (checked per case: the float64 reference is run on the absolute values), so fp32 arithmetic is exact in ANY
          summation order - MFMA chains, LDS combines, float atomics into the gradient slots, double accumulators - and the result must
          equal the float64 one bit for bit.  A dropped row, a clamped row counted twice or a wrong border tap changes an integer.
          The step's forward / input-gradient GEMMs run on the f32 MFMA (the training packs carry no split-f16 operands), so they are exact too.
  RANDOM  standard-normal data, element-wise |kernel - float64| <= 4 * e32 + 4 ulp, e32 = max |torch fp32 CPU - float64| of the same
          output, ulp = spacing of the output's largest float32 magnitude (the error of a sum scales with its terms, not with the element).
BatchNorm is random only (its arithmetic divides).  Where an activation's sign decides (dy, dgamma, dbeta of a ReLU / LeakyReLU layer) the
elements whose float64 pre-activation is below 1e-5 in magnitude are undetermined in fp32: they are left out of the dy comparison (at most
0.5 % of the elements, asserted), and what they could add to a channel's dgamma / dbeta - and through the two means to that channel's dy -
is added to that channel's bound, nothing else is.

Which exact case reaches which kernel of csrc/kernels_bwd.hip (template variant in brackets):
  wgrad_kernel          [2,2 pw] pw24-58-m1, pw58-58-m7, pw58-58-off-acc      [2,4 pw] pw116-116-m257, pw232-232-m999, pw116-116-cap (slices clipped 4 -> 2)
                        [3,3 pw] pw464-96, pw96-255-head                       [2,2 dense] c3-6-14, c3-6-14-strip   [2,4 dense] c3-8-16, c3-8-16-m1
                        [3,3 dense] c3-96-96 (one slice), c3-96-96-m297 (two slices, the cut inside an image), c3-96-96-b3
                        wgrad_reduce_kernel in all of them; ragged last slice: m257 (136 + 121 rows), m999 (3 x 256 + 231), m297 (152 + 145)
                        the 1.5x / 2.0x widths (no tile beyond these three): [2,4 pw] pw122-122-off-acc (one slice, a channel slice of the unit tensor),
                        pw244-244-m297, pw488-488-m297 (two slices)   [3,3 pw] pw352-352-m297 (two slices), pw976-96, pw704-96 (31 / 22 k-tiles for 33 / 24)
  dw_wgrad_kernel       [1,vec] dw*-s1 (W = 7, 8, 9, 13: below, at and above one run of 8)     [2,vec] dw*-s2 (W = 6, 10, 12: Wo = 3, 5, 6 around the run of 4;
                        odd H / W in dw232-s2-odd, dw58-s2-odd, dw488-s2-odd), rows_sum_kernel; dw122- / dw244- / dw352- / dw488-*: the wide branch widths on 64,
                        128 and 256 channel-pair lanes (at 256 a block holds ONE row-lane: the LDS combine adds nothing); dw232-s1-cap clips the block count (14 -> 8).  The non-vector variants [*,false] need an
                        odd channel offset or count: no tensor of the network has one, the forward kernel cannot read one, the entry refuses it (asserted).
  dw_dgrad_s2_kernel    dw*-s2, accumulate 0 and 1        stem_wgrad_kernel  stem-* (Wo = 15, 16, 17, 24: a ragged and a full last 16-pixel step; stem-cap: more rows than 4 x blocks)
  col_reduce_kernel     [3: plain column sum] dbias of every conv case (pw96-255-head: odd C on a padded row, 10 blocks over the 8 slots)
                        [0 / 2: BatchNorm sums] the BatchNorm cases below (random data)
  maxpool_idx_kernel, maxpool_bwd_kernel    test_maxpool_exact        resample_kernel (modes 0-3)    test_resample
  strided_copy_kernel   the accumulate route of every stride-1 dx (tmp, then += into the view) and the unit form's even channels (test_bn, exact part)
  pack_bwd_kernel       [0] pw dx  [1] depthwise stride-1 dx  [2] dense dx          grad_combine_kernel  dw / dbias of every conv case
  bn_apply_kernel       [1 dense] plain   [2 shuffle] unit form          bn_bwd_kernel / col_reduce_kernel<2>  [vec] plain dense dz
                        [non-vec] the unit form (dz_cs = 2), bn-dzoff (odd dz_off).  bn-*x122 / x176 / x244 / x352 / x488: the wide widths, plain and unit form;
                        col_reduce_kernel's LDS combine with 4, 2, 2, 1 and 1 row-lanes per block (1.0x: 2 at C = 232).  bn_apply_kernel<0> (scalar stores) and the odd-C lanes of these kernels
                        serve no layer of the network; they read the pair (c, c + 1) of a dense row, one float past an odd-C tensor's end, so the entry refuses odd C.
Not reached at these sizes: launch_dw's long-run variants (R = 4 / 8) need more than 261888 threads, i.e. tensors of millions of elements; they are forward
kernels of kernels_conv.hip, and tests/test_gpu_infer_ops.py checks each of them on its own against float64 (the inference parity tests run them only inside
whole networks).

Measured on an MI355X: the worst (kernel error) / (4 * e32 + 4 ulp) over the random cases of each output, with that case's kernel error and e32.
Every exact case matched bit for bit.
  conv y      0.25  pw464-96         7.6e-05 / 6.8e-05        conv dx     0.29  pw58-58-m7       6.2e-06 / 3.5e-06
  conv dw     0.23  c3-6-14-strip    2.9e-06 / 1.2e-06        conv dbias  0.14  dw232-s1-w13     4.8e-06 / 4.8e-06
  bn mean     0.07  bn-64x24-unit    6.5e-09 / 9.6e-09        bn invstd   0.08  bn-7x58-relu     1.2e-07 / 1.3e-07
  bn z        0.16  bn-dzoff         3.5e-07 / 3.2e-07        bn running  0.15  bn-7x58-relu     mean 2.2e-08 / 2.2e-08, var 1.3e-07 / 1.1e-07
  bn dy       0.19  bn-64x24-relu    4.9e-07 / 3.9e-07        bn dgamma   0.16  bn-333x116-unit  3.6e-06 / 3.6e-06
  bn dbeta    0.07  bn-64x24-relu    4.1e-07 / 4.3e-07        resample    0.13  mode 2, 4<->2    5.4e-07 / 5.4e-07
  undecided activation signs: at most 2.6e-05 of a case's elements (bn-333x116), none in six of the ten cases.
  With the 1.5x / 2.0x widths added, five of the worst cases moved to them, none above 0.20: conv dbias 0.17 dw244-s1-w7 (2.8e-06 / 2.3e-06), bn mean 0.08, bn z 0.17 and
  bn dy 0.20 bn-65x352-leaky (1.5e-08 / 1.7e-08, 4.0e-07 / 3.7e-07, 7.6e-07 / 4.7e-07), bn dbeta 0.08 bn-65x352-unit (9.4e-07 / 9.7e-07); undecided signs at most 4.4e-05
  (bn-65x352).  Every exact case at the wide widths matched bit for bit.
The cases notice what the whole-step tests cannot.  Tried once with deliberately wrong libraries: the last row pair of an M slice masked off in
wgrad_kernel together with a bottom-border tap of the dense im2col reading the next image failed every pointwise and dense case, exact and random; the last
pixel of a partial run dropped in dw_wgrad_kernel failed every depthwise case that has a partial run (W = 8 has none and rightly passed); one row counted
twice in col_reduce_kernel failed every BatchNorm case whose doubled row lies in the mutated loop (its tail loop: bn-7x58; its unrolled loop: all others).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from f64_bar import bar as _bar, ints as _ints, normal as _normal
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hop():
    from yolo_nano_amd import capi
    h = capi.Handle(64, 20, arch.MULTI_ANCHOR_SIZE)
    yield h
    h.close()


# =====================================================================================================================================
# convolutions: forward, input gradient, weight gradient, bias gradient
# =====================================================================================================================================
PW, DW, C3, STEM = 0, 1, 2, 3
# id: kind, Cin, Cout, stride, (B, H, W), options: x_ld / x_off (channel slice of a wider tensor), y_ld (padded head row), cap (partial_cap as a
# multiple of one copy of dw), acc (values of `accumulate` to run)
CONV_CASES = {
    # pointwise: the network's layers; M = 1, 7, 257, 999 (slices 1, 1, 2, 4); two / three images with H != W
    "pw24-58-m1": (PW, 24, 58, 1, (1, 1, 1), {}),
    "pw58-58-m7": (PW, 58, 58, 1, (1, 1, 7), {}),
    "pw116-116-m257": (PW, 116, 116, 1, (1, 257, 1), {}),
    "pw232-232-m999": (PW, 232, 232, 1, (3, 9, 37), {}),
    "pw464-96": (PW, 464, 96, 1, (2, 9, 7), {"acc": (0, 1)}),
    "pw96-255-head": (PW, 96, 255, 1, (3, 5, 5), {"y_ld": 256}),
    "pw58-58-off-acc": (PW, 58, 58, 1, (2, 9, 7), {"x_ld": 116, "x_off": 58, "acc": (0, 1)}),      # pw1 of a stride-1 unit: the second half of the unit tensor
    "pw116-116-cap": (PW, 116, 116, 1, (3, 9, 37), {"cap": 2}),
    # the 1.5x / 2.0x networks: pw1 of a 2.0x stage-2 unit (bf 122: no multiple of 4) on the second half of its unit tensor; the unit GEMMs of the
    # wider stages at M = 297 (two slices of 152 + 145 rows, the cut inside an image); the two widest laterals
    "pw122-122-off-acc": (PW, 122, 122, 1, (2, 9, 7), {"x_ld": 244, "x_off": 122, "acc": (0, 1)}),
    "pw244-244-m297": (PW, 244, 244, 1, (3, 9, 11), {}),
    "pw352-352-m297": (PW, 352, 352, 1, (3, 9, 11), {}),
    "pw488-488-m297": (PW, 488, 488, 1, (3, 9, 11), {}),
    "pw976-96": (PW, 976, 96, 1, (2, 9, 7), {}),
    "pw704-96": (PW, 704, 96, 1, (2, 9, 7), {}),
    # dense 3x3: the network's 96 -> 96, and the two small shapes that select the other tiles
    "c3-96-96": (C3, 96, 96, 1, (2, 9, 7), {"acc": (0, 1)}),
    "c3-96-96-b3": (C3, 96, 96, 1, (3, 5, 5), {}),
    "c3-96-96-m297": (C3, 96, 96, 1, (3, 9, 11), {}),
    "c3-6-14": (C3, 6, 14, 1, (2, 9, 7), {}),
    "c3-6-14-strip": (C3, 6, 14, 1, (2, 1, 7), {}),
    "c3-8-16": (C3, 8, 16, 1, (3, 5, 5), {}),
    "c3-8-16-m1": (C3, 8, 16, 1, (1, 1, 1), {}),
    # depthwise stride 1: W on each side of the run of 8
    "dw24-s1-w7": (DW, 24, 24, 1, (2, 5, 7), {"acc": (0, 1)}),
    "dw58-s1-w8": (DW, 58, 58, 1, (2, 6, 8), {"acc": (0, 1)}),
    "dw116-s1-w9": (DW, 116, 116, 1, (3, 5, 9), {"acc": (0, 1)}),
    "dw232-s1-w13": (DW, 232, 232, 1, (2, 4, 13), {"acc": (0, 1)}),
    "dw58-s1-off": (DW, 58, 58, 1, (2, 5, 9), {"x_ld": 116, "x_off": 58, "acc": (0, 1)}),
    "dw232-s1-cap": (DW, 232, 232, 1, (3, 9, 11), {"cap": 8}),
    # depthwise stride 2: the run of 4; odd extents
    "dw24-s2-w6": (DW, 24, 24, 2, (2, 8, 6), {"acc": (0, 1)}),
    "dw58-s2-w10": (DW, 58, 58, 2, (2, 6, 10), {"acc": (0, 1)}),
    "dw116-s2-w12": (DW, 116, 116, 2, (3, 4, 12), {"acc": (0, 1)}),
    "dw232-s2-odd": (DW, 232, 232, 2, (2, 7, 9), {"acc": (0, 1)}),
    "dw58-s2-odd": (DW, 58, 58, 2, (1, 5, 5), {"acc": (0, 1)}),
    # the branch widths of 2.0x and 1.5x stage 4: 122 (61 channel pairs on 64 lanes), 244 (122 on 128), 352 and 488 (176 / 244 on 256 lanes: one row-lane per block)
    "dw122-s1-w9": (DW, 122, 122, 1, (2, 5, 9), {"acc": (0, 1)}),
    "dw244-s1-w7": (DW, 244, 244, 1, (2, 5, 7), {"acc": (0, 1)}),
    "dw352-s1-w8": (DW, 352, 352, 1, (2, 4, 8), {"acc": (0, 1)}),
    "dw488-s1-w13": (DW, 488, 488, 1, (2, 4, 13), {"acc": (0, 1)}),
    "dw122-s2-w6": (DW, 122, 122, 2, (2, 8, 6), {"acc": (0, 1)}),
    "dw244-s2-w10": (DW, 244, 244, 2, (2, 6, 10), {"acc": (0, 1)}),
    "dw352-s2-w12": (DW, 352, 352, 2, (3, 4, 12), {"acc": (0, 1)}),
    "dw488-s2-odd": (DW, 488, 488, 2, (2, 7, 9), {"acc": (0, 1)}),
    # stem: Wo = 16, 15, 24, 17; B = 1 and 3
    "stem-32x32-b1": (STEM, 3, 24, 2, (1, 32, 32), {}),
    "stem-32x32-b3": (STEM, 3, 24, 2, (3, 32, 32), {}),
    "stem-34x30-b1": (STEM, 3, 24, 2, (1, 34, 30), {}),
    "stem-34x30-b3": (STEM, 3, 24, 2, (3, 34, 30), {}),
    "stem-64x48-b1": (STEM, 3, 24, 2, (1, 64, 48), {}),
    "stem-64x48-b3": (STEM, 3, 24, 2, (3, 64, 48), {}),
    "stem-33x34-b3": (STEM, 3, 24, 2, (3, 33, 34), {}),
    "stem-cap": (STEM, 3, 24, 2, (3, 34, 30), {"cap": 3}),
}


def _wgrad_tile(N, K):
    """launch_wgrad's choice, restated: the tile with the fewest (padded) 32x32 MFMA tiles, ties to the larger one"""
    t = lambda nt, kt: -(-N // (nt * 32)) * nt * -(-K // (kt * 32)) * kt
    c22, c24, c33 = t(2, 2), t(2, 4), t(3, 3)
    return (3, 3) if c33 <= c24 and c33 <= c22 else ((2, 4) if c24 <= c22 else (2, 2))


def test_conv_cases_reach_every_wgrad_tile():
    seen = {(k, _wgrad_tile(co, ci * (9 if k == C3 else 1))) for k, ci, co, _, _, _ in CONV_CASES.values() if k in (PW, C3)}
    assert seen == {(k, t) for k in (PW, C3) for t in ((2, 2), (2, 4), (3, 3))}


def _wshape(kind, cin, cout):
    return {PW: (cout, cin, 1, 1), DW: (cout, 1, 3, 3), C3: (cout, cin, 3, 3), STEM: (cout, 3, 3, 3)}[kind]


def _conv_data(case, gen, seed):
    kind, cin, cout, stride, (B, H, W), opt = CONV_CASES[case]
    rs = np.random.RandomState(seed)
    x_ld, x_off, y_ld = opt.get("x_ld", cin), opt.get("x_off", 0), opt.get("y_ld", cout)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d = {"x": gen(rs, B, 3, H, W) if kind == STEM else gen(rs, B, H, W, x_ld), "w": gen(rs, *_wshape(kind, cin, cout)), "bias": gen(rs, cout),
         "dy": gen(rs, B, Ho, Wo, y_ld), "prior": None if kind == STEM else gen(rs, B, H, W, x_ld)}
    d["dy"][..., cout:] = 0.0                                # the padding column of a head row carries no gradient
    return d, (x_ld, x_off, y_ld)


def _conv_ref(case, d, dtype, absolute=False):
    """F.conv2d + autograd in `dtype` -> y, dx (the conv's channels only), dw, dbias; absolute: on |values| (the sum of the terms' magnitudes)"""
    kind, cin, cout, stride, _, opt = CONV_CASES[case]
    x_off = opt.get("x_off", 0)
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    xs = d["x"] if kind == STEM else d["x"][..., x_off:x_off + cin].permute(0, 3, 1, 2)
    xs = f(xs).to(dtype).clone().requires_grad_(True)
    w = f(d["w"]).to(dtype).clone().requires_grad_(True)
    b = f(d["bias"]).to(dtype).clone().requires_grad_(True)
    y = F.conv2d(xs, w, b, stride=stride, padding=0 if kind == PW else 1, groups=cin if kind == DW else 1)
    y.backward(f(d["dy"])[..., :cout].permute(0, 3, 1, 2).to(dtype))
    return {"y": y.detach().permute(0, 2, 3, 1), "dx": xs.grad.permute(0, 2, 3, 1) if kind != STEM else None, "dw": w.grad, "dbias": b.grad}


def _conv_run(hop, case, d, geom, accumulate):
    kind, cin, cout, stride, _, opt = CONV_CASES[case]
    x_ld, x_off, y_ld = geom
    wn = d["w"].numel()
    dx = d["prior"].cuda() if kind != STEM else None
    y, dx, dw, db = hop.op_f32_conv(kind, d["x"].cuda(), d["w"].cuda(), d["bias"].cuda(), stride=stride, dy=d["dy"].cuda(), x_off=x_off, cin=cin,
                                    y_ld=y_ld, dx=dx, accumulate=accumulate, partial_cap=opt.get("cap", 0) * wn)
    torch.cuda.synchronize()
    return {"y": y.cpu(), "dx": dx.cpu() if dx is not None else None, "dw": dw.cpu(), "dbias": db.cpu()}


def _dx_expected(case, d, geom, ref_dx, accumulate, dtype):
    """the whole dx tensor: the conv's channels written (or added to), every other channel as it was"""
    _, cin, _, _, _, _ = CONV_CASES[case]
    x_ld, x_off, _ = geom
    e = d["prior"].to(dtype).clone()
    sl = e[..., x_off:x_off + cin]
    e[..., x_off:x_off + cin] = sl + ref_dx if accumulate else ref_dx
    return e


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_conv_exact(hop, case):
    """Integer data: y, dx, dw, dbias equal the float64 results bit for bit."""
    kind, cin, cout, _, _, opt = CONV_CASES[case]
    d, geom = _conv_data(case, _ints, 11)
    ref = _conv_ref(case, d, torch.float64)
    mag = _conv_ref(case, d, torch.float64, absolute=True)
    for k, v in mag.items():                                 # the exactness claim: every sum of magnitudes stays below 2**24
        if v is not None:
            assert float(v.max()) + 3.0 < 2 ** 24, (k, float(v.max()))
    for accumulate in opt.get("acc", (0,)):
        got = _conv_run(hop, case, d, geom, accumulate)
        np.testing.assert_array_equal(got["y"][..., :cout].numpy(), ref["y"].float().numpy(), err_msg="y")
        assert not got["y"][..., cout:].any(), "the padding column of y is zero"
        np.testing.assert_array_equal(got["dw"].numpy(), ref["dw"].float().numpy(), err_msg="dw")
        np.testing.assert_array_equal(got["dbias"].numpy(), ref["dbias"].float().numpy(), err_msg="dbias")
        if kind != STEM:
            np.testing.assert_array_equal(got["dx"].numpy(), _dx_expected(case, d, geom, ref["dx"], accumulate, torch.float64).float().numpy(),
                                          err_msg="dx (accumulate %d)" % accumulate)


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_conv_random(hop, case):
    """Standard-normal data: every output within 4 * e32 + 4 ulp of float64, element by element."""
    kind, cin, cout, _, _, opt = CONV_CASES[case]
    d, geom = _conv_data(case, _normal, 12)
    r64, r32 = _conv_ref(case, d, torch.float64), _conv_ref(case, d, torch.float32)
    for accumulate in opt.get("acc", (0,)):
        got = _conv_run(hop, case, d, geom, accumulate)
        _bar("y", case, got["y"][..., :cout], r64["y"], r32["y"])
        _bar("dw", case, got["dw"], r64["dw"], r32["dw"])
        _bar("dbias", case, got["dbias"], r64["dbias"], r32["dbias"])
        if kind != STEM:
            _bar("dx", "%s acc%d" % (case, accumulate), got["dx"], _dx_expected(case, d, geom, r64["dx"], accumulate, torch.float64),
                 _dx_expected(case, d, geom, r32["dx"], accumulate, torch.float32))


def test_conv_refuses_what_the_kernels_cannot_read(hop):
    """The forward depthwise kernel loads channel pairs: an odd channel offset (which no tensor of the network has) is an error, not a wrong answer."""
    from yolo_nano_amd import capi
    rs = np.random.RandomState(1)
    x, w = _ints(rs, 1, 4, 4, 50).cuda(), _ints(rs, 24, 1, 3, 3).cuda()
    with pytest.raises(capi.YnError):
        hop.op_f32_conv(DW, x, w, stride=1, x_off=25, cin=24)
    with pytest.raises(capi.YnError):
        hop.op_f32_conv(PW, x, _ints(rs, 8, 24, 1, 1).cuda(), x_off=1, cin=24)
    with pytest.raises(capi.YnError):                        # dbias of an odd channel count needs the padded row
        hop.op_f32_conv(PW, x[..., :48].contiguous(), _ints(rs, 7, 48, 1, 1).cuda(), dy=_ints(rs, 1, 4, 4, 7).cuda())
    with pytest.raises(capi.YnError):                        # BatchNorm lanes own channel pairs
        hop.op_f32_bn(_ints(rs, 8, 7).cuda(), _ints(rs, 7).cuda(), _ints(rs, 7).cuda())


# =====================================================================================================================================
# BatchNorm (train mode) + activation, plain and as the last layer of a ShuffleV2 unit
# =====================================================================================================================================
# id: M, C, act, unit form, (dz_ld - C, dz_off) of a plain dz view
BN_CASES = {
    "bn-64x24-relu": (64, 24, 1, False, (0, 0)),
    "bn-129x58": (129, 58, 0, False, (0, 0)),
    "bn-333x116-leaky": (333, 116, 2, False, (0, 0)),
    "bn-500x232-relu": (500, 232, 1, False, (0, 0)),
    "bn-4097x96-leaky": (4097, 96, 2, False, (0, 0)),
    "bn-7x58-relu": (7, 58, 1, False, (0, 0)),
    "bn-129x58-unit": (129, 58, 1, True, (0, 0)),
    "bn-333x116-unit": (333, 116, 1, True, (0, 0)),
    "bn-64x24-unit-leaky": (64, 24, 2, True, (0, 0)),
    "bn-dzoff": (129, 58, 2, False, (6, 3)),
    # the BatchNorm widths of 1.5x / 2.0x: 122 only occurs as a unit's last layer (2.0x stage 2); 176 ... 488 as pw1 (plain) and pw2 (unit form)
    "bn-77x122-unit": (77, 122, 1, True, (0, 0)),
    "bn-129x176-relu": (129, 176, 1, False, (0, 0)),
    "bn-129x176-unit": (129, 176, 1, True, (0, 0)),
    "bn-300x244": (300, 244, 0, False, (0, 0)),
    "bn-300x244-unit": (300, 244, 1, True, (0, 0)),
    "bn-65x352-leaky": (65, 352, 2, False, (0, 0)),
    "bn-65x352-unit": (65, 352, 1, True, (0, 0)),
    "bn-200x488-relu": (200, 488, 1, False, (0, 0)),
    "bn-200x488-unit-leaky": (200, 488, 2, True, (0, 0)),
}
AMBIGUOUS = 1e-5


def _bn_ref(d, act, dtype):
    y = d["y"].to(dtype).clone().requires_grad_(True)
    g, b = d["gamma"].to(dtype).clone().requires_grad_(True), d["beta"].to(dtype).clone().requires_grad_(True)
    rm, rv = d["rm"].to(dtype).clone(), d["rv"].to(dtype).clone()
    pre, mean, invstd = torch.native_batch_norm(y, g, b, rm, rv, True, 0.1, arch.BN_EPS)
    z = F.relu(pre) if act == 1 else (F.leaky_relu(pre, 0.1) if act == 2 else pre)
    z.backward(d["dz"].to(dtype))
    return {"pre": pre.detach(), "z": z.detach(), "mean": mean.detach(), "invstd": invstd.detach(), "rm": rm, "rv": rv, "dy": y.grad, "dgamma": g.grad, "dbeta": b.grad}


@pytest.mark.parametrize("case", list(BN_CASES))
def test_bn(hop, case):
    M, C, act, unit, (extra, dz_off) = BN_CASES[case]
    rs = np.random.RandomState(21)
    d = {"y": _normal(rs, M, C), "gamma": 1.0 + 0.1 * _normal(rs, C), "beta": 0.1 * _normal(rs, C), "rm": 0.1 * _normal(rs, C),
         "rv": torch.from_numpy(rs.uniform(0.5, 1.5, C).astype(np.float32)), "dz": _normal(rs, M, C)}
    r64, r32 = _bn_ref(d, act, torch.float64), _bn_ref(d, act, torch.float32)
    rm, rv = d["rm"].cuda(), d["rv"].cuda()
    if unit:
        passthrough, deven = _ints(rs, M, C), _ints(rs, M, C)
        dunit = torch.stack([deven, d["dz"]], 2).reshape(M, 2 * C)                     # dunit[:, 2c] = deven, dunit[:, 2c+1] = dz
        out = hop.op_f32_bn(d["y"].cuda(), d["gamma"].cuda(), d["beta"].cuda(), act, passthrough=passthrough.cuda(), running=(rm, rv), dz=dunit.cuda())
        out = {k: v.cpu() for k, v in out.items()}
        np.testing.assert_array_equal(out["z"][:, 0::2].numpy(), passthrough.numpy(), err_msg="pass-through half of the unit output")
        np.testing.assert_array_equal(out["deven"].numpy(), deven.numpy(), err_msg="even channels of the unit gradient")
        z = out["z"][:, 1::2]
    else:
        dzv = _normal(rs, M, C + extra)
        dzv[:, dz_off:dz_off + C] = d["dz"]
        out = hop.op_f32_bn(d["y"].cuda(), d["gamma"].cuda(), d["beta"].cuda(), act, running=(rm, rv), dz=dzv.cuda(), dz_off=dz_off)
        out = {k: v.cpu() for k, v in out.items()}
        z = out["z"]
    torch.cuda.synchronize()
    out["rm"], out["rv"] = rm.cpu(), rv.cpu()
    for k, got in (("mean", out["mean"]), ("invstd", out["invstd"]), ("z", z), ("rm", out["rm"]), ("rv", out["rv"])):
        _bar(k, case, got, r64[k], r32[k])
    # gradients: the elements whose activation sign fp32 cannot decide, and what they can move
    amb = (r64["pre"].abs() < AMBIGUOUS) if act else torch.zeros(M, C, dtype=torch.bool)
    share = float(amb.double().mean())
    print("RATIO ambiguous %-22s share %.2e" % (case, share))
    assert share <= 0.005
    step = (1.0 if act == 1 else 0.9) * d["dz"].double().abs() * amb                   # |dz| * |act'(+) - act'(-)| per undecided element
    xhat = (d["y"].double() - r64["mean"]) * r64["invstd"]
    s_beta, s_gamma = step.sum(0), (step * xhat.abs()).sum(0)
    _bar("dbeta", case, out["dbeta"], r64["dbeta"], r32["dbeta"], slack=s_beta)
    _bar("dgamma", case, out["dgamma"], r64["dgamma"], r32["dgamma"], slack=s_gamma)
    k = (d["gamma"].double() * r64["invstd"]).abs()
    clean = ~amb.any(0)                                                                # e32 of dy from the channels no undecided element touches
    _bar("dy", case, out["dy"], r64["dy"], torch.where(clean[None, :], r32["dy"].double(), r64["dy"]),
         slack=k[None, :] * (s_beta[None, :] + xhat.abs() * s_gamma[None, :]) / M, keep=~amb)


# =====================================================================================================================================
# max pool with recorded arg-max, FPN / PAN adds
# =====================================================================================================================================
@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (2, 10, 6), (2, 16, 16), (2, 7, 9)])
def test_maxpool_exact(hop, B, H, W):
    """Post-ReLU integers (about half exact zeros: ties are the common case, as in the stem's output): the recorded index is torch's (first maximum
    in window scan order) and dx is autograd's, bit for bit."""
    C = 24
    rs = np.random.RandomState(31)
    x = _ints(rs, B, H, W, C).clamp_min(0.0)
    assert 0.35 < float((x == 0).double().mean()) < 0.75
    xn = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    y64, idx64 = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
    dy = _ints(rs, B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    assert tuple(y64.shape[2:]) == tuple(dy.shape[1:3])
    y64.backward(dy.permute(0, 3, 1, 2).double())
    y, idx, dx = hop.op_f32_maxpool(x.cuda(), dy.cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(y.cpu().numpy(), y64.detach().permute(0, 2, 3, 1).float().numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), idx64.permute(0, 2, 3, 1).to(torch.int32).numpy())
    np.testing.assert_array_equal(dx.cpu().numpy(), xn.grad.permute(0, 2, 3, 1).float().numpy())


def _resample_ref(mode, a, b, prior, dtype):
    n = lambda t: t.permute(0, 3, 1, 2).to(dtype)
    back = lambda t: t.permute(0, 2, 3, 1)
    if mode == 0:
        return back(n(a) + F.interpolate(n(b), scale_factor=2, mode="nearest"))
    if mode == 1:
        return back(n(a) + F.interpolate(n(b), scale_factor=0.5, mode="nearest"))
    B, H, W, C = a.shape
    src = torch.zeros((B, C, H // 2, W // 2) if mode == 2 else (B, C, 2 * H, 2 * W), dtype=dtype, requires_grad=True)
    F.interpolate(src, scale_factor=2 if mode == 2 else 0.5, mode="nearest").backward(n(a))
    return prior.to(dtype) + back(src.grad)


@pytest.mark.parametrize("gen", ["ints", "normal"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("hi,lo", [(6, 3), (10, 5), (4, 2)])
def test_resample(hop, hi, lo, mode, gen):
    """out = a + up2(b), out = a + down(b) and their accumulating backwards (non-zero prior contents) against F.interpolate(mode="nearest") + autograd:
    bit-exact on integers, 4 * e32 + 4 ulp on normal data."""
    B, C = 2, 96
    rs = np.random.RandomState(41 + mode)
    g = _ints if gen == "ints" else _normal
    big, small = (hi, hi + 2), (lo, lo + 1)                                             # (H, W) of the two maps, W != H
    # `a` carries the entry's extent; the other map is b (modes 0 / 1) or the accumulated output (modes 2 / 3)
    (ha, wa), (hb, wb) = (big, small) if mode in (0, 2) else (small, big)
    a, b, prior = g(rs, B, ha, wa, C), g(rs, B, hb, wb, C), g(rs, B, hb, wb, C)
    out = hop.op_f32_resample(mode, a.cuda(), b.cuda() if mode <= 1 else None, out=prior.cuda() if mode >= 2 else None)
    torch.cuda.synchronize()
    r64 = _resample_ref(mode, a, b, prior, torch.float64)
    assert out.shape == r64.shape
    if gen == "ints":
        np.testing.assert_array_equal(out.cpu().numpy(), r64.float().numpy())
    else:
        _bar("resample", "mode%d %d<->%d" % (mode, hi, lo), out.cpu(), r64, _resample_ref(mode, a, b, prior, torch.float32))
