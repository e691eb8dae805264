"""Every inference conv / pool kernel variant of csrc/kernels_conv.hip on its own against float64 torch on the CPU, through the single-operator
entries (yn_op_dwconv3x3 / _conv3x3 / _stem / _stem_pool / _maxpool3x3s2 / _pwconv / _pwconv_shuffle).  The launchers pick a variant from the
shape; tests/infer_op_cases.py holds the shapes and a restatement of those rules, tests/test_infer_ops_cases_cpu.py checks that the shapes reach
every variant, and every case here asserts the symbol of the kernel that ran (the profile record of the call).

Two kinds of case per shape, as in tests/test_gpu_train_ops.py.
  EXACT   x, w, bias (and the second input of a fused resample-add) are integers in {-3..3}, activation none or ReLU: every product and partial sum
          is an integer below 2**24 (checked per case on the absolute values), so the result equals the float64 one bit for bit in any summation
          order.  That holds for the split-f16 kernels too: such integers are exact in the `hi` half, `lo` is 0 (csrc/yn_split.h), and the MFMAs
          accumulate in fp32.  LeakyReLU is left to the random cases (0.1f * v is not the float64 product).
  RANDOM  standard-normal data, all three activations, element-wise |kernel - float64| <= 4 * e32 + 4 ulp with e32 = max |torch fp32 CPU - float64|
          of the same output (tests/f64_bar.py).
The max pool is compared exactly on random floats (max is exact), with windows that hold only negative values.

Which case reaches which kernel (template arguments in brackets):
  dwconv3x3_kernel      [1,4,2] dw24-s1-w1 / -w2 / -w3-h1, dw116-s1-w5     [1,2,4] dw58-s1-w1 / -w3 / -w4 / -w5-h1 / -w9     [2,4,2] dw116-s2-w1 / -w4 / -w10,
                        dw24-s2-w5-h1, dw232-s2-w9     [2,2,2] dw58-s2-w1 / -w3 / -w6-h1 / -w9: Wo = R - 1, R, R + 1, 2R + 1, one-row and one-column strips
                        [1,4,4] dw232-s1-long  [1,2,8] dw58-s1-long  [2,4,4] dw464-s2-long  [2,2,4] dw58-s2-long: the smallest tensors with >= 1024 blocks
                        the branch widths of 1.5x / 2.0x: [1,4,2] dw88- / dw244- / dw352- / dw488-s1-*   [2,4,2] the same widths' -s2-* (odd H and W)
                        [1,2,4] dw122-s1-w5 / -w9   [2,2,2] dw122-s2-w5 / -w9 (122 is the one wide width that is no multiple of 4)
  conv3x3_split_kernel  [1,1,9] c3s-1tile(-rs), c3s-3tiles(-rs), c3s-w65, c3s-n80   [1,1,3] c3s-w66 / -w70 / -w109   [1,1,1] c3s-w110 / -w112 / -w124
                        [1,2,1] c3s-86tiles   [3,2] c3s-257tiles
  conv3x3_halo_tap_kernel (exact_f32)  [1,96,1] c3t-1tile, c3t-3tiles-rs, c3t-w23 / -w32 / -w96, c3t-n192, c3t-n80   [1,96,2] c3t-w24, c3t-26x26, c3t-w31
                        [3,96,1] c3t-257tiles
  conv3x3_halo_kernel   [1] c3h-32-32 (+ resample), c3h-64-160   [2] c3h-64-64   [3] c3h-32-96, c3h-96-75 (odd Cout), c3h-96-96-w97 / -w112 (exact_f32)
  gemm_conv_kernel, im2col form   [4,1,3] c3g-96-96-w113 (exact_f32), c3g-96-96-w125, c3g-256-96 (+ resample)   [4,1,1] c3g-256-32, c3g-96-64-w124
  stem_kernel           stem-*: Wo = 16, 15, 17; B = 1 and 3
  stem_pool_kernel      sp-*: pooled extents below, at and above the 8 x 7 tile, odd conv extents (the -inf padding of the last window), B = 2 and 3
  maxpool_kernel        mp-*; mp-2nd-pass: the grid-stride loop's second turn
  gemm_conv_kernel<4,1,1,0,16,2> / gemm_split_kernel<4,1,1,32>   the pointwise shape list, plain and with the concat+shuffle epilogue (the other
                        configurations of each family are pinned bit-identical to these by test_gpu_parity.py); PW_WIDE_CASES: every K / N of the 1.5x and
                        2.0x networks - unit GEMMs (K = N = 88 ... 488), stage entries (24 -> 88 / 122, 176 -> 88, ... 488 -> 244), laterals (K = 704 / 976)

Measured on an MI355X: the worst (kernel error) / (4 * e32 + 4 ulp) over the random cases of each family, with that case's kernel error and e32.
Every exact case matched bit for bit.
  depthwise           0.18  dw232-s2-w9 act 1          1.4e-06 / 1.0e-06        stem_kernel         0.19  stem-32x32-b3 act 1     4.2e-06 / 3.6e-06
  conv3x3_split       0.10  c3s-w110 act 1             3.5e-05 / 7.8e-05        stem_pool_kernel    0.17  sp-96 act 0             4.6e-06 / 4.8e-06
  conv3x3_halo_tap    0.26  c3t-w96 act 0              8.9e-05 / 7.9e-05        pointwise f32-MFMA  0.42  1x58->58 act 1          4.1e-06 / 1.5e-06
  conv3x3_halo        0.25  c3h-96-96-w97 act 1        8.5e-05 / 7.7e-05        pointwise split-f16 0.14  77x48->24 act 1         3.5e-06 / 4.4e-06
  gemm_conv (3x3)     0.27  c3g-256-96 act 1           3.6e-04 / 3.2e-04        (the shuffle form gives the same figures as the plain one: same bits)
The split-f16 kernels stay below half of the f32-MFMA kernels' error on the same problems (c3s-* against c3t-*, pointwise split against f32).
With the 1.5x / 2.0x widths added the worst cases moved to them: depthwise 0.23 dw122-s1-w9 act 1 (2.0e-06 / 1.1e-06), pointwise f32-MFMA 0.47 33x352->352 act 0
(6.2e-05 / 2.6e-05), pointwise split-f16 0.15 on the same problem (1.9e-05); every exact case, K = 976 included, matched bit for bit.
The cases notice what the whole-network tests cannot.  Tried once with a deliberately wrong library, three mask changes (no address, bound or loop limit
touched): (1) dwconv3x3_block's column mask left on for the column just past the right edge (the clamped load then brings the last column in) failed every
depthwise case, exact and random, whose last window reaches past the edge - all stride-1 cases, the four long-run ones included, and the stride-2 cases of
odd W; dw116-s2-w4, dw116-s2-w10 and dw58-s2-w6-h1 (even W at stride 2: no window reaches column W) rightly passed.  (2) conv3x3_split_kernel's bottom-row
tap mask left on in every tile but the first failed all twelve split cases of more than one tile, in all five variants; c3s-1tile and c3s-1tile-rs (one
tile) and every case of the three other families, which the change does not touch, passed.  (3) stem_pool_kernel's `live` test dropping the last conv
column failed all eight sp-* cases; the stem_kernel, max pool and pointwise cases passed.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import infer_op_cases as ioc
from f64_bar import bar, ints, normal
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu

EXACT_ACTS, RANDOM_ACTS = (0, 1), (0, 1, 2)


@pytest.fixture(scope="module")
def hop():
    from yolo_nano_amd import capi
    h = capi.Handle(64, 20, arch.MULTI_ANCHOR_SIZE)
    yield h
    h.close()


def _ran(h, fn):
    """fn() under the handle's profile: its result (on the CPU) and the kernel symbols its launches recorded"""
    h.profile_enable(True)
    try:
        y = fn()
        torch.cuda.synchronize()
        names = [r[1] for r in h.profile_records()]
    finally:
        h.profile_enable(False)
    return y.cpu(), names


def _act(t, act):
    return F.relu(t) if act == 1 else (F.leaky_relu(t, 0.1) if act == 2 else t)


def _same(got, ref64, what):
    """bit for bit: the float32 result, widened, is the float64 one"""
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    if not torch.equal(got.double(), ref64):
        bad = (got.double() != ref64).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r against %r" % (what, len(bad), got.numel(), i, float(got[i]), float(ref64[i])))


def _below_2_24(mag, what):
    assert float(mag.max()) + 3.0 < 2 ** 24, (what, float(mag.max()))


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


# =====================================================================================================================================
# depthwise 3x3
# =====================================================================================================================================
def _dw_data(case, gen, seed):
    C, stride, (B, H, W) = ioc.DW_CASES[case]
    rs = np.random.RandomState(seed)
    return gen(rs, B, H, W, C), gen(rs, C, 1, 3, 3), gen(rs, C)


def _dw_ref(case, x, w, b, dtype):
    C, stride, _ = ioc.DW_CASES[case]
    return _nhwc(F.conv2d(_nchw(x).to(dtype), w.to(dtype), b.to(dtype), stride=stride, padding=1, groups=C))


def _dw_run(hop, case, x, w, b, act):
    C, stride, (B, H, W) = ioc.DW_CASES[case]
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y, names = _ran(hop, lambda: hop.op_dwconv3x3(xd, wd, bd, stride, act))
    assert names == [ioc.dw_kernel(ioc.dw_variant(C, stride, B, H, W))], names
    return y


@pytest.mark.parametrize("case", list(ioc.DW_CASES))
def test_dw_exact(hop, case):
    x, w, b = _dw_data(case, ints, 51)
    pre = _dw_ref(case, x, w, b, torch.float64)
    _below_2_24(_dw_ref(case, x.abs(), w.abs(), b.abs(), torch.float64), case)
    for act in EXACT_ACTS:
        _same(_dw_run(hop, case, x, w, b, act), _act(pre, act), "%s act %d" % (case, act))


@pytest.mark.parametrize("case", list(ioc.DW_CASES))
def test_dw_random(hop, case):
    x, w, b = _dw_data(case, normal, 52)
    p64, p32 = _dw_ref(case, x, w, b, torch.float64), _dw_ref(case, x, w, b, torch.float32)
    for act in RANDOM_ACTS:
        bar("dw", "%s act%d" % (case, act), _dw_run(hop, case, x, w, b, act), _act(p64, act), _act(p32, act))


# =====================================================================================================================================
# dense 3x3 (+ the fused FPN / PAN resample-add)
# =====================================================================================================================================
def _c3_family(kernel):
    return {"conv3x3_split_kernel": "c3split", "conv3x3_halo_tap_kernel": "c3tap", "conv3x3_halo_kernel": "c3halo", "gemm_conv_kernel": "c3gemm"}[kernel.split("<")[0]]


@functools.lru_cache(maxsize=None)
def _c3_problem(cin, cout, shape, mode, kind):
    """data and references of one (shape, resample mode), shared by the cases that differ only in the handle mode: x, x2, w, b and the
    pre-activation results in float64, float32 and (exact kind) float64 on the absolute values"""
    B, H, W = shape
    gen = ints if kind == "exact" else normal
    rs = np.random.RandomState(61 + mode + (0 if kind == "exact" else 10))
    x, w, b = gen(rs, B, H, W, cin), gen(rs, cout, cin, 3, 3), gen(rs, cout)
    x2 = None if mode == 0 else (gen(rs, B, H // 2, W // 2, cin) if mode == 1 else gen(rs, B, 2 * H, 2 * W, cin))

    def ref(dtype, f=lambda t: t):
        s = f(x).to(dtype)
        if mode == 1:                                        # a + up2(b): out[y, x] += b[y // 2, x // 2]
            s = s + f(x2).to(dtype).repeat_interleave(2, 1).repeat_interleave(2, 2)
        elif mode == 2:                                      # a + down(b): out[y, x] += b[2y, 2x]
            s = s + f(x2).to(dtype)[:, 0::2, 0::2]
        return _nhwc(F.conv2d(_nchw(s), f(w).to(dtype), f(b).to(dtype), padding=1)).contiguous()
    return x, x2, w, b, ref(torch.float64), ref(torch.float32) if kind == "random" else None, ref(torch.float64, torch.abs) if kind == "exact" else None


def _c3_each(hop, case, kind, acts):
    """[(tag, kernel output, pre64, pre32, act)] for every resample mode and activation of the case, having asserted the kernel"""
    cin, cout, (B, H, W), exact_f32, modes = ioc.C3_CASES[case]
    want = ioc.c3_kernel(cin, cout, B, H, W, exact_f32)
    out = []
    hop.exact_f32(exact_f32)
    try:
        for mode in modes:
            x, x2, w, b, p64, p32, mag = _c3_problem(cin, cout, (B, H, W), mode, kind)
            if mag is not None:
                _below_2_24(mag, case)
            xd, wd, bd, x2d = x.cuda(), w.cuda(), b.cuda(), x2.cuda() if x2 is not None else None
            for act in acts:
                y, names = _ran(hop, lambda: hop.op_conv3x3(xd, wd, bd, act, x2=x2d, resample=mode))
                assert names == [want], names
                out.append(("%s rs%d act%d" % (case, mode, act), y, p64, p32, act))
    finally:
        hop.exact_f32(False)
    return out


@pytest.mark.parametrize("case", list(ioc.C3_CASES))
def test_c3_exact(hop, case):
    for tag, y, p64, _, act in _c3_each(hop, case, "exact", EXACT_ACTS):
        _same(y, _act(p64, act), tag)


@pytest.mark.parametrize("case", list(ioc.C3_CASES))
def test_c3_random(hop, case):
    cin, cout, (B, H, W), exact_f32, _ = ioc.C3_CASES[case]
    fam = _c3_family(ioc.c3_kernel(cin, cout, B, H, W, exact_f32))
    for tag, y, p64, p32, act in _c3_each(hop, case, "random", RANDOM_ACTS):
        bar(fam, tag, y, _act(p64, act), _act(p32, act))


# =====================================================================================================================================
# stem conv, stem conv + max pool, max pool
# =====================================================================================================================================
def _stem_data(shape, gen, seed):
    B, H, W = shape
    rs = np.random.RandomState(seed)
    return gen(rs, B, 3, H, W), gen(rs, 24, 3, 3, 3), gen(rs, 24)


def _stem_ref(x, w, b, dtype):
    return F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=2, padding=1)        # NCHW


def _stem_run(hop, pooled, x, w, b, act):
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y, names = _ran(hop, lambda: (hop.op_stem_pool if pooled else hop.op_stem)(xd, wd, bd, act))
    assert names == ["stem_pool_kernel<24>" if pooled else "stem_kernel<24>"], names
    return y


def _stem_out(pre, act, pooled):
    """activation, then (the fused form) max_pool2d(3, 2, 1), as NHWC"""
    z = _act(pre, act)
    return _nhwc(F.max_pool2d(z, 3, 2, 1) if pooled else z)


STEM_ALL = [("stem", c) for c in ioc.STEM_CASES] + [("pool", c) for c in ioc.STEM_POOL_CASES]


@pytest.mark.parametrize("form,case", STEM_ALL)
def test_stem_exact(hop, form, case):
    pooled = form == "pool"
    x, w, b = _stem_data((ioc.STEM_POOL_CASES if pooled else ioc.STEM_CASES)[case], ints, 71)
    pre = _stem_ref(x, w, b, torch.float64)
    _below_2_24(_stem_ref(x.abs(), w.abs(), b.abs(), torch.float64), case)
    for act in EXACT_ACTS:
        _same(_stem_run(hop, pooled, x, w, b, act), _stem_out(pre, act, pooled), "%s act %d" % (case, act))


@pytest.mark.parametrize("form,case", STEM_ALL)
def test_stem_random(hop, form, case):
    pooled = form == "pool"
    x, w, b = _stem_data((ioc.STEM_POOL_CASES if pooled else ioc.STEM_CASES)[case], normal, 72)
    p64, p32 = _stem_ref(x, w, b, torch.float64), _stem_ref(x, w, b, torch.float32)
    for act in RANDOM_ACTS:
        bar("stempool" if pooled else "stem", "%s act%d" % (case, act), _stem_run(hop, pooled, x, w, b, act), _stem_out(p64, act, pooled), _stem_out(p32, act, pooled))


@pytest.mark.parametrize("case", list(ioc.MAXPOOL_CASES))
def test_maxpool_exact(hop, case):
    """Random floats shifted down by one, so that many windows hold only negative values (zero padding instead of -inf would win them)."""
    B, H, W, C = ioc.MAXPOOL_CASES[case]
    x = normal(np.random.RandomState(81), B, H, W, C) - 1.0
    xd = x.cuda()
    y, names = _ran(hop, lambda: hop.op_maxpool(xd))
    assert names == ["maxpool_kernel"], names
    assert tuple(y.shape) == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    negative = 0
    for i in range(B):                                       # image by image: the large case stays small in float64
        ref = _nhwc(F.max_pool2d(_nchw(x[i:i + 1]).double(), 3, 2, 1))
        negative += int((ref < 0).sum())
        _same(y[i:i + 1], ref, "%s image %d" % (case, i))
    assert negative > 0


# =====================================================================================================================================
# pointwise, plain and with the concat + channel-shuffle epilogue: the first configuration of each family
# =====================================================================================================================================
def _pw_data(M, cin, cout, gen, seed):
    rs = np.random.RandomState(seed + M + cin)
    return gen(rs, 1, 1, M, cin), gen(rs, cout, cin, 1, 1), gen(rs, cout), gen(rs, 1, 1, M, cout)


def _pw_ref(x, w, b, dtype):
    return _nhwc(F.conv2d(_nchw(x).to(dtype), w.to(dtype), b.to(dtype)))


def _pw_each(hop, fam, M, cin, cout, x, w, b, passthrough, acts):
    """[(form, act, y)] for the plain entry and, for an even Cout, the shuffle entry (whose even channels are checked here: the pass-through, exactly)"""
    xd, wd, bd, pd = x.cuda(), w.cuda(), b.cuda(), passthrough.cuda()
    out = []
    hop.set_pw_config(hop.pw_families()[fam][0])
    try:
        for act in acts:
            y, names = _ran(hop, lambda: hop.op_pwconv(xd, wd, bd, act))
            assert names == [ioc.PW_FIRST_KERNEL[fam]], names
            out.append(("pw", act, y))
            if cout % 2 == 0:
                y, names = _ran(hop, lambda: hop.op_pwconv_shuffle(xd, pd, wd, bd, act))
                assert names == [ioc.PW_FIRST_KERNEL[fam]], names
                assert tuple(y.shape) == (1, 1, M, 2 * cout)
                assert torch.equal(y[..., 0::2], passthrough), "pass-through half of the unit output"
                out.append(("shuf", act, y[..., 1::2]))
    finally:
        hop.set_pw_config(-1)
    return out


@pytest.mark.parametrize("fam", [0, 1], ids=["f32", "split"])
@pytest.mark.parametrize("M,cin,cout,act", ioc.PW_CASES + ioc.PW_WIDE_CASES)
def test_pw_exact(hop, M, cin, cout, act, fam):
    x, w, b, passthrough = _pw_data(M, cin, cout, ints, 91)
    pre = _pw_ref(x, w, b, torch.float64)
    _below_2_24(_pw_ref(x.abs(), w.abs(), b.abs(), torch.float64), (M, cin, cout))
    for form, a, y in _pw_each(hop, fam, M, cin, cout, x, w, b, passthrough, EXACT_ACTS):
        _same(y, _act(pre, a), "%s %dx%d->%d act %d" % (form, M, cin, cout, a))


@pytest.mark.parametrize("fam", [0, 1], ids=["f32", "split"])
@pytest.mark.parametrize("M,cin,cout,act", ioc.PW_CASES + ioc.PW_WIDE_CASES)
def test_pw_random(hop, M, cin, cout, act, fam):
    x, w, b, passthrough = _pw_data(M, cin, cout, normal, 92)
    p64, p32 = _pw_ref(x, w, b, torch.float64), _pw_ref(x, w, b, torch.float32)
    for form, a, y in _pw_each(hop, fam, M, cin, cout, x, w, b, passthrough, RANDOM_ACTS):
        bar(form + ("-f32", "-split")[fam], "%dx%d->%d act%d" % (M, cin, cout, a), y, _act(p64, a), _act(p32, a))
