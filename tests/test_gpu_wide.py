"""The 1.5x and 2.0x backbones as whole networks against float64, with 1.0x through the same function as the control.

Per (backbone, H, W, B) of wide_cases.CASES, on ONE handle with weights.make_state_dict(backbone, 20):
  1. yn_forward_taps (c3, c4, c5) and yn_forward_raw, every tensor element-wise within f64_bar.bar (4 * e32 + 4 ulp) of oracle.torch_port.TorchNet in
     float64, e32 = the float32 TorchNet's distance from it - in the default (split-f16) family and again under yn_exact_f32.  The taps come first, in
     stage order, so that a failure names its stage.
  2. the profile records of the backbone units and the laterals ARE wide_cases.plan(...): which kernel ran is asserted, not assumed (both families).
  3. yn_down_fuse, yn_unit_chain and yn_group_launch off in turn, yn_chain_pipe and yn_stage_fuse in every mode: raw heads bit-identical to the default run,
     records = the plan of that switch; on a wide backbone no stage_pipe_kernel / unit_pipe_kernel / pw_pipe_kernel in any backbone or lateral record (the
     detection heads are 96 channels wide whatever the backbone: with yn_group_launch off the autotuner may give them pw_pipe_kernel<96,96>).
  4. the default run three more times under yn_use_graph (capture, two replays), both families: bit-identical.  The five-launch stride-2 units fork and join
     streams; only the wide backbones and the exact family take that route inside a captured graph.
  5. range_status() == (False, False).
H != W runs as a window (yn_set_grid_rect); TorchNet is fully convolutional and takes the H x W input as it stands.

unit_chain_kernel<2,2,4,4> at bf 244 (the exact family from 256 tiles of 64 stage-3 pixels) needs 2.0x at 512 x 512 x 16: no float64 CPU reference within a
few seconds, so test_big_exact_chain_tile compares yn_unit_chain on against off, bit for bit, kernel names asserted; the off path (three launches per unit) is
the one the small shapes check against float64.

The bar is the per-kernel suites' own and holds with its factor 4 for whole networks: the control sits at the same err / bar as the wide backbones in the split family
(0.27 against 0.28) and below them in the exact one (0.40 against 0.58, where the f32 MFMA's longer sums show).  Measured on an MI355X inside the whole suite, all 180
RATIO lines below 0.6; the worst tap and the worst head of each backbone and family:
  RATIO split    1.0x 64x64x2 c4        err 4.384e-06  e32 3.602e-06  ulp 4.768e-07  err/bar 0.269
  RATIO split    1.0x 192x192x15 head16 err 1.736e-05  e32 1.814e-05  ulp 9.537e-07  err/bar 0.227
  RATIO exact    1.0x 64x64x2 c4        err 4.627e-06  e32 3.602e-06  ulp 4.768e-07  err/bar 0.284
  RATIO exact    1.0x 160x160x3 head32  err 2.225e-05  e32 1.285e-05  ulp 9.537e-07  err/bar 0.403
  RATIO split    1.5x 192x192x15 c4     err 1.921e-05  e32 1.643e-05  ulp 1.907e-06  err/bar 0.262
  RATIO split    1.5x 96x160x2 head16   err 2.867e-05  e32 2.448e-05  ulp 3.815e-06  err/bar 0.253
  RATIO exact    1.5x 96x160x2 c5       err 1.713e-05  e32 1.148e-05  ulp 9.537e-07  err/bar 0.345
  RATIO exact    1.5x 96x96x1 head32    err 2.131e-05  e32 8.260e-06  ulp 9.537e-07  err/bar 0.578
  RATIO split    2.0x 192x192x15 c5     err 1.828e-05  e32 1.851e-05  ulp 1.907e-06  err/bar 0.224
  RATIO split    2.0x 96x160x2 head32   err 2.043e-05  e32 1.610e-05  ulp 1.907e-06  err/bar 0.284
  RATIO exact    2.0x 64x64x2 c5        err 1.110e-05  e32 6.111e-06  ulp 4.768e-07  err/bar 0.421
  RATIO exact    2.0x 192x192x15 head16 err 8.277e-05  e32 4.001e-05  ulp 3.815e-06  err/bar 0.472
The kernel errors reproduce from run to run; e32 is torch's fp32 on the host CPU and moved with the host and the process (1.5x 96x96x1 head32: 1.354e-05 when this
module ran alone, 8.260e-06 inside the suite - err/bar 0.37 and 0.58 for the same 2.131e-05).
The cases notice a wrong kernel.  Tried once with two deliberately wrong libraries (value-only changes, no address touched): (1) gemm_split_tile skipping its final
partial 16-deep k-step failed all fifteen network cases, the c3 tap first (1.5x and 2.0x stage 2 enter with K = 24; errors of 5 ... 10), and exactly the split-family
cases of PW_WIDE_CASES with K % 16 != 0 (K = 24, 88, 122, 244, 488; K = 176, 352, 704, 976 and the f32 family rightly passed), exact and random; the exact-family
test_big_exact_chain_tile, which the change does not touch, passed.  (2) gemm_epilogue not storing the last column (the last quad in its 16-byte form) failed all
sixteen cases here and all 104 pointwise cases of tests/test_gpu_infer_ops.py.
"""
import functools

import numpy as np
import pytest
import torch

import wide_cases as wc
from f64_bar import bar
from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu

C = 20


@pytest.fixture(scope="module")
def capi():
    from yolo_nano_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return c


@functools.lru_cache(maxsize=None)
def _state(backbone):
    return weights.make_state_dict(backbone, C)


@functools.lru_cache(maxsize=4)
def _problem(backbone, H, W, B):
    """the input and the float64 / float32 references of one case, NHWC: (x, [c3, c4, c5, head8, head16, head32] in float64, the same in float32)"""
    from oracle.torch_port import TorchNet
    x = np.random.RandomState(1000 * H + 10 * W + B).standard_normal((B, 3, H, W)).astype(np.float32)
    nhwc = lambda ts: [t.permute(0, 2, 3, 1).contiguous() for t in ts]
    t64, h64 = TorchNet(_state(backbone), backbone, C, dtype=torch.float64).forward_taps(x)
    t32, h32 = TorchNet(_state(backbone), backbone, C).forward_taps(x)
    return x, nhwc(t64 + h64), nhwc(t32 + h32)


def _handle(capi, backbone, H, W, B):
    h = capi.Handle(max(H, W), C, arch.MULTI_ANCHOR_SIZE, backbone, 0.001, 0.5, max_batch=B)
    h.load_state_dict(_state(backbone))
    h.fold_bn()
    if H != W:
        h.set_grid_rect(H, W)
    return h


def _profiled(h, x):
    """the raw heads of one profiled forward and its records"""
    h.profile_enable(True)
    try:
        raw = [t.clone() for t in h.forward_raw(x)]
        torch.cuda.synchronize()
        recs = h.profile_records()
    finally:
        h.profile_enable(False)
    return raw, recs


def _same(got, ref, what):
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), "%s: head %d differs in %d of %d elements (max %g)" % (what, i, int((a != b).sum()), a.numel(), float((a - b).abs().max()))


NAMES = ("c3", "c4", "c5", "head8", "head16", "head32")


@pytest.mark.parametrize("backbone,H,W,B", wc.CASES)
def test_wide_network(capi, backbone, H, W, B):
    xn, r64, r32 = _problem(backbone, H, W, B)
    tag = "%s %dx%dx%d" % (backbone, H, W, B)
    st = torch.cuda.Stream()                                 # a stream of the handle's own: graph capture needs one
    with torch.cuda.stream(st):
        _network_steps(_handle(capi, backbone, H, W, B), backbone, H, W, B, tag, xn, r64, r32)


def _network_steps(h, backbone, H, W, B, tag, xn, r64, r32):
    try:
        x = torch.as_tensor(xn).cuda()
        raws = {}
        for exact in (False, True):
            fam = "exact" if exact else "split"
            h.exact_f32(exact)
            # 1. taps and heads against float64
            taps = [t.cpu() for t in h.forward_taps(x)]
            raws[exact] = [t.clone() for t in h.forward_raw(x)]
            missed = []
            for name, got, a, b in zip(NAMES, taps + [t.cpu() for t in raws[exact]], r64, r32):
                try:
                    bar(fam, "%s %s" % (tag, name), got, a, b)
                except AssertionError as e:
                    missed.append(str(e))
            assert not missed, "\n".join(missed)
            # 2. the kernels that ran are the plan's
            raw, recs = _profiled(h, x)
            _same(raw, raws[exact], "%s %s profiled" % (tag, fam))
            bad = wc.matches(recs, wc.plan(backbone, H, W, B, exact=exact), exact, backbone)
            assert bad is None, "%s %s: %s\n%s" % (tag, fam, bad, wc.backbone_records(recs))
            # 4. captured and replayed
            out = [torch.empty_like(t) for t in raws[exact]]
            h.use_graph(True)
            try:
                for rep in range(3):
                    for t in out:
                        t.fill_(float("nan"))
                    h.forward_raw(x, out=out)
                    _same(out, raws[exact], "%s %s graph run %d" % (tag, fam, rep))
            finally:
                h.use_graph(False)
        h.exact_f32(False)
        # 3. the switches are pure speed matters
        switches = [("down_fuse", h.down_fuse, (False,), True, "down_fuse"), ("unit_chain", h.unit_chain, (0,), 1, "unit_chain"),
                    ("group_launch", h.group_launch, (False,), True, "group_launch"), ("chain_pipe", h.chain_pipe, (0, 2), 1, "chain_pipe"),
                    ("stage_fuse", h.stage_fuse, (0, 2), 1, None)]
        for name, setter, values, default, kw in switches:
            for v in values:
                setter(v)
                try:
                    raw, recs = _profiled(h, x)
                finally:
                    setter(default)
                _same(raw, raws[False], "%s %s(%s)" % (tag, name, v))
                if backbone in wc.WIDE:
                    piped = [r for r in wc.backbone_records(recs) if r[1].startswith(wc.PIPE_PREFIXES)]     # (the 96 -> 96 heads are no wide layer: pw_pipe_kernel<96,96> may serve them)
                    assert not piped, "%s %s(%s): %s" % (tag, name, v, piped)
                if kw is not None and (backbone in wc.WIDE or name != "chain_pipe" or v == 0):
                    bad = wc.matches(recs, wc.plan(backbone, H, W, B, **{kw: v}), False, backbone)
                    assert bad is None, "%s %s(%s): %s\n%s" % (tag, name, v, bad, wc.backbone_records(recs))
        _same(h.forward_raw(x), raws[False], "%s after the switches" % tag)
        # 5.
        assert h.range_status() == (False, False), tag
    finally:
        h.close()


def test_big_exact_chain_tile(capi):
    """unit_chain_kernel<2,2,4,4> at bf 244: yn_unit_chain on against off, stage 3's tap and the raw heads bit for bit"""
    backbone, H, W, B = wc.BIG_EXACT
    h = _handle(capi, backbone, H, W, B)
    try:
        h.autotune(False)                                    # (the pointwise tile is a speed matter; timing 40 layer shapes at this size is not what this test is about)
        h.exact_f32(True)
        x = torch.as_tensor(np.random.RandomState(5).standard_normal((B, 3, H, W)).astype(np.float32)).cuda()
        h.unit_chain(0)
        raw0, recs0 = _profiled(h, x)
        tap0 = h.forward_taps(x)[1].clone()
        h.unit_chain(1)
        raw1, recs1 = _profiled(h, x)
        for recs, kw in ((recs0, {"unit_chain": 0}), (recs1, {})):
            bad = wc.matches(recs, wc.plan(backbone, H, W, B, exact=True, **kw), True, backbone)
            assert bad is None, "%s\n%s" % (bad, wc.backbone_records(recs))
        ran = [k for n, k in wc.backbone_records(recs1) if n.startswith("backbone.stage3.") and "dw+pw2" in n]
        assert ran == ["unit_chain_kernel<2,2,4,4>"] * 7, ran
        assert not any(k.startswith("unit_chain") for _, k in wc.backbone_records(recs0))
        _same(raw1, raw0, "unit_chain on against off")
        assert torch.equal(h.forward_taps(x)[1], tap0), "stage 3's tap"
        assert float(tap0.abs().max()) > 0.0 and bool(torch.isfinite(tap0).all())
        assert h.range_status() == (False, False)
    finally:
        h.close()
