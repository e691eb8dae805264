"""stem_pool_kernel against the two kernels it fuses (yn_op_stem followed by yn_op_maxpool3x3s2) and against float64, on random normal data with
activations 0, 1 and 2.

The two routes are NOT bit-equal in channel 0, and were not before this test existed: stem_pool_kernel computes channel 0's products 15 ... 26 as a
rounded multiply and a rounded add (csrc/kernels_conv.hip, the kernel's header), stem_kernel fuses all 27.  On this data 1 - 2 % of the pooled
values differ, all of them in channel 0 (sp-32: 52 of 3 072; 416 x 416, B = 2: 7 180 of 519 168).  So:
  channels 1 ... 23: bit for bit what the two-kernel route gives;
  all 24 channels:   the element-wise float64 bar of tests/f64_bar.py (4 * the float32 reference's own error + 4 ulp), as test_gpu_infer_ops.py.

Which input path a case takes (the kernel chooses by the parity of W; nothing of it is observable from outside, tests/test_isa_stem_cpu.py pins
both paths in the assembly):
  paired loads (W even): sp-32, sp-64, sp-96, sp-27x26, sp-25x58, sp-40x36, sp-64x34, sp-6x2
  27 single loads (W odd): sp-33x23, sp-30x31, sp-3x5
In the paired path a lane takes column 2 cx - 1 from the lane to its left, and the two kinds of lane that have no such neighbour load it themselves.
Thread t is conv row t / 15, conv column t % 15 of the tile, whose first conv column is cx = 14 * tile_x - 1:
  the first lane of a conv row (t % 15 = 0): cx = -1 in the first column tile (dead: everything masked), cx = 13, 27 further right, in every case
    with more than 7 pooled columns; its right-hand neighbour (t % 15 = 1) is cx = 0 there, whose column 2 cx - 1 = -1 lies outside the image and
    whose left neighbour is dead - the value arrives by the shift and only the reader's own mask removes it;
  lane 0 of a wavefront in mid-row (t = 64, 128, 192: conv columns 4, 8, 12): cx = 3, 7, 11 in the first column tile and cx = 17, 21, 25 in the
    second, which with W 34 / 36 (Wc = 17 / 18) is the image's last conv column or just beyond it, and with W 2, 26 is partly dead;
  tiles that reach beyond the image on the right (W 2, 26, 34, 36, 58) or below (every H): dead lanes read clamped addresses."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import infer_op_cases as ioc
from f64_bar import bar, normal
from yolo_nano_amd import arch

pytestmark = pytest.mark.gpu

CASES = dict(ioc.STEM_POOL_CASES)
CASES.update({"sp-40x36": (2, 40, 36), "sp-64x34": (3, 64, 34), "sp-6x2": (2, 6, 2)})
PAIRED = {n for n, (_, _, W) in CASES.items() if W % 2 == 0}
ACTS = (0, 1, 2)


@pytest.fixture(scope="module")
def hop():
    from yolo_nano_amd import capi
    h = capi.Handle(64, 20, arch.MULTI_ANCHOR_SIZE)
    yield h
    h.close()


def _act(t, act):
    return F.relu(t) if act == 1 else (F.leaky_relu(t, 0.1) if act == 2 else t)


@functools.lru_cache(maxsize=None)
def _problem(case):
    """x, w, b and the pre-activation conv in float64 and float32 (NCHW), computed once per case"""
    B, H, W = CASES[case]
    rs = np.random.RandomState(81)
    x, w, b = normal(rs, B, 3, H, W), normal(rs, 24, 3, 3, 3), normal(rs, 24)
    pre = [F.conv2d(x.to(d), w.to(d), b.to(d), stride=2, padding=1) for d in (torch.float64, torch.float32)]
    return x, w, b, pre[0], pre[1]


def test_cases_cover_both_paths():
    assert {CASES[n][2] for n in PAIRED} == {32, 64, 96, 26, 58, 36, 34, 2}
    assert {CASES[n][2] for n in set(CASES) - PAIRED} == {23, 31, 5}
    assert set(ioc.STEM_POOL_CASES) <= set(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_stem_pool_against_its_two_kernels_and_float64(hop, case):
    x, w, b, p64, p32 = _problem(case)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    assert xd.data_ptr() % 8 == 0                            # the paired path also wants the image 8-byte aligned
    for act in ACTS:
        fused = hop.op_stem_pool(xd, wd, bd, act).cpu()
        two = hop.op_maxpool(hop.op_stem(xd, wd, bd, act)).cpu()
        assert fused.shape == two.shape, (tuple(fused.shape), tuple(two.shape))
        diff = fused.view(torch.int32) != two.view(torch.int32)
        chans = sorted(set(diff.nonzero()[:, 3].tolist()))
        print("BITS %-10s act %d: %d of %d elements differ from stem + maxpool, channels %s" % (case, act, int(diff.sum()), fused.numel(), chans))
        assert not diff[..., 1:].any(), "%s act %d: channels %s differ from yn_op_stem + yn_op_maxpool3x3s2" % (case, act, chans)
        ref = [F.max_pool2d(_act(p, act), 3, 2, 1).permute(0, 2, 3, 1) for p in (p64, p32)]
        bar("stempool", "%s act%d" % (case, act), fused, ref[0], ref[1])
