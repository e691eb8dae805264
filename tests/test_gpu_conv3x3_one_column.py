"""The split-f16 dense 3x3 between 128 and 255 tiles, where launch_conv3x3 now takes the one-column form conv3x3_split_kernel<3,2> instead of the three block columns of
<1,2,1> (tests/test_conv3x3_one_column_rule_cpu.py restates the rule), through hop.op_conv3x3 as tests/test_gpu_infer_ops.py runs the other shapes.  Per shape and resample mode:
  * exact integer data in {-3..3}: the output IS the float64 reference, for every activation;
  * random data: the c3split family's bar of tests/f64_bar.py;
  * the output is bit-identical, image by image, to the same images run in two pieces of which the first selects <1,2,1> (86-127 tiles), and in pieces of at most 85
    tiles, which select <1,1,9>: a layer's bits do not depend on the form its size selects.
The recorded kernel names confirm which form ran."""
import pytest
import torch

from test_conv3x3_one_column_rule_cpu import ONE, SPLIT9, THREE, c3_kernel_rule
from test_gpu_infer_ops import EXACT_ACTS, RANDOM_ACTS, _act, _below_2_24, _c3_problem, _ran, _same, hop    # noqa: F401 (hop: the fixture)
from f64_bar import bar

pytestmark = pytest.mark.gpu

# id: (B, H, W), resample modes, the form the rule selects
CASES = {
    "c1-128tiles": ((165, 9, 11), (0,), ONE),           # 16 335 pixels: exactly 128 tiles, cuts mid-row and mid-image, the last tile ragged (79 pixels)
    "c1-127tiles": ((164, 9, 11), (0,), THREE),         # one image fewer: 127 tiles, the three columns stay
    "c1-rs": ((136, 10, 12), (1, 2), ONE),              # 16 320 pixels, 128 tiles, both fused resample-adds
    "c1-26x26": ((25, 26, 26), (0,), ONE),              # the benchmark's map, 133 tiles
}


def _run(hop, x, x2, w, b, act, mode, want):
    xd, wd, bd, x2d = x.cuda(), w.cuda(), b.cuda(), x2.cuda() if x2 is not None else None
    y, names = _ran(hop, lambda: hop.op_conv3x3(xd, wd, bd, act, x2=x2d, resample=mode))
    assert names == [want], names
    return y


@pytest.mark.parametrize("case", list(CASES))
def test_one_column_exact(hop, case):
    shape, modes, want = CASES[case]
    assert c3_kernel_rule(96, 96, *shape, False) == want
    for mode in modes:
        x, x2, w, b, p64, _, mag = _c3_problem(96, 96, shape, mode, "exact")
        _below_2_24(mag, case)
        for act in EXACT_ACTS:
            _same(_run(hop, x, x2, w, b, act, mode, want), _act(p64, act), "%s rs%d act%d" % (case, mode, act))


@pytest.mark.parametrize("case", list(CASES))
def test_one_column_random(hop, case):
    shape, modes, want = CASES[case]
    for mode in modes:
        x, x2, w, b, p64, p32, _ = _c3_problem(96, 96, shape, mode, "random")
        for act in RANDOM_ACTS:
            bar("c3split", "%s rs%d act%d" % (case, mode, act), _run(hop, x, x2, w, b, act, mode, want), _act(p64, act), _act(p32, act))


@pytest.mark.parametrize("case", list(CASES))
def test_bits_do_not_depend_on_the_form(hop, case):
    (B, H, W), modes, want = CASES[case]
    act = 2
    for mode in modes:
        x, x2, w, b, _, _, _ = _c3_problem(96, 96, (B, H, W), mode, "random")
        y = _run(hop, x, x2, w, b, act, mode, want)
        cut = lambda t, i, j: None if t is None else t[i:j]
        na = -(-86 * 128 // (H * W))                         # the fewest images that make 86 tiles: the first piece runs as three columns
        assert c3_kernel_rule(96, 96, na, H, W, False) == THREE and 0 < B - na
        for i, j in ((0, na), (na, B)):
            piece = _run(hop, x[i:j], cut(x2, i, j), w, b, act, mode, c3_kernel_rule(96, 96, j - i, H, W, False))
            assert torch.equal(piece, y[i:j]), "%s rs%d: images %d..%d differ from their own run" % (case, mode, i, j)
        per = 85 * 128 // (H * W)                            # images per piece: at most 85 tiles
        assert c3_kernel_rule(96, 96, per, H, W, False) == SPLIT9
        for i in range(0, B, per):
            piece = _run(hop, x[i:i + per], cut(x2, i, i + per), w, b, act, mode, SPLIT9)
            assert torch.equal(piece, y[i:i + per]), "%s rs%d: images %d.. differ from the <1,1,9> run" % (case, mode, i)
