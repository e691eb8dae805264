"""launch_conv3x3's rule for the split-f16 family between 128 and 255 tiles of 128 pixels (26x26 at bs 32: 169), restated: inside the `tiles * 3 >= 256` branch the
one-column form conv3x3_split_kernel<3,2> takes the launch when there is a tile for at least every second CU (tiles * 2 >= 256); below that the three block columns of
<1,2,1> stay.  Every other launch keeps the form tests/infer_op_cases.py::c3_kernel states; tests/test_gpu_conv3x3_one_column.py takes its expected names from
c3_kernel_rule below."""
import os
import re

import infer_op_cases as ioc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "kernels_conv.hip")).read()

THREE, ONE, SPLIT9 = "conv3x3_split_kernel<1,2>", "conv3x3_split_kernel<3,2>", "conv3x3_split_kernel<1,1,9>"


def c3_kernel_rule(cin, cout, B, H, W, exact_f32):
    k = ioc.c3_kernel(cin, cout, B, H, W, exact_f32)
    return ONE if k == THREE and ioc.c3_tiles(B, H, W) * 2 >= 256 else k


def test_every_c3_case_keeps_its_kernel():
    for name, (cin, cout, (B, H, W), exact, _) in ioc.C3_CASES.items():
        assert c3_kernel_rule(cin, cout, B, H, W, exact) == ioc.c3_kernel(cin, cout, B, H, W, exact), name
    assert ioc.c3_tiles(*ioc.C3_CASES["c3s-86tiles"][2]) == 86            # the one case inside the branch: below the rule


def test_the_benchmark_maps():
    assert c3_kernel_rule(96, 96, 32, 26, 26, False) == ONE and ioc.c3_kernel(96, 96, 32, 26, 26, False) == THREE       # smooth_0 / smooth_2: 169 tiles
    assert c3_kernel_rule(96, 96, 32, 52, 52, False) == ONE               # smooth_1, as before
    assert c3_kernel_rule(96, 96, 32, 13, 13, False) == SPLIT9            # smooth_3, as before
    assert c3_kernel_rule(96, 96, 32, 26, 26, True) == ioc.c3_kernel(96, 96, 32, 26, 26, True)       # the f32 family is not touched


def test_edges_of_the_rule():
    assert ioc.c3_tiles(24, 26, 26) == 127 and c3_kernel_rule(96, 96, 24, 26, 26, False) == THREE
    assert ioc.c3_tiles(25, 26, 26) == 133 and c3_kernel_rule(96, 96, 25, 26, 26, False) == ONE
    assert ioc.c3_tiles(165, 9, 11) == 128 and c3_kernel_rule(96, 96, 165, 9, 11, False) == ONE           # 16 335 pixels: exactly 128 tiles, the last one ragged
    assert ioc.c3_tiles(164, 9, 11) == 127 and c3_kernel_rule(96, 96, 164, 9, 11, False) == THREE
    assert ioc.c3_tiles(48, 26, 26) == 254 and c3_kernel_rule(96, 96, 48, 26, 26, False) == ONE           # the upper edge is the branch's own: from 256 tiles <3,2> anyway
    assert ioc.c3_tiles(16, 26, 26) == 85 and c3_kernel_rule(96, 96, 16, 26, 26, False) == SPLIT9


def test_the_source_states_this_rule():
    flat = re.sub(r"\s+", "", re.sub(r"//[^\n]*", "", SRC))
    branch = flat[flat.index("}elseif(tiles*3>=256){"):flat.index("}elseif(conv3x3_split_lds(a.W,1,1,9)<=160*1024){")]
    assert branch.startswith("}elseif(tiles*3>=256){if(tiles*2>=256){g_last_kernel=\"conv3x3_split_kernel<3,2>\";"
                             "hipLaunchKernelGGL((conv3x3_split_kernel<3,2>),dim3(xcd_grid(tiles),1),dim3(256),conv3x3_split_lds(a.W,3,2),s,a);return;}"
                             "g_last_kernel=\"conv3x3_split_kernel<1,2>\";"), branch[:400]
