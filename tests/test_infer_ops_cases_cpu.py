"""The case tables of tests/infer_op_cases.py reach every kernel variant that tests/test_gpu_infer_ops.py is there for (by the restated
dispatch rules; the GPU cases then assert that the named kernel is the one that ran), and the restated LDS formulas and thresholds are
the ones csrc/kernels_conv.hip states."""
import os
import re

import infer_op_cases as ioc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "kernels_conv.hip")).read()


def test_depthwise_cases_reach_all_eight_variants():
    by_variant = {}
    for name, (C, stride, (B, H, W)) in ioc.DW_CASES.items():
        assert B >= 2 and C % 2 == 0, name
        by_variant.setdefault(ioc.dw_variant(C, stride, B, H, W), []).append(name)
    assert sorted(by_variant) == sorted(ioc.DW_VARIANTS)
    for v, names in by_variant.items():
        assert any(ioc.dw_last_run_partial(*ioc.DW_CASES[n][:2], *ioc.DW_CASES[n][2]) for n in names), "no partial last run for %s" % (v,)
    # the short-run variants at Wo = R - 1, R, R + 1, 2R + 1, each with a one-row and a one-column strip
    for v in ((1, 4, 2), (1, 2, 4), (2, 4, 2), (2, 2, 2)):
        shapes = [(ioc.DW_CASES[n][1], ioc.DW_CASES[n][2]) for n in by_variant[v]]
        R = v[2]
        assert {R - 1, R, R + 1, 2 * R + 1} <= {(W - 1) // s + 1 for s, (_, _, W) in shapes}, v
        assert any(H == 1 for _, (_, H, _) in shapes) and any(W == 1 for _, (_, _, W) in shapes), v
    for v in ((2, 4, 2), (2, 2, 2)):                         # odd extents at stride 2
        assert any(ioc.DW_CASES[n][2][1] % 2 and ioc.DW_CASES[n][2][2] % 2 and ioc.DW_CASES[n][2][1] > 1 for n in by_variant[v]), v
    # the long-run cases are as small as the rule allows: a few blocks above the threshold, no tensor above ~16 M floats
    for n in ("dw232-s1-long", "dw58-s1-long", "dw464-s2-long", "dw58-s2-long"):
        C, stride, (B, H, W) = ioc.DW_CASES[n]
        st, vec, R = ioc.dw_variant(C, stride, B, H, W)
        blocks = (B * ((H - 1) // st + 1) * (((W - 1) // st + 1 + R - 1) // R) * (C // vec) + 255) // 256
        assert ioc.DW_LONG_BLOCKS <= blocks < ioc.DW_LONG_BLOCKS + 32 and B * H * W * C <= 17 * 2 ** 20, (n, blocks)


def test_depthwise_cases_cover_the_wide_branch_widths():
    """C = 88 / 176 / 352 (1.5x) and 122 / 244 / 488 (2.0x): each wide width the table names runs at both strides with B >= 2 and odd H and W at stride 2;
    122 - no multiple of 4 - is what brings the 2-channel variants to a wide backbone."""
    assert ioc.DW_WIDE_C == (88, 122, 244, 352, 488)
    for C in ioc.DW_WIDE_C:
        mine = [c for c in ioc.DW_CASES.values() if c[0] == C]
        assert {c[1] for c in mine} == {1, 2}, C
        assert all(c[2][0] >= 2 for c in mine), C
        assert any(c[1] == 2 and c[2][1] % 2 and c[2][2] % 2 and c[2][1] > 1 for c in mine), C
        vecs = {ioc.dw_variant(c[0], c[1], *c[2])[1] for c in mine}
        assert vecs == ({2} if C % 4 else {4}), C
    two = {ioc.dw_variant(c[0], c[1], *c[2]) for c in ioc.DW_CASES.values() if c[0] == 122}
    assert two == {(1, 2, 4), (2, 2, 2)}
    R = {1: 4, 2: 2}
    for stride in (1, 2):                                    # and the 2-channel cases of 122 sit past one run: a partial last run
        assert any(dw_wo(c) > R[stride] and dw_wo(c) % R[stride] for c in ioc.DW_CASES.values() if c[0] == 122 and c[1] == stride)


def dw_wo(case):
    C, stride, (B, H, W) = case
    return (W - 1) // stride + 1


def test_pointwise_wide_cases_hold_every_width_of_the_wide_networks():
    from yolo_nano_amd import arch
    have = set(ioc.PW_WIDE_CASES)
    assert len(have) == len(ioc.PW_WIDE_CASES) and not have & set(ioc.PW_CASES)
    need = set()                                             # every (K, N) a pointwise layer of the two backbones and their laterals has
    for bb in ("1.5x", "2.0x"):
        cin = 24
        for C in arch.STAGE_CH[bb]:
            need |= {(C // 2, C // 2), (cin, C // 2), (C, 96)}
            cin = C
    assert need <= {(k, n) for _, k, n, _ in ioc.PW_WIDE_CASES}, need - {(k, n) for _, k, n, _ in ioc.PW_WIDE_CASES}
    assert set(ioc.PW_WIDE_CASES) >= {(129, 88, 88, 1), (127, 122, 122, 1), (65, 176, 176, 1), (129, 244, 244, 1), (33, 352, 352, 1), (130, 488, 488, 1),
                                      (333, 24, 88, 1), (333, 24, 122, 1), (77, 176, 88, 1), (77, 244, 122, 1), (66, 352, 176, 1), (66, 488, 244, 1),
                                      (200, 704, 96, 2), (200, 976, 96, 2)}
    for M, k, n, act in ioc.PW_WIDE_CASES:
        assert M % 32 and k % 2 == 0 and n % 2 == 0, (M, k, n)           # ragged M; an even N: the shuffle entry runs too
        assert 9 * k + 3 < 2 ** 24                                       # integers in {-3..3}: exact in fp32 in any order
    assert all(M >= 64 and act == 2 for M, _, _, act in ioc.PW_WIDE_LATERAL)
    assert all(k == n for _, k, n, _ in ioc.PW_WIDE_UNIT) and all(k != n for _, k, n, _ in ioc.PW_WIDE_ENTRY)
    assert max(k for _, k, _, _ in ioc.PW_WIDE_CASES) == 976 and max(n for _, _, n, _ in ioc.PW_WIDE_CASES) == 488


C3_EXPECT = {
    "c3s-1tile": "conv3x3_split_kernel<1,1,9>", "c3s-1tile-rs": "conv3x3_split_kernel<1,1,9>", "c3s-3tiles": "conv3x3_split_kernel<1,1,9>",
    "c3s-3tiles-rs": "conv3x3_split_kernel<1,1,9>", "c3s-w65": "conv3x3_split_kernel<1,1,9>", "c3s-w66": "conv3x3_split_kernel<1,1,3>",
    "c3s-w70": "conv3x3_split_kernel<1,1,3>", "c3s-w109": "conv3x3_split_kernel<1,1,3>", "c3s-w110": "conv3x3_split_kernel<1,1,1>",
    "c3s-w112": "conv3x3_split_kernel<1,1,1>", "c3s-w124": "conv3x3_split_kernel<1,1,1>", "c3s-86tiles": "conv3x3_split_kernel<1,2>",
    "c3s-257tiles": "conv3x3_split_kernel<3,2>", "c3s-n80": "conv3x3_split_kernel<1,1,9>",
    "c3t-1tile": "conv3x3_halo_tap_kernel<1,96,1>", "c3t-3tiles-rs": "conv3x3_halo_tap_kernel<1,96,1>", "c3t-w23": "conv3x3_halo_tap_kernel<1,96,1>",
    "c3t-w24": "conv3x3_halo_tap_kernel<1,96,2>", "c3t-26x26": "conv3x3_halo_tap_kernel<1,96,2>", "c3t-w31": "conv3x3_halo_tap_kernel<1,96,2>",
    "c3t-w32": "conv3x3_halo_tap_kernel<1,96,1>", "c3t-w96": "conv3x3_halo_tap_kernel<1,96,1>", "c3t-n192": "conv3x3_halo_tap_kernel<1,96,1>",
    "c3t-n80": "conv3x3_halo_tap_kernel<1,96,1>", "c3t-257tiles": "conv3x3_halo_tap_kernel<3,96,1>",
    "c3h-32-32": "conv3x3_halo_kernel<1>", "c3h-64-64": "conv3x3_halo_kernel<2>", "c3h-32-96": "conv3x3_halo_kernel<3>", "c3h-64-160": "conv3x3_halo_kernel<1>",
    "c3h-96-75": "conv3x3_halo_kernel<3>", "c3h-96-96-w97": "conv3x3_halo_kernel<3>", "c3h-96-96-w112": "conv3x3_halo_kernel<3>",
    "c3g-96-96-w113": "gemm_conv_kernel<4,1,3,1,16,2>", "c3g-96-96-w125": "gemm_conv_kernel<4,1,3,1,16,2>", "c3g-256-96": "gemm_conv_kernel<4,1,3,1,16,2>",
    "c3g-256-32": "gemm_conv_kernel<4,1,1,1,16,2>", "c3g-96-64-w124": "gemm_conv_kernel<4,1,1,1,16,2>",
}


def _c3(name):
    cin, cout, (B, H, W), exact, _ = ioc.C3_CASES[name]
    return ioc.c3_kernel(cin, cout, B, H, W, exact)


def test_dense3x3_cases_reach_all_thirteen_kernels():
    assert sorted(C3_EXPECT) == sorted(ioc.C3_CASES)
    for name, kernel in C3_EXPECT.items():
        assert _c3(name) == kernel, name
    assert {_c3(n) for n in ioc.C3_CASES} == set(ioc.C3_KERNELS) and len(ioc.C3_KERNELS) == 13
    for name, (cin, cout, (B, H, W), _, modes) in ioc.C3_CASES.items():
        assert cin % 32 == 0 and B >= 2, name
        if set(modes) & {1, 2}:
            assert H % 2 == 0 and W % 2 == 0, name           # a + up2(x2) needs even extents
    # what the issue asks of the cases beyond one per kernel
    tiles = lambda n: ioc.c3_tiles(*ioc.C3_CASES[n][2])
    rs = lambda n: {1, 2} <= set(ioc.C3_CASES[n][4])
    split9 = [n for n in ioc.C3_CASES if _c3(n) == "conv3x3_split_kernel<1,1,9>"]
    assert any(tiles(n) == 1 and rs(n) for n in split9) and any(tiles(n) > 1 and rs(n) for n in split9)
    assert any(rs(n) for n in ioc.C3_CASES if _c3(n).startswith("conv3x3_halo_tap_kernel"))
    B, H, W = ioc.C3_CASES["c3s-3tiles"][2]
    assert 128 % W and 128 % (H * W) and tiles("c3s-3tiles") == 3      # the tile cuts fall mid-row and mid-image
    assert 86 <= tiles("c3s-86tiles") < 256 <= tiles("c3s-257tiles")
    assert any(ioc.C3_CASES[n][1] % 32 for n in ioc.C3_CASES)        # a live column mask
    halo = {ioc.C3_CASES[n][:2] for n in ioc.C3_CASES if _c3(n).startswith("conv3x3_halo_kernel")}
    assert any(ci != 96 and (co // 32) % 2 == 1 and (co // 32) % 3 for ci, co in halo) and any(ci != 96 and (co // 32) % 2 == 0 for ci, co in halo) and \
        any(ci != 96 and (co // 32) % 3 == 0 for ci, co in halo)


def test_restated_rules_are_the_ones_the_source_states():
    """The formulas and limits are compared as text (white space aside): an edit of a launcher's rule has to be followed here."""
    flat = re.sub(r"\s+", "", SRC)
    for piece in (
            "conv3x3_split_lds(intW,intNT,intNH,intTPS=1){return((size_t)2*(128+2*W+2)*(96/NH+8)+(size_t)TPS*2*6*(32*NT)*8)*2;}",
            "return((size_t)((npix*(Cin+2)+3)&~3)+(size_t)(Cin/2/split)*(32*NT*2))*sizeof(float);",
            "return((size_t)((npix*(Cin+2)+3)&~3)+2*16*(32*NT*2))*sizeof(float);",
            "constintNT=nt32>=3&&nt32%3==0?3:(nt32%2==0?2:1);",
            "conv3x3_split_lds(a.W,1,1)<=160*1024){", "if(tiles>=256){", "}elseif(tiles*3>=256){", "}elseif(conv3x3_split_lds(a.W,1,1,9)<=160*1024){",
            "}elseif(conv3x3_split_lds(a.W,1,1,3)<=160*1024){", "conv3x3_halo_tap_lds(a.W,96,3)<=160*1024){", "if(tiles*(a.Npad/96)>=256){",
            "}elseif(conv3x3_halo_tap_lds(a.W,96,1)>80*1024&&conv3x3_halo_tap_lds(a.W,96,1,2)<=80*1024){", "if(lds<=160*1024&&a.K/2<=256){",
            "autoblocks_for=[&](intvec,intr){return((long)a.B*Ho*((Wo+r-1)/r)*(a.C/vec)+255)/256;};",
            "if(v4){if(blocks_for(4,4)>=1024)YN_DW(1,4,4)elseYN_DW(1,4,2)}", "else{if(blocks_for(2,8)>=1024)YN_DW(1,2,8)elseYN_DW(1,2,4)}",
            "if(v4){if(blocks_for(4,4)>=1024)YN_DW(2,4,4)elseYN_DW(2,4,2)}", "else{if(blocks_for(2,4)>=1024)YN_DW(2,2,4)elseYN_DW(2,2,2)}",
            "constexprintPR=8,PC=7,", "if(blocks>256*32)blocks=256*32;"):
        assert piece in flat, piece
    assert (ioc.LDS_MAX, ioc.LDS_HALF, ioc.DW_LONG_BLOCKS, ioc.POOL_TILE, ioc.MAXPOOL_MAX_BLOCKS) == (160 * 1024, 80 * 1024, 1024, (8, 7), 256 * 32)


def test_stem_and_pool_cases_sit_on_both_sides_of_every_edge():
    assert {B for B, _, _ in ioc.STEM_CASES.values()} == {1, 3}
    assert {((W - 1) // 2 + 1) % 2 for _, _, W in ioc.STEM_CASES.values()} == {0, 1}
    ext = {n: ioc.stem_pool_extents(H, W) for n, (_, H, W) in ioc.STEM_POOL_CASES.items()}
    assert all(B >= 2 for B, _, _ in ioc.STEM_POOL_CASES.values())
    assert {6, 7, 8, 15, 16, 24} <= {p[1] for _, p in ext.values()} and {7, 8, 9, 16, 24} <= {p[0] for _, p in ext.values()}
    assert ext["sp-33x23"][0][0] == 17 and any(c[1] % 2 for c, _ in ext.values())          # odd conv extents: the window of the last pooled pixel hangs over
    PR, PC = ioc.POOL_TILE
    assert ext["sp-64"][1] == (2 * PR, 16) and 16 % PC                                      # two full row tiles, a ragged third column tile
    assert any(p[0] < PR and p[1] < PC for _, p in ext.values())
    assert {C for _, _, _, C in ioc.MAXPOOL_CASES.values()} == {4, 24}
    assert any(H == 1 for _, H, _, _ in ioc.MAXPOOL_CASES.values()) and any(W == 1 for _, _, W, _ in ioc.MAXPOOL_CASES.values())
    assert {(H % 2, W % 2) for _, H, W, _ in ioc.MAXPOOL_CASES.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    big = [ioc.maxpool_threads(*c) for c in ioc.MAXPOOL_CASES.values() if ioc.maxpool_threads(*c) > ioc.MAXPOOL_MAX_BLOCKS * 256]
    assert len(big) == 1 and big[0] < ioc.MAXPOOL_MAX_BLOCKS * 256 * 1.01               # a second pass, and no larger than that takes
