"""The case tables of tests/test_gpu_infer_ops.py and, next to them, a restatement in Python of the rules by which the launchers of
csrc/kernels_conv.hip pick a kernel from the shape (launch_dw, launch_conv3x3, launch_stem_pool's tile grid, launch_maxpool's block cap).
tests/test_infer_ops_cases_cpu.py asserts without a GPU that the tables reach every variant; every GPU case then asserts that the kernel
which ran is the one the restatement names, so a moved threshold fails loudly instead of quietly testing another kernel.

All tensors are NHWC on the device; a shape below is (B, H, W) of the input.
"""

# =====================================================================================================================================
# depthwise 3x3: dwconv3x3_kernel<STRIDE, VEC, R>
# =====================================================================================================================================
DW_LONG_BLOCKS = 1024                                        # a long-run variant needs this many 256-thread blocks


def dw_variant(C, stride, B, H, W):
    """launch_dw's choice (STRIDE, VEC, R) for a dense [B,H,W,C] tensor (row strides = C, channel offsets 0)"""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    v4 = C % 4 == 0
    blocks_for = lambda vec, r: (B * Ho * ((Wo + r - 1) // r) * (C // vec) + 255) // 256
    if stride == 1:
        if v4:
            return (1, 4, 4) if blocks_for(4, 4) >= DW_LONG_BLOCKS else (1, 4, 2)
        return (1, 2, 8) if blocks_for(2, 8) >= DW_LONG_BLOCKS else (1, 2, 4)
    if v4:
        return (2, 4, 4) if blocks_for(4, 4) >= DW_LONG_BLOCKS else (2, 4, 2)
    return (2, 2, 4) if blocks_for(2, 4) >= DW_LONG_BLOCKS else (2, 2, 2)


def dw_kernel(variant):
    return "dwconv3x3_kernel<%d,%d,%d>" % variant


DW_VARIANTS = [(1, 4, 4), (1, 4, 2), (1, 2, 8), (1, 2, 4), (2, 4, 4), (2, 4, 2), (2, 2, 4), (2, 2, 2)]

# id: C, stride, (B, H, W).  Short-run variants: Wo = R - 1, R, R + 1, 2R + 1; strips H = 1 and W = 1 (both column clamps on the same column); odd
# extents at stride 2; always B >= 2 (a wrong row clamp reads the neighbouring image).  Long-run variants: the smallest tensors the rule allows.
DW_CASES = {
    # <1,4,2>: R = 2, Wo = W = 1, 2, 3, 5
    "dw24-s1-w1": (24, 1, (2, 5, 1)),
    "dw24-s1-w2": (24, 1, (2, 4, 2)),
    "dw24-s1-w3-h1": (24, 1, (2, 1, 3)),
    "dw116-s1-w5": (116, 1, (3, 5, 5)),
    # <1,2,4>: R = 4, W = 1, 3, 4, 5, 9
    "dw58-s1-w1": (58, 1, (2, 3, 1)),
    "dw58-s1-w3": (58, 1, (2, 4, 3)),
    "dw58-s1-w4": (58, 1, (2, 3, 4)),
    "dw58-s1-w5-h1": (58, 1, (2, 1, 5)),
    "dw58-s1-w9": (58, 1, (3, 5, 9)),
    # <2,4,2>: R = 2, Wo = 1, 2, 3, 5 (W = 1, 4, 5, 9 / 10)
    "dw116-s2-w1": (116, 2, (2, 5, 1)),
    "dw116-s2-w4": (116, 2, (2, 7, 4)),
    "dw24-s2-w5-h1": (24, 2, (2, 1, 5)),
    "dw232-s2-w9": (232, 2, (2, 9, 9)),
    "dw116-s2-w10": (116, 2, (3, 6, 10)),
    # <2,2,2>: R = 2, Wo = 1, 2, 3, 5 (W = 1, 3, 6, 9)
    "dw58-s2-w1": (58, 2, (2, 3, 1)),
    "dw58-s2-w3": (58, 2, (2, 4, 3)),
    "dw58-s2-w6-h1": (58, 2, (2, 1, 6)),
    "dw58-s2-w9": (58, 2, (3, 7, 9)),
    # the long-run variants (>= 1024 blocks): 1044, 1031, 1048 and 1033 blocks; the last run of every row is partial (one pixel)
    "dw232-s1-long": (232, 1, (2, 48, 189)),
    "dw58-s1-long": (58, 1, (2, 70, 513)),
    "dw464-s2-long": (464, 2, (2, 67, 265)),
    "dw58-s2-long": (58, 2, (2, 135, 529)),
    # the branch widths of the 1.5x / 2.0x backbones (88 / 176 / 352 and 122 / 244 / 488): each at both strides, Wo on the same marks around R,
    # odd H and W at stride 2.  C = 122 is the wide backbones' only channel count that is no multiple of 4: the 2-channel variants
    "dw88-s1-w3": (88, 1, (2, 4, 3)),                        # <1,4,2>, Wo = R + 1
    "dw88-s2-w5": (88, 2, (2, 5, 5)),                        # <2,4,2>, Wo = 3
    "dw122-s1-w5": (122, 1, (2, 3, 5)),                      # <1,2,4>, Wo = R + 1
    "dw122-s1-w9": (122, 1, (3, 5, 9)),                      # <1,2,4>, Wo = 2R + 1
    "dw122-s2-w5": (122, 2, (2, 5, 5)),                      # <2,2,2>, Wo = 3
    "dw122-s2-w9": (122, 2, (3, 7, 9)),                      # <2,2,2>, Wo = 5
    "dw244-s1-w5": (244, 1, (2, 3, 5)),                      # <1,4,2>, Wo = 2R + 1
    "dw244-s2-w7": (244, 2, (2, 7, 7)),                      # <2,4,2>, Wo = 4
    "dw352-s1-w2": (352, 1, (2, 3, 2)),                      # <1,4,2>, Wo = R
    "dw352-s2-w3": (352, 2, (2, 5, 3)),                      # <2,4,2>, Wo = R
    "dw488-s1-w3": (488, 1, (2, 5, 3)),                      # <1,4,2>, Wo = R + 1
    "dw488-s2-w9": (488, 2, (3, 9, 9)),                      # <2,4,2>, Wo = 2R + 1
}
DW_WIDE_C = (88, 122, 244, 352, 488)


def dw_last_run_partial(C, stride, B, H, W):
    Wo = (W - 1) // stride + 1
    return Wo % dw_variant(C, stride, B, H, W)[2] != 0


# =====================================================================================================================================
# dense 3x3: launch_conv3x3
# =====================================================================================================================================
LDS_MAX, LDS_HALF = 160 * 1024, 80 * 1024


def split_lds(W, NT, NH, TPS=1):
    return (2 * (128 + 2 * W + 2) * (96 // NH + 8) + TPS * 2 * 6 * (32 * NT) * 8) * 2


def halo_tap_lds(W, Cin, NT, split=1):
    npix = 128 + 2 * W + 2
    return (((npix * (Cin + 2) + 3) & ~3) + (Cin // 2 // split) * (32 * NT * 2)) * 4


def halo_lds(W, Cin, NT):
    npix = 128 + 2 * W + 2
    return (((npix * (Cin + 2) + 3) & ~3) + 2 * 16 * (32 * NT * 2)) * 4


def c3_tiles(B, H, W):
    return (B * H * W + 127) // 128


def c3_kernel(Cin, Cout, B, H, W, exact_f32):
    """launch_conv3x3's choice, as the symbol the profile records, for a dense input (in_ld = Cin, out_ld = Cout, offsets 0).  exact_f32: the handle
    mode that withholds the split-f16 weight packs (the same happens when a weight is outside the f16 range)."""
    Npad = (Cout + 31) // 32 * 32
    nt32 = Npad // 32
    NT = 3 if nt32 >= 3 and nt32 % 3 == 0 else (2 if nt32 % 2 == 0 else 1)
    tiles = c3_tiles(B, H, W)
    vec_out = Cout % 4 == 0                                  # 16-byte stores: N, out_ld (= Cout here) multiples of 4
    if not exact_f32 and Cin == 96 and Npad == 96 and vec_out and split_lds(W, 1, 1) <= LDS_MAX:
        if tiles >= 256:
            return "conv3x3_split_kernel<3,2>"
        if tiles * 3 >= 256:
            return "conv3x3_split_kernel<1,2>"               # <1,2,1>: the recorded symbol leaves the default TPS = 1 out
        if split_lds(W, 1, 1, 9) <= LDS_MAX:
            return "conv3x3_split_kernel<1,1,9>"
        if split_lds(W, 1, 1, 3) <= LDS_MAX:
            return "conv3x3_split_kernel<1,1,3>"
        return "conv3x3_split_kernel<1,1,1>"
    if Cin == 96 and NT == 3 and vec_out and halo_tap_lds(W, 96, 3) <= LDS_MAX:
        if tiles * (Npad // 96) >= 256:
            return "conv3x3_halo_tap_kernel<3,96,1>"
        if halo_tap_lds(W, 96, 1) > LDS_HALF and halo_tap_lds(W, 96, 1, 2) <= LDS_HALF:
            return "conv3x3_halo_tap_kernel<1,96,2>"
        return "conv3x3_halo_tap_kernel<1,96,1>"
    if Cin % 32 == 0 and halo_lds(W, Cin, NT) <= LDS_MAX and Cin // 2 <= 256:
        return "conv3x3_halo_kernel<%d>" % NT
    return "gemm_conv_kernel<4,1,3,1,16,2>" if nt32 % 3 == 0 else "gemm_conv_kernel<4,1,1,1,16,2>"


C3_KERNELS = ["conv3x3_split_kernel<3,2>", "conv3x3_split_kernel<1,2>", "conv3x3_split_kernel<1,1,9>", "conv3x3_split_kernel<1,1,3>",
              "conv3x3_split_kernel<1,1,1>", "conv3x3_halo_tap_kernel<3,96,1>", "conv3x3_halo_tap_kernel<1,96,2>", "conv3x3_halo_tap_kernel<1,96,1>",
              "conv3x3_halo_kernel<1>", "conv3x3_halo_kernel<2>", "conv3x3_halo_kernel<3>", "gemm_conv_kernel<4,1,3,1,16,2>",
              "gemm_conv_kernel<4,1,1,1,16,2>"]

# id: Cin, Cout, (B, H, W), exact_f32 handle mode, fused resample modes to run (0 = plain; 1 = + up2(x2), x2 [B,H/2,W/2]; 2 = + down(x2), x2 [B,2H,2W])
C3_CASES = {
    # split-f16 family (the network's 96 -> 96 neck convs)
    "c3s-1tile": (96, 96, (2, 7, 6), False, (0,)),                       # <1,1,9>, M = 84
    "c3s-1tile-rs": (96, 96, (2, 6, 8), False, (1, 2)),                  # <1,1,9>, M = 96, both resample-adds
    "c3s-3tiles": (96, 96, (3, 9, 11), False, (0,)),                     # <1,1,9>, M = 297: tile cuts at 128 / 256, mid-row (11 columns) and mid-image (99 pixels)
    "c3s-3tiles-rs": (96, 96, (3, 10, 12), False, (1, 2)),               # <1,1,9>, M = 360
    "c3s-w65": (96, 96, (2, 3, 65), False, (0,)),                        # <1,1,9> at its widest map
    "c3s-w66": (96, 96, (2, 3, 66), False, (0,)),                        # <1,1,3> at its narrowest
    "c3s-w70": (96, 96, (2, 3, 70), False, (0,)),                        # <1,1,3>
    "c3s-w109": (96, 96, (2, 2, 109), False, (0,)),                      # <1,1,3> at its widest
    "c3s-w110": (96, 96, (2, 2, 110), False, (0,)),                      # <1,1,1> at its narrowest
    "c3s-w112": (96, 96, (2, 3, 112), False, (0,)),                      # <1,1,1>
    "c3s-w124": (96, 96, (2, 2, 124), False, (0,)),                      # <1,1,1> at the widest map the family takes
    "c3s-86tiles": (96, 96, (3, 61, 60), False, (0,)),                   # <1,2,1>: 86 tiles, the last one ragged (100 pixels)
    "c3s-257tiles": (96, 96, (5, 81, 81), False, (0,)),                  # <3,2>: 257 tiles, the last one ragged (37 pixels)
    "c3s-n80": (96, 80, (3, 9, 11), False, (0,)),                        # <1,1,9>, the column mask of the epilogue live (Npad = 96)
    # f32-MFMA family: what exact_f32 and the range-guard fallback run
    "c3t-1tile": (96, 96, (2, 7, 6), True, (0,)),                        # <1,96,1>
    "c3t-3tiles-rs": (96, 96, (3, 10, 12), True, (0, 1, 2)),             # <1,96,1>
    "c3t-w23": (96, 96, (2, 3, 23), True, (0,)),                         # <1,96,1> below the half-tap window
    "c3t-w24": (96, 96, (2, 3, 24), True, (0,)),                         # <1,96,2> at W = 24 ...
    "c3t-26x26": (96, 96, (2, 26, 26), True, (0,)),                      # <1,96,2>, the map it was written for
    "c3t-w31": (96, 96, (2, 3, 31), True, (0,)),                         # ... and 31
    "c3t-w32": (96, 96, (2, 3, 32), True, (0,)),                         # <1,96,1> above it
    "c3t-w96": (96, 96, (2, 2, 96), True, (0,)),                         # <1,96,1> at the widest map of the tap kernels
    "c3t-n192": (96, 192, (3, 9, 11), True, (0,)),                       # <1,96,1>, six block columns
    "c3t-n80": (96, 80, (3, 9, 11), True, (0,)),                         # <1,96,1>, column mask live
    "c3t-257tiles": (96, 96, (5, 81, 81), True, (0,)),                   # <3,96,1>
    # conv3x3_halo_kernel<NT>: channel counts other than the neck's
    "c3h-32-32": (32, 32, (3, 10, 12), False, (0, 1, 2)),                # <1>
    "c3h-64-64": (64, 64, (3, 9, 11), False, (0,)),                      # <2>
    "c3h-32-96": (32, 96, (3, 9, 11), False, (0,)),                      # <3>
    "c3h-64-160": (64, 160, (2, 7, 6), False, (0,)),                     # <1>, five block columns
    "c3h-96-75": (96, 75, (3, 9, 11), False, (0,)),                      # <3>: an odd Cout keeps the 96-channel kernels' 16-byte stores out; column mask live
    "c3h-96-96-w97": (96, 96, (2, 2, 97), True, (0,)),                   # <3>: the f32 family beyond the tap kernels' LDS
    "c3h-96-96-w112": (96, 96, (2, 2, 112), True, (0,)),                 # <3> at its widest map
    # gemm_conv_kernel, MODE 1 (im2col on the fly): maps too wide / too deep for an LDS-resident halo
    "c3g-96-96-w113": (96, 96, (2, 2, 113), True, (0,)),                 # <4,1,3>
    "c3g-96-96-w125": (96, 96, (2, 2, 125), False, (0,)),                # <4,1,3>: the split family's LDS limit
    "c3g-256-96": (256, 96, (3, 10, 12), False, (0, 1, 2)),              # <4,1,3>
    "c3g-256-32": (256, 32, (3, 9, 11), False, (0,)),                    # <4,1,1>
    "c3g-96-64-w124": (96, 64, (2, 2, 124), False, (0,)),                # <4,1,1>
}

# =====================================================================================================================================
# stem (stem_kernel), stem + max pool (stem_pool_kernel: 8 x 7 pooled pixels per block from a 17 x 15 conv tile), max pool
# =====================================================================================================================================
STEM_CASES = {"stem-32x32-b1": (1, 32, 32), "stem-32x32-b3": (3, 32, 32), "stem-34x30-b1": (1, 34, 30), "stem-33x34-b3": (3, 33, 34)}   # Wo = 16, 16, 15, 17

POOL_TILE = (8, 7)                                           # pooled rows, columns of one block


def stem_pool_extents(H, W):
    """(Hc, Wc) of the conv output, (Hp, Wp) of the pooled output"""
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (Hc, Wc), ((Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1)


STEM_POOL_CASES = {
    "sp-32": (2, 32, 32),                                    # 8 x 8 pooled: one row tile, a second column tile of one column
    "sp-64": (2, 64, 64),                                    # 16 x 16: two full row tiles, three column tiles, the last ragged (2 columns)
    "sp-96": (2, 96, 96),                                    # 24 x 24
    "sp-33x23": (2, 33, 23),                                 # Hp = 9 from an odd conv extent (Hc = 17), Wp = 6
    "sp-27x26": (2, 27, 26),                                 # Hp = 7, Wp = 7 (Wc = 13)
    "sp-30x31": (3, 30, 31),                                 # Hp = 8, Wp = 8
    "sp-25x58": (2, 25, 58),                                 # Hp = 7, Wp = 15 (Hc = 13, Wc = 29)
    "sp-3x5": (2, 3, 5),                                     # a map smaller than one tile: 1 x 2 pooled
}

MAXPOOL_MAX_BLOCKS = 256 * 32
# id: (B, H, W, C)
MAXPOOL_CASES = {
    "mp-8x8-c24": (2, 8, 8, 24), "mp-7x9-c24": (2, 7, 9, 24), "mp-10x7-c4": (2, 10, 7, 4), "mp-h1-c4": (2, 1, 9, 4), "mp-w1-c24": (2, 6, 1, 24),
    "mp-1x1-c4": (3, 1, 1, 4),
    "mp-2nd-pass": (2, 837, 838, 24),                        # 2 106 732 threads against 256 * 32 blocks of 256: 9 580 take a second turn
}


def maxpool_threads(B, H, W, C):
    return B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * (C // 4)


# =====================================================================================================================================
# pointwise: the shape list of test_op_pointwise_shapes_vs_oracle (M, Cin, Cout, act), first configuration of each family
# =====================================================================================================================================
PW_CASES = [(1, 58, 58, 1), (127, 116, 116, 1), (129, 232, 232, 1), (1000, 464, 96, 2), (333, 24, 58, 1), (4096, 96, 255, 0), (77, 48, 24, 1), (5000, 96, 96, 2)]
# the 1.5x (176 / 352 / 704, bf 88 / 176 / 352) and 2.0x (244 / 488 / 976, bf 122 / 244 / 488) networks: the unit GEMMs (K = N = bf), the GEMMs that enter a
# stage (cin != cout: stage 2's pw1 and branch 1's pw read the stem's 24 channels; stages 3 / 4 enter with K = N = the unit list's 176 ... 488, the halved
# N here are the same K against a narrower last tile) and the laterals of all three stages.  Ragged M throughout; N = 88 leaves 8, N = 122 six, N = 244 twelve and
# N = 488 twenty-four masked columns of the last 32-column tile, K = 122 / 244 / 488 end inside an octet pair of the split operands
PW_WIDE_UNIT = [(129, 88, 88, 1), (127, 122, 122, 1), (65, 176, 176, 1), (129, 244, 244, 1), (33, 352, 352, 1), (130, 488, 488, 1)]
PW_WIDE_ENTRY = [(333, 24, 88, 1), (333, 24, 122, 1), (77, 176, 88, 1), (77, 244, 122, 1), (66, 352, 176, 1), (66, 488, 244, 1)]
PW_WIDE_LATERAL = [(200, 704, 96, 2), (200, 976, 96, 2), (100, 176, 96, 2), (100, 352, 96, 2), (100, 244, 96, 2), (100, 488, 96, 2)]
PW_WIDE_CASES = PW_WIDE_UNIT + PW_WIDE_ENTRY + PW_WIDE_LATERAL
PW_FIRST_KERNEL = ("gemm_conv_kernel<4,1,1,0,16,2>", "gemm_split_kernel<4,1,1,32>")      # f32-MFMA family, split-f16 family
