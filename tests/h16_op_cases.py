"""The case tables of tests/test_gpu_train_h16_ops.py and, next to them, a restatement in Python of the rules by which the launchers of
csrc/kernels_h16.hip pick a kernel and a grid from the shape (launch_hgemm's NT, launch_hwgrad's tile and slice count, launch_hdw's five-way
choice and NR, hlanes_for, launch_hdw_wgrad's G).  tests/test_h16_ops_cases_cpu.py asserts without a GPU that the tables reach every
variant; every GPU case then asserts that the kernels which ran are the ones the restatement names, in order.

A launcher that issues two kernels records both names joined by "+" (hwgrad*_kernel+hwgrad_reduce_kernel, hcol_reduce_kernel<2>+hbn_bwd_kernel,
hstem_bwd_kernel<0>+hstem_bwd_kernel<1>); launch_hdw_wgrad adds the grid rows of its sum kernel in brackets ([1] below 64 workgroups, [16] from 64 on).

All tensors are NHWC; a shape below is (B, H, W) of the conv's input.  Channel maps as csrc/kernels_h16.hip: dense rows padded to a multiple
of 8 halves, a "gapped" 2 bf-channel unit tensor as two planes of roundup8(bf).
"""

GEMM_TILE_ROWS = 128          # hgemm_kernel's BM: the statistics epilogues sum fp32 over one such tile
WG_BLOCKS, WG_SLICE_ROWS, WG_MAX_SLICES = 2048, 512, 512      # launch_hwgrad
DW_R = 4                      # hdw_run_kernel / hdw_wgrad_kernel: output pixels per run
DW_GTARGET_STAT, DW_GTARGET = 256, 4096                        # launch_hdw: workgroups of runs with / without statistics
DW_WGRAD_GMAX, DW_WGRAD_RUNS = 2048, 4                         # launch_hdw_wgrad
STEM_BLOCK = 85               # pixels per workgroup of hstem_apply_pool_kernel / hstem_bwd_kernel
STEM_WGRAD_CHUNK = 64         # pixels per chunk of hstem_wgrad_kernel
FINISH_MAX_BLOCKS = 2048      # launch_hgrad_finish
PART_FLOATS = 4 << 20         # the op entries' weight-gradient scratch
GRAD_SLOTS = 8


def r8(c):
    return (c + 7) & ~7


def r32(c):
    return (c + 31) & ~31


def chan_map(C, gapped):
    """(half, gap, Cp) of C logical channels"""
    half = C // 2 if gapped else C
    return half, (r8(half) - half if gapped else 0), (2 * r8(half) if gapped else r8(C))


def hlanes_for(Cp):
    l = 1
    while l < (Cp >> 3) and l < 256:
        l <<= 1
    return l


def hgemm_nt(Npad):
    n32 = Npad // 32
    return 4 if n32 % 4 == 0 else (3 if n32 % 3 == 0 else (2 if n32 % 2 == 0 else 1))


def hgemm_kernel(Npad, taps, stat):
    return "hgemm_kernel<%d,%d,%d>" % (hgemm_nt(Npad), taps, stat)


def hwgrad_choice(M, Np, Kp, taps, cap):
    """launch_hwgrad: (TN, TK, slices, slices before the partial_cap clip)"""
    TN, TK = (2 if Np > 64 else 1), (2 if Kp > 64 else 1)
    gn, gk = -(-Np // (64 * TN)), -(-Kp // (64 * TK)) * taps
    slices = min(WG_BLOCKS // (gn * gk), WG_MAX_SLICES, -(-M // WG_SLICE_ROWS))
    free = max(slices, 1)
    nk = Np * Kp * taps
    if slices * nk > cap:
        slices = cap // nk
    return TN, TK, max(slices, 1), free


def hwgrad_kernel(Np, Kp, taps):
    TN, TK = (2 if Np > 64 else 1), (2 if Kp > 64 else 1)
    k = "hwgrad_kernel<%d>" % taps if (TN, TK) == (1, 1) else "hwgrad2_kernel<%d,%d,%d>" % (taps, TN, TK)
    return k + "+hwgrad_reduce_kernel"


def hwgrad_slice_rows(M, slices):
    """rows of one M slice (a multiple of the kernel's 64-row tile)"""
    return -(-(-(-M // slices)) // 64) * 64


def hdw_choice(Cp, stride, B, H, W, stat):
    """launch_hdw: (kernel, NR) - NR blocks of runs per workgroup, 0 for the one-pixel kernels"""
    if stride == 1 and Cp <= 256:
        PB = 256 // (Cp >> 3)
        runs = B * H * ((W + 3) // 4)
        nb1 = -(-runs // PB)
        cap = DW_GTARGET_STAT if stat else DW_GTARGET
        return "hdw_run_kernel<%d>" % stat, -(-nb1 // cap)
    return "hdw_kernel<%d>" % stride, 0


def hdw_wgrad_choice(Cp, C, stride, B, H, W, cap):
    """launch_hdw_wgrad: (kernel record, G, G before the part_cap clip)"""
    OL = hlanes_for(Cp)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    npix = B * Ho * ((Wo + 3) // 4)
    per = (256 // OL) * DW_WGRAD_RUNS
    free = max(min(-(-npix // per), DW_WGRAD_GMAX), 1)
    G = free
    if G * C * 9 > cap:
        G = cap // (C * 9)
    G = max(G, 1)
    return "hdw_wgrad_kernel<%d>+hdw_wgrad_sum_kernel[%d]" % (stride, 16 if G >= 64 else 1), G, free


# =====================================================================================================================================
# convolutions through yn_op_h16_conv2
# =====================================================================================================================================
PW, DW, C3 = 0, 1, 2
# id: kind, Cin, Cout, stride, (B, H, W), options:
#   gapped   the input is a two-plane unit tensor              plane  x AND dx are the second plane of a two-plane tensor of 2 Cin channels
#   acc      the values of `accumulate` to run (default (0,))  cap    partial_cap in copies of the launcher's own unit (Np Kp taps | 9 C)
#   bias     a bias (forward)                                  want   which gradients (default all three)
#   lim      the integers of the exact case lie in [-lim, lim] (default 3)
CONV_CASES = {
    # ---- pointwise: M = 1, 7, 127, 129, 297, 513, 1025 around the 128-row tile and the 512-row weight-gradient slice
    "pw24-58-m1": (PW, 24, 58, 1, (1, 1, 1), {}),
    "pw58-58-m7": (PW, 58, 58, 1, (1, 1, 7), {}),
    "pw58-116-m127": (PW, 58, 116, 1, (1, 127, 1), {}),
    "pw116g-58-m129": (PW, 116, 58, 1, (1, 3, 43), {"gapped": 1}),
    "pw116-116-m297": (PW, 116, 116, 1, (3, 9, 11), {"acc": (0, 1)}),
    "pw232g-116-m513": (PW, 232, 116, 1, (3, 9, 19), {"gapped": 1}),
    "pw464g-96-m1025": (PW, 464, 96, 1, (1, 25, 41), {"gapped": 1}),
    "pw96-96-m297": (PW, 96, 96, 1, (3, 9, 11), {"acc": (0, 1)}),
    "pw96-255-bias": (PW, 96, 255, 1, (1, 3, 43), {"bias": 1}),
    "pw58-24-m7": (PW, 58, 24, 1, (1, 7, 1), {}),                                       # the one-tile-wide forward GEMM
    "pw116-116-cap2": (PW, 116, 116, 1, (1, 25, 41), {"cap": 2}),                       # 3 slices clipped to 2
    "pw116-116-cap1": (PW, 116, 116, 1, (1, 25, 41), {"cap": 1}),                       # and to 1
    "pw58-58-plane": (PW, 58, 58, 1, (3, 9, 11), {"plane": 1, "acc": (0, 1)}),          # pw1 of a stride-1 unit: reads, and writes dx into, the second half
    # ---- dense 3x3: image borders inside a tile, a tile boundary inside an image, a slice cut inside an image, a one-row strip
    "c3-96-96-b2": (C3, 96, 96, 1, (2, 9, 7), {"acc": (0, 1)}),
    "c3-96-96-b3": (C3, 96, 96, 1, (3, 5, 5), {}),
    "c3-96-96-m1": (C3, 96, 96, 1, (1, 1, 1), {}),
    "c3-96-96-strip": (C3, 96, 96, 1, (2, 1, 7), {}),
    "c3-96-96-m399": (C3, 96, 96, 1, (1, 21, 19), {}),
    "c3-96-96-m297": (C3, 96, 96, 1, (3, 9, 11), {}),
    "c3-96-96-m1353": (C3, 96, 96, 1, (3, 11, 41), {"lim": 2}),                         # three slices of 512 rows, the cuts inside images
    "c3-16-24": (C3, 16, 24, 1, (2, 9, 7), {}),                                         # hwgrad_kernel<9>
    "c3-24-96": (C3, 24, 96, 1, (2, 9, 7), {}),                                         # hwgrad2_kernel<9,2,1>
    "c3-96-24": (C3, 96, 24, 1, (2, 9, 7), {}),                                         # hwgrad2_kernel<9,1,2>
    # ---- depthwise stride 1: W below / at / above the run of 4; H = 1; B = 1 and 3
    "dw24-s1-w3-h1": (DW, 24, 24, 1, (1, 1, 3), {"acc": (0, 1)}),
    "dw58-s1-w4": (DW, 58, 58, 1, (3, 5, 4), {"acc": (0, 1)}),
    "dw116g-s1-w5": (DW, 116, 116, 1, (1, 6, 5), {"gapped": 1, "bias": 1}),
    "dw232g-s1-w8": (DW, 232, 232, 1, (3, 4, 8), {"gapped": 1}),
    "dw96-s1-w13": (DW, 96, 96, 1, (1, 7, 13), {"acc": (0, 1), "bias": 1}),
    "dw352-s1-w5": (DW, 352, 352, 1, (3, 5, 5), {"acc": (0, 1), "want": ("dx",)}),      # hdw_kernel<1>: more than 256 padded channels
    "dw58-s1-plane": (DW, 58, 58, 1, (3, 5, 9), {"plane": 1, "acc": (0, 1)}),           # in_off / out_off / x_off of a unit tensor's second half
    "dw232g-s1-cap": (DW, 232, 232, 1, (3, 9, 11), {"gapped": 1, "cap": 2}),            # G 3 -> 2
    "dw232g-s1-g65": (DW, 232, 232, 1, (3, 172, 13), {"gapped": 1, "want": ("dw",)}),   # 65 weight-gradient workgroups: the 16-row sum grid
    # ---- depthwise stride 2: odd and even extents
    "dw24-s2-5x5": (DW, 24, 24, 2, (1, 5, 5), {"acc": (0, 1)}),
    "dw58-s2-7x9": (DW, 58, 58, 2, (3, 7, 9), {"plane": 1, "acc": (0, 1)}),             # dgrad_s2 into a dx view, wgrad with x_off
    "dw116g-s2-8x6": (DW, 116, 116, 2, (3, 8, 6), {"gapped": 1, "acc": (0, 1)}),
    "dw232g-s2-cap": (DW, 232, 232, 2, (3, 9, 21), {"gapped": 1, "cap": 1}),            # G 2 -> 1
    "dw232g-s2-g66": (DW, 232, 232, 2, (3, 128, 85), {"gapped": 1, "want": ("dw",)}),   # 66 workgroups
}


def conv_geometry(case):
    """what the entry derives from a case: dict Cp, Np, Npad, Npadb, taps, x_ld, x_off, unit (floats of one partial copy), cap"""
    kind, cin, cout, stride, (B, H, W), opt = CONV_CASES[case]
    half, gap, Cp = chan_map(cin, opt.get("gapped", 0))
    Np = Cp if kind == DW else r8(cout)
    taps = 9 if kind == C3 else 1
    unit = 9 * cout if kind == DW else Np * Cp * taps
    plane = opt.get("plane", 0)
    return dict(Cp=Cp, Np=Np, Npad=r32(cout), Npadb=r32(Cp), taps=taps, x_ld=2 * cin if plane else cin, x_off=cin if plane else 0, unit=unit,
                cap=opt["cap"] * unit if "cap" in opt else 0, Mi=B * H * W, Mo=B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1))


def conv_kernels(case, stat=0):
    """the records of one yn_op_h16_conv2 call with dy, in order: forward, dx, dbias, dw, the combine"""
    kind, cin, cout, stride, (B, H, W), opt = CONV_CASES[case]
    g = conv_geometry(case)
    want = opt.get("want", ("dx", "dw", "dbias"))
    cap = g["cap"] or PART_FLOATS
    if kind == DW:
        fwd = hdw_choice(g["Cp"], stride, B, H, W, 1 if stat == 1 else 0)[0]
        dx = "hdw_dgrad_s2_kernel" if stride == 2 else hdw_choice(g["Cp"], 1, B, H, W, 2 if stat == 2 else 0)[0]
        dw = hdw_wgrad_choice(g["Cp"], cout, stride, B, H, W, cap)[0]
    else:
        fwd, dx = hgemm_kernel(g["Npad"], g["taps"], 0), hgemm_kernel(g["Npadb"], g["taps"], 0)
        dw = hwgrad_kernel(g["Np"], g["Cp"], g["taps"])
    names = [fwd]
    if "dx" in want:
        names.append(dx)
    if "dbias" in want:
        names.append("hcol_reduce_kernel<3>")
    if "dw" in want:
        names.append(dw)
    if "dw" in want or "dbias" in want:
        names.append("hgrad_finish_kernel")
    return names


# the depthwise run kernel's statistics epilogues: id -> (conv case shape) C, gapped, (B, H, W), stat, act of the layer below (stat 2)
DW_STAT_CASES = {
    "dws58-fwd": (58, 0, (3, 5, 9), 1, 0),
    "dws24-fwd-h1": (24, 0, (1, 1, 3), 1, 0),
    "dws232g-fwd-nr2": (232, 1, (3, 172, 13), 1, 0),          # 2064 runs in 258 blocks of 8: NR = 2
    "dws116g-bwd-relu": (116, 1, (3, 6, 5), 2, 1),
    "dws24-bwd-leaky": (24, 0, (3, 7, 13), 2, 2),
    "dws96-bwd-none": (96, 0, (1, 7, 4), 2, 0),
    "dws232g-bwd-relu-nr2": (232, 1, (3, 172, 13), 2, 1),
}

# hgemm_kernel's statistics epilogues through yn_op_h16_gemm_stats: id -> kind, Cin, Cout, gapped, (B, H, W), act of the layer below
GEMM_STAT_CASES = {
    "gs58-24": (PW, 58, 24, 0, (3, 11, 9), 1),                # forward NT 1, backward NT 2
    "gs24-58": (PW, 24, 58, 0, (2, 15, 15), 1),               # forward NT 2, backward NT 1
    "gs96-96": (PW, 96, 96, 0, (2, 13, 13), 2),               # NT 3 both ways
    "gs116-116": (PW, 116, 116, 0, (2, 19, 17), 1),           # NT 4 both ways
    "gs116g-58": (PW, 116, 58, 1, (2, 10, 12), 0),            # the layer below has the unit's two-plane map
    "gs-c3-96-96": (C3, 96, 96, 0, (2, 12, 11), 2),           # dense 3x3 at the network's NT 3
}


def gemm_stat_kernels(case):
    kind, cin, cout, gapped, _, _ = GEMM_STAT_CASES[case]
    taps = 9 if kind == C3 else 1
    return [hgemm_kernel(r32(cout), taps, 1), hgemm_kernel(r32(chan_map(cin, gapped)[2]), taps, 2)]


# =====================================================================================================================================
# stem, max pool, the fused stem, BatchNorm, glue
# =====================================================================================================================================
STEM_CASES = {"stem-32x32-b1": (1, 32, 32), "stem-34x30-b3": (3, 34, 30), "stem-33x34-b3": (3, 33, 34), "stem-64x48-b1": (1, 64, 48), "stem-64x48-b3": (3, 64, 48),
              "stem-33x34-b1": (1, 33, 34)}
POOL_CASES = {"pool-16x16-b1": (1, 16, 16), "pool-16x16-b3": (3, 16, 16), "pool-17x15-b3": (3, 17, 15), "pool-9x11-b1": (1, 9, 11), "pool-9x11-b3": (3, 9, 11)}


def stem_wgrad_ranges(B, H, W):
    """hstem_wgrad_kernel: (workgroups, pixels per workgroup, pixels of the last chunk of the last non-empty workgroup)"""
    npix = B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
    G = max(min(-(-npix // 256), 2048), 1)
    per = -(-(-(-npix // G)) // STEM_WGRAD_CHUNK) * STEM_WGRAD_CHUNK
    last = npix - (-(-npix // per) - 1) * per
    return G, per, (last - 1) % STEM_WGRAD_CHUNK + 1


# M, C, act: the shapes of tests/test_gpu_train_h16.py, then the batches of four and their tail, and the channel counts with a ragged last octet
BN_CASES = [(500, 58, 1), (4097, 96, 2), (333, 24, 1), (129, 232, 0), (64, 116, 1), (20000, 58, 1), (9001, 24, 2), (5000, 232, 1), (30011, 96, 0), (300000, 24, 1),
            (1, 58, 1), (3, 116, 2), (4, 24, 1), (5, 232, 1), (4, 12, 2), (5, 14, 1), (3, 12, 0), (1, 14, 2)]
BN_UNIT_CASES = [(6000, 58, 1), (4000, 116, 1), (9000, 24, 1), (3000, 12, 2), (2000, 14, 1), (70000, 58, 1), (1, 58, 1), (5, 116, 2), (3, 12, 1), (4, 14, 2), (4, 24, 0)]

RESAMPLE_SIZES = [(6, 3), (10, 5), (4, 2)]                    # (hi, lo): the maps are hi x (hi + 2) and lo x (lo + 1)
RESAMPLE_MODES = [0, 1, 2, 3]

# hgather_kernel as the step uses it: id -> use, bf, M
GATHER_CASES = {"even-58-m1": ("even", 58, 1), "even-58-m1000": ("even", 58, 1000), "even-116-m1000": ("even", 116, 1000), "even-116-m1": ("even", 116, 1),
                "branch1-58-m1000": ("branch1", 58, 1000), "branch1-116-m1": ("branch1", 116, 1), "copy-58-m1000": ("copy", 58, 1000), "copy-116-m1": ("copy", 116, 1)}


def gather_args(use, bf):
    """the launcher's map arguments for the step's three uses over a unit gradient of 2 bf channels (two planes of roundup8(bf)):
    even    its even logical channels -> the FIRST plane of a two-plane input gradient (pads of that plane zeroed)
    branch1 the same channels -> a dense bf-channel tensor (branch1's output gradient)
    copy    a dense bf-channel tensor -> another, channel for channel"""
    bfp = r8(bf)
    if use == "even":
        return dict(src_ld=2 * bfp, src_off=0, src_cs=2, src_half=bf, src_gap=bfp - bf, dst_ld=2 * bfp, dst_off=0, dst_cs=1, dst_half=bf, dst_gap=bfp - bf, n=bf, npad=bfp)
    if use == "branch1":
        return dict(src_ld=2 * bfp, src_off=0, src_cs=2, src_half=bf, src_gap=bfp - bf, dst_ld=bfp, dst_off=0, dst_cs=1, dst_half=bf, dst_gap=0, n=bf, npad=bfp)
    return dict(src_ld=bfp, src_off=0, src_cs=1, src_half=bf, src_gap=0, dst_ld=bfp, dst_off=0, dst_cs=1, dst_half=bf, dst_gap=0, n=bf, npad=bfp)


FINISH_SIZES = [1, 255, 257, FINISH_MAX_BLOCKS * 256 + 257]   # the last one: the grid-stride loop takes a second pass

# Variants the tables do not reach, and why (tests/test_h16_ops_cases_cpu.py lists them instead of omitting them silently)
UNREACHED = {
    "hdw_run_kernel<0> with NR > 1": "without statistics launch_hdw aims at 4096 workgroups of 8192 output elements each: NR = 2 needs a tensor of 33.6 M elements "
                                     "(a quarter of a gigabyte as float64 on the CPU); the NR loop is the same code in <1> and <2>, which reach NR = 2 at 1.6 M elements",
}
