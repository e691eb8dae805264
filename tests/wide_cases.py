"""What tests/test_gpu_wide.py and tests/test_wide_cases_cpu.py share: the launch plan of the backbone (run_network / run_unit_chain of csrc/yn_api.hip,
down2_covers / unit_chain_dispatch of csrc/kernels_chain.hip, launch_unit_pipe of csrc/kernels_pipe.hip) restated in Python for the 1.5x and 2.0x
backbones, with 1.0x as the control that goes through the same function.

plan(backbone, H, W, B, ...) returns the profile records a forward must leave for the backbone and the laterals, in launch order: [(layer name, kernel)].
A kernel is the recorded symbol, except for a pointwise GEMM: its tile configuration is the autotuner's (a pure speed matter, pinned bit-identical by
test_op_pointwise_every_tile_configuration_bit_identical), so the plan names the FAMILY (PW) and pw_ok() says which symbols belong to it.

The plan at the wide widths (stage widths 176 / 352 / 704 and 244 / 488 / 976, branch widths bf = half of them), split-f16 family:

  unit                     1.5x                                                        2.0x
  stage 2, stride-2 unit   pw1 + down2_kernel<1,4>, cin 24 != bf 88, Npad 96           bf 122 is no multiple of 4: five launches (fork / join)
  stage 2, stride-1 units  unit_chain2_kernel<4,1,3,4,2>, bf 88 < Npad 96              no chain form without channel quads at Npad 128: three launches per
                                                                                       unit, the 2-channel depthwise variants
  stage 3, stride-2 unit   pw1 + down2_kernel<2,4>, Npad 192                           pw1 + down2_kernel<2,4>, cin = bf = 244, Npad 256; with unit 1's pw1 as
                                                                                       its last phase up to 2048 output pixels
  stage 3, stride-1 units  Npad 192: no chain form, three launches per unit            unit_chain2_kernel<1,4,2,4,3>
  stage 4                  cin 352 > 256: five launches; Npad 352: units unchained     cin 488: five launches; Npad 512: units unchained
  laterals                 K = 176 / 352 / 704 in one grouped launch                   K = 244 / 488 / 976
The exact_f32 family has no stride-2 unit kernel (five launches at every stage) and chains with unit_chain_kernel<4,1,3,4> (bf 88) and <1,4,2,4> or,
from 256 tiles of 64 pixels, <2,2,4,4> (bf 244).  No stage_pipe_kernel / unit_pipe_kernel / pw_pipe_kernel form exists at any wide width.
"""
import infer_op_cases as ioc
from yolo_nano_amd import arch

PW = "pointwise"                                             # a pointwise GEMM of the handle's family, any tile configuration
WIDE = ("1.5x", "2.0x")
CONTROL = "1.0x"
PIPE_PREFIXES = ("stage_pipe_kernel", "unit_pipe_kernel", "pw_pipe_kernel")

NEXT_PAYS_MAX = 32 * 64                                      # run_network: down2_kernel also computes unit 1's pw1 up to this many output pixels
CHAIN_BIG_TILES = 256                                        # unit_chain_dispatch, exact family at Npad 256: <2,2,4,4> from this many 64-pixel tiles
UNIT_PIPE_WIDTHS = (232, 116, 58, 96, 48, 24)               # launch_unit_pipe's instantiated widths
STAGE_PIPE_WIDTHS = (24, 48, 96, 116)                        # stage_pipe_form's
PW_PIPE_FORMS = ((116, 128), (116, 96), (58, 64), (96, 96), (48, 64), (24, 32), (24, 64), (232, 256), (232, 96))      # launch_pw_pipe's (K, Npad)


def npad(n):
    return (n + 31) // 32 * 32


def pw_ok(kernel, exact, backbone):
    """does `kernel` belong to the pointwise family the handle mode runs?  pw_pipe_kernel only where a form of it exists: never on a wide backbone"""
    if exact:
        return kernel.startswith(("gemm_conv_kernel<", "gemm_direct_kernel<"))
    return kernel.startswith("gemm_split_kernel<") or (backbone not in WIDE and kernel.startswith("pw_pipe_kernel<"))


# ---- csrc/kernels_chain.hip ---------------------------------------------------------------------------------------------------------------------
def down_unit_covers(cin, bf):
    """down_unit_pipe_kernel's instantiated widths: stage 2 of 1.0x and 0.5x"""
    return cin == 24 and bf in (58, 24)


def down2_covers(cin, bf, H, W):
    return H > 1 and W > 1 and bf >= 4 and cin >= 4 and bf % 4 == 0 and cin % 4 == 0 and bf <= 256 and cin <= 256 and npad(bf) <= 256


def down2_kernel(bf):
    return "down2_kernel<1,4>" if npad(bf) <= 128 else "down2_kernel<2,4>"


def unit_chain_form(bf, M, exact):
    """unit_chain_dispatch's tile for a stage of dense [M][bf] / [M][2 bf] tensors (all row strides multiples of 4 exactly when bf is), or None"""
    Np, v4 = npad(bf), bf % 4 == 0
    if bf % 2:
        return None
    if not exact:
        forms = {(64, False): "2,2,1,2,4", (64, True): "2,2,1,4,4", (128, True): "1,4,1,4,4" if M <= 4096 else "2,2,2,4,3", (256, True): "1,4,2,4,3",
                 (32, True): "4,1,1,4,4", (96, True): "4,1,3,4,2"}
        f = forms.get((Np, v4))
        return "unit_chain2_kernel<%s>" % f if f else None
    tiles64 = (M + 63) // 64
    forms = {(64, False): "2,2,1,2", (64, True): "2,2,1,4", (128, True): "2,2,2,4", (256, True): "2,2,4,4" if tiles64 >= CHAIN_BIG_TILES else "1,4,2,4",
             (32, True): "4,1,1,4", (96, True): "4,1,3,4"}
    f = forms.get((Np, v4))
    return "unit_chain_kernel<%s>" % f if f else None


# ---- csrc/yn_stage_form.h, csrc/kernels_pipe.hip: what only the control can reach ------------------------------------------------------------------
def plane_stride(C):
    return ((((C + 7) >> 3) + 1) & ~1) * 8 + 8


def unit_pipe_lds(bf, W, bm):
    row = (bf * 4 + 15) // 16 * 16
    window = ((bm + 2 * W + 2) * bf * 4 + 8 + 15) & ~15
    return window + bm * row + 2 * bm * plane_stride(bf) * 2 + bm * 4 + 10 * bf * 4


def unit_pipe_form(bf, M, W, last, mode):
    """launch_unit_pipe's kernel for a split-family unit of the network (ReLU pointwise, linear depthwise convs, dense tensors), or None"""
    if not mode or bf not in UNIT_PIPE_WIDTHS or M % 8 or (bf > 128 and npad(bf) != 256):
        return None
    min_tiles = 1 if bf > 128 else 256
    for nw in ((8,) if bf > 128 else (4, 8)):
        bm = 32 * (nw // (2 if bf <= 64 else (4 if bf <= 128 else 8)))
        if unit_pipe_lds(bf, W, bm) <= (80 if nw == 4 else 160) * 1024:
            if mode < 2 and (M + bm - 1) // bm < min_tiles:
                return None
            return "unit_pipe_kernel<%d,%s,%d>" % (bf, "true" if last else "false", nw)
    return None


# ---- csrc/yn_api.hip: run_network's backbone and laterals -----------------------------------------------------------------------------------------
def maps(H, W):
    """(h, w) of the stage 2 / 3 / 4 output maps"""
    return [(H // s, W // s) for s in arch.STRIDES]


def plan(backbone, H, W, B, exact=False, down_fuse=True, unit_chain=1, group_launch=True, chain_pipe=1):
    """[(layer name, kernel symbol or PW)] of the backbone and lateral records of one forward, in launch order.  stage_fuse is taken at its default (1):
    a stage runs as one launch from 256 tiles only, which the shapes of this suite stay below on the control (asserted) and which no wide width has."""
    out = []
    cin, h, w = 24, H // 4, W // 4
    for si, (R, C) in enumerate(zip(arch.STAGE_REPEATS, arch.STAGE_CH[backbone])):
        st, bf, ho, wo = si + 2, C // 2, h // 2, w // 2
        Mo = B * ho * wo
        P0 = "backbone.stage%d.0" % st
        chain = unit_chain_form(bf, Mo, exact) if unit_chain and R > 1 else None
        use_down = down_fuse and not exact and down_unit_covers(cin, bf)
        use_down2 = not use_down and down_fuse and not exact and down2_covers(cin, bf, h, w)
        down_chained = bool(use_down2 and Mo <= NEXT_PAYS_MAX and chain)
        if use_down:
            out.append((P0 + ".unit", "down_unit_pipe_kernel<%d,%d,true>" % (cin, bf)))
        elif use_down2:
            out += [(P0 + ".b2.pw1", PW), (P0 + (".dw+pw2|b1+pw1n" if down_chained else ".dw+pw2|b1"), down2_kernel(bf))]
        else:                                                # five launches: branch 1 on a side stream, joined in front of pw2's concat + shuffle
            out += [(P0 + ".b1.dw", ioc.dw_kernel(ioc.dw_variant(cin, 2, B, h, w))), (P0 + ".b1.pw", PW), (P0 + ".b2.pw1", PW),
                    (P0 + ".b2.dw", ioc.dw_kernel(ioc.dw_variant(bf, 2, B, h, w))), (P0 + ".b2.pw2", PW)]
        if chain:
            if not exact and bf in STAGE_PIPE_WIDTHS and 2 <= R - 2 <= 7:
                assert (Mo + 31) // 32 < 256, "a shape at which the control's stage may run as one launch: restate launch_stage_pipe first"
            if not down_chained:
                out.append(("backbone.stage%d.1.b2.pw1" % st, PW))
            for bi in range(1, R):
                last = bi == R - 1
                pipe = None if exact else unit_pipe_form(bf, Mo, wo, last, chain_pipe)
                out.append(("backbone.stage%d.%d.dw+pw2%s" % (st, bi, "" if last else "+pw1n"), pipe or chain))
        else:
            for bi in range(1, R):
                P = "backbone.stage%d.%d" % (st, bi)
                out += [(P + ".b2.pw1", PW), (P + ".b2.dw", ioc.dw_kernel(ioc.dw_variant(bf, 1, B, ho, wo))), (P + ".b2.pw2", PW)]
        cin, h, w = C, ho, wo
    if group_launch and not exact:
        out.append(("conv1x1_*", "gemm_split_group_kernel"))
    else:
        out += [("conv1x1_%d" % i, PW) for i in range(3)]
    return out


def backbone_records(records):
    """the (name, kernel) pairs of the profile records plan() speaks about"""
    return [(r[0], r[1]) for r in records if r[0].startswith(("backbone.stage", "conv1x1_"))]


def matches(records, want, exact, backbone):
    """None when the records are the plan, else a message naming the first difference"""
    got = backbone_records(records)
    for i, ((gn, gk), (wn, wk)) in enumerate(zip(got, want)):
        ok = gn == wn and (pw_ok(gk, exact, backbone) if wk == PW else (gk.startswith(wk + "<") if wk == "gemm_split_group_kernel" else gk == wk))
        if not ok:
            return "record %d: %s ran %s, the plan names %s %s" % (i, gn, gk, wn, wk)
    if len(got) != len(want):
        return "%d records against %d planned; first unmatched: %s" % (len(got), len(want), (got + want)[min(len(got), len(want))],)
    return None


def kernels(want):
    return {k for _, k in want}


# ---- the shapes: (H, W, B); H != W runs as a window (yn_set_grid_rect) -----------------------------------------------------------------------------
# S 64 x 2: 8 / 4 / 2 maps, a tile spans both images.  96 x 1: 12 / 6 / 3, an odd stage-4 map, 36 stage-3 pixels = a ragged 32-row tile.  160 x 3:
# 20 / 10 / 5, odd maps at two stages.  96 x 160 x 2: row stride != column count.  192 x 15: 2160 stage-3 pixels > 2048 - down2_kernel<2,4> without unit 1's pw1
# (the smallest such batch at the smallest S whose stage-3 map is not a multiple of the 32-pixel tile: 15 x 144; S = 160 would take B = 21).
SHAPES = ((64, 64, 2), (96, 96, 1), (160, 160, 3), (96, 160, 2), (192, 192, 15))
BIG_EXACT = ("2.0x", 512, 512, 16)                          # 16 384 stage-3 pixels = 256 tiles of 64: unit_chain_kernel<2,2,4,4>, GPU-only (on against off)
CASES = [(bb, H, W, B) for bb in WIDE + (CONTROL,) for H, W, B in SHAPES]
