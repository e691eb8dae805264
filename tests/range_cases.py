"""What tests/test_range_cases_cpu.py and tests/test_gpu_range_guard.py share: the table of every place where the split-f16 kernels split an
activation (x = hi + lo * 2^-11, csrc/yn_split.h), the weight engineering that heats exactly one such place, the inputs, and the grid rules of
the persistent kernels restated in Python.  Pure numpy / Python: nothing here needs a GPU.

THE IDEA.  A site is a PRODUCER layer (some of its output channels) and the CONSUMER layers that read those channels.  make_hot(sd, site, f)
multiplies the producer's BatchNorm weight and bias by f - ReLU, leaky ReLU and the identity are positively homogeneous, so those channels come out f
times larger - and the consumers' weights on exactly those input channels by 1 / f.  f is a power of two: both scalings are exact, and downstream of the
consumers the network computes what it computed before (test_neutralisation).  The batch is one quiet image repeated with one loud image (the same
pattern, LOUD times the amplitude) at a chosen index; f is chosen so that the float64 oracle sees the hot channels in (16 376, 32 752] (up to half the limit
of 65 504) in the quiet image and above 131 008 (twice the limit) in the loud one, and everything else below 32 752 in both (test_margins).  Then the loud
image MUST raise the handle's range flag through the kernel that splits those channels - nothing else can: every other split value is in range, and the
NaN that the overflowing split leaves downstream never raises it (fmaxf drops a NaN) - and the all-quiet batch must not.

WHAT IS SPLIT WHERE (the tracking sites of csrc/, TRACKING below) and the launch switches that move a site from one kernel to another (rows()).
"""
import math

import numpy as np

from yolo_nano_amd import arch

LIMIT = 65504.0                      # range_report's threshold (yn_split.h)
QUIET_MAX = 32752.0                  # half of it: what a quiet peak may reach
LOUD_MIN = 131008.0                  # twice: what a loud peak must reach
LOUD = 64.0                          # amplitude of the loud image over the quiet one (a power of two)

# =====================================================================================================================================
# The source files: how many times range_report( and the tracking calls (range_track( , split_store< , split2( ) occur in each, and in which kernel
# (occurrences, not lines: range_track(range_track(amax, v0), v1) counts twice).  test_table_completeness counts the files: a new splitting kernel cannot arrive without a row here.
# (file -> [(kernel or helper, range_report sites, tracking sites, what is tracked)])
# =====================================================================================================================================
TRACKING = {
    "yn_split.h": [("range_track / range_report: the definitions, twice each (guard on / compiled out)", 2, 2, "-"),
                   ("split_store<N>: the helper's one range_track per element", 0, 1, "N adjacent values")],
    "yn_unit_tile.h": [("split2: the helper of unit_pipe_kernel / stage_pipe_kernel (its definition, and the split_store<2> inside)", 0, 2, "an (x1, y) pair of x2'")],
    "yn_device.h": [("gemm_split_tile", 1, 1, "the A rows of every gemm_split_kernel / gemm_split_group_kernel / head_decode(_group)_kernel")],
    "kernels_conv.hip": [("conv3x3_split_kernel", 1, 1, "the halo pixels, behind the resample-add")],
    "kernels_chain.hip": [("unit_chain2_kernel", 2, 2, "one lambda of two channels, used for the depthwise output and for x2'; reports: last unit / not last"),
                          ("down_unit_pipe_kernel", 1, 5, "the input window = pw1's operand (1); branch 1's and branch 2's depthwise outputs (two channels each)"),
                          ("down2_kernel", 2, 3, "both depthwise outputs (one lambda); x2' of the chained form (two channels); reports: before / behind the next pw1"),
                          ("dwpw_pipe_block", 1, 1, "the depthwise output (heads' layers .0 and .2)")],
    "kernels_pipe.hip": [("unit_pipe_kernel", 1, 2, "the depthwise output; x2' through split2"),
                         ("pw_pipe_kernel", 1, 1, "the input rows")],
    "kernels_stage.hip": [("stage_pipe_kernel", 1, 2, "the depthwise output; x2' through split2")],
    "kernels_post.hip": [("head_tail_block", 1, 2, "layer .2's output (depthwise); layer .3's output")],
}
N_REPORT_SITES = 12                  # range_report( call sites in kernels (the two definitions in yn_split.h apart)


def declared_counts(fname):
    return sum(r[1] for r in TRACKING[fname]), sum(r[2] for r in TRACKING[fname])


# =====================================================================================================================================
# Channel provenance (TorchNet.block: chunk, concat, shuffle in two groups)
# =====================================================================================================================================
def unit_positions(branch, chans):
    """positions in a unit's shuffled output of channels `chans` of branch 0 (the first half of the concat: x1 / b1.pw) or 1 (b2.pw2)"""
    return [2 * j + branch for j in chans]


def carriers(backbone, stage, unit, pos):
    """Which input columns of which later layers carry the channels at positions `pos` of the output of unit `unit` of `stage`:
    -> [(layer name, [columns / channels])].  A stride-1 unit passes its first half through (concat position p -> shuffled position 2 p) and feeds
    the second half to b2.pw1; the stage's output goes to its lateral and to both branches of the next stage's stride-2 unit."""
    out = []
    R, C = arch.STAGE_REPEATS[stage - 2], arch.STAGE_CH[backbone][stage - 2]
    bf = C // 2
    pos = sorted(pos)
    for k in range(unit + 1, R):
        x2 = [p - bf for p in pos if p >= bf]
        if x2:
            out.append(("backbone.stage%d.%d.b2.pw1" % (stage, k), x2))
        pos = [2 * p for p in pos if p < bf]
    if pos:
        out.append(("conv1x1_%d" % (stage - 2), pos))
        if stage < 4:
            out.append(("backbone.stage%d.0.b1.dw" % (stage + 1), pos))
            out.append(("backbone.stage%d.0.b2.pw1" % (stage + 1), pos))
    return out


# =====================================================================================================================================
# Sites
# =====================================================================================================================================
class Site:
    """producers: [(layer, channels or None = all)], consumers: [(layer, input columns or None)], splits: the consumers whose input a kernel splits
    (the GEMM-shaped ones; a depthwise consumer reads fp32), kind / stage / unit: what rows() needs"""

    def __init__(self, name, kind, producers, consumers, stage=0, unit=0):
        self.name, self.kind, self.producers, self.consumers, self.stage, self.unit = name, kind, producers, consumers, stage, unit

    def splits(self, specs):
        return [l for l, _ in self.consumers if specs[l].kind != "dw3"]

    def __repr__(self):
        return "Site(%s)" % self.name


def sites(backbone):
    """every site of one backbone, in network order"""
    out = []
    ch = arch.STAGE_CH[backbone]
    out.append(Site("stem", "stem", [("stem", None)], [("backbone.stage2.0.b1.dw", None), ("backbone.stage2.0.b2.pw1", None)], 2, 0))
    for si, (R, C) in enumerate(zip(arch.STAGE_REPEATS, ch)):
        st, bf = si + 2, C // 2
        P = "backbone.stage%d." % st
        upper = list(range(bf // 2, bf))                     # the channels of a branch that land in the second half of the shuffled output: x2 of the next unit
        out.append(Site("s%d.0.b2.dw" % st, "down.dw2", [(P + "0.b2.dw", None)], [(P + "0.b2.pw2", None)], st, 0))
        out.append(Site("s%d.0.b1.dw" % st, "down.dw1", [(P + "0.b1.dw", None)], [(P + "0.b1.pw", None)], st, 0))
        out.append(Site("s%d.0.out" % st, "down.out", [(P + "0.b2.pw2", upper)], carriers(backbone, st, 0, unit_positions(1, upper)), st, 0))
        for k in sorted({1, R // 2, R - 1}):                 # a first, a middle and the last stride-1 unit
            out.append(Site("s%d.%d.b2.dw" % (st, k), "unit.dw", [(P + "%d.b2.dw" % k, None)], [(P + "%d.b2.pw2" % k, None)], st, k))
            if k < R - 1:
                out.append(Site("s%d.%d.out" % (st, k), "unit.out", [(P + "%d.b2.pw2" % k, upper)], carriers(backbone, st, k, unit_positions(1, upper)), st, k))
        out.append(Site("s%d.%d.out" % (st, R - 1), "stage.out", [(P + "%d.b2.pw2" % (R - 1), None)],
                        carriers(backbone, st, R - 1, unit_positions(1, range(bf))), st, R - 1))
    # The neck: what conv3x3_split_kernel splits is the SUM of a lateral and its resampled neighbour, so every addend of a sum must be hot with the
    # same f, and every other reader of an addend must be cooled.  conv1x1_2 feeds smooth_0 (+ up) and smooth_3 (+ down(smooth_2)): with
    # conv1x1_1, conv1x1_2 and smooth_2 hot, the sums in front of smooth_0 (up) and smooth_3 (down) are hot and head 2's first depthwise conv is the only
    # other reader.  Likewise conv1x1_0, smooth_0, smooth_1: the sums in front of smooth_1 (up) and smooth_2 (down), and head 1's first depthwise conv.
    # A sum cannot be heated alone, so each neck site arms one up-sum and one down-sum together; the operator test (test_split_f16_range_guard) arms
    # each resample mode of conv3x3_split_kernel on its own.
    out.append(Site("neck.p4p5", "neck", [("conv1x1_1", None), ("conv1x1_2", None), ("smooth_2", None)],
                    [("smooth_0", None), ("smooth_3", None), ("head_det_2.0", None)]))
    out.append(Site("neck.p3p4", "neck", [("conv1x1_0", None), ("smooth_0", None), ("smooth_1", None)],
                    [("smooth_1", None), ("smooth_2", None), ("head_det_1.0", None)]))
    for h in (1, 2, 3):
        for j in (0, 2, 3):
            out.append(Site("head%d.%d" % (h, j), "head.%d" % j, [("head_det_%d.%d" % (h, j), None)], [("head_det_%d.%d" % (h, j + 1), None)], h, j))
    return out


def site_by_name(backbone, name):
    return next(s for s in sites(backbone) if s.name == name)


def make_hot(sd, site, f, backbone="1.0x", num_classes=20):
    """A copy of the state dict with the site's producer channels f times larger and its consumers' weights on those channels f times smaller"""
    specs = {s.name: s for s in arch.conv_specs(backbone, num_classes)}
    f = np.float32(f)
    assert f > 0 and math.frexp(float(f))[0] == 0.5, "f must be a power of two: both scalings are exact"
    inv = np.float32(1.0) / f
    out = {k: v.copy() for k, v in sd.items()}
    for layer, chans in site.producers:
        s = specs[layer]
        assert s.bn is not None, layer
        idx = slice(None) if chans is None else np.asarray(list(chans))
        out[s.bn + ".weight"][idx] *= f
        out[s.bn + ".bias"][idx] *= f
    for layer, cols in site.consumers:
        s = specs[layer]
        idx = slice(None) if cols is None else np.asarray(list(cols))
        w = out[s.conv + ".weight"]
        if s.kind == "dw3":
            w[idx] *= inv                                    # [C, 1, 3, 3]: a depthwise conv's input channels are its channels
        else:
            w[:, idx] *= inv                                 # [Cout, Cin, k, k]
    return out


# =====================================================================================================================================
# Inputs and the choice of f
# =====================================================================================================================================
def pattern(S, seed=3):
    rs = np.random.RandomState(40009 * seed + S)
    return rs.standard_normal((1, 3, S, S)).astype(np.float32)


def oracle_pair(S):
    """the two images the oracle ever runs: [quiet, loud]"""
    p = pattern(S)
    return np.concatenate([p, p * np.float32(LOUD)], 0)


def batch(S, B, loud_at=None):
    """B quiet images, the loud one at index loud_at (None: all quiet)"""
    p = pattern(S)
    x = np.repeat(p, B, 0)
    if loud_at is not None:
        x[loud_at] = p[0] * np.float32(LOUD)
    return x


def positions(B):
    return sorted({0, B // 2, B - 1})


def peaks_of(sd, backbone, S, num_classes=20):
    """{name: [quiet peak, loud peak]} of the float64 oracle on oracle_pair(S), and its raw heads"""
    import torch
    from oracle.torch_port import TorchNet
    pk = {}
    heads = TorchNet(sd, backbone, num_classes, dtype=torch.float64, peaks=pk).forward_raw(oracle_pair(S))
    return pk, heads


def hot_peaks(site, pk, specs):
    """(quiet, loud) peak of what the site's kernels split: the inputs of its GEMM-shaped consumers"""
    q = max(float(pk[l + ":in"][0]) for l in site.splits(specs))
    lo = min(float(pk[l + ":in"][1]) for l in site.splits(specs))
    return q, lo


def choose_f(sd, site, backbone, S, num_classes=20):
    """-> (f, the heated state dict, its peaks, its float64 raw heads on oracle_pair(S)).  f is the largest power of two that keeps the QUIET image's
    split values at or below QUIET_MAX, so they sit in (16 376, 32 752] - the upper half of what the guard lets pass; the loud image, LOUD = 64 times
    the amplitude, then lands at 18 to 64 times that (the neck sums, with their input-independent bias share, grow least).  Found on the heated network
    itself: a first run at 2^10, where the hot channels dominate whatever else the consumers read; the scaling is exact, so the second run only
    confirms.  The margins are asserted by the tests, not here."""
    specs = {s.name: s for s in arch.conv_specs(backbone, num_classes)}
    f = 1024.0
    for _ in range(3):
        hot = make_hot(sd, site, f, backbone, num_classes)
        pk, heads = peaks_of(hot, backbone, S, num_classes)
        q = hot_peaks(site, pk, specs)[0]
        step = 2.0 ** math.floor(math.log2(QUIET_MAX / q))
        if step == 1.0:
            break
        f *= step
    return f, hot, pk, heads


def margins(site, pk, specs):
    """None when the heated network's peaks keep the margins, else what is wrong.  Hot layers: the producers (their own output) and the split
    consumers' inputs.  Everything else - every other layer's output and input, in both images - stays at or below QUIET_MAX."""
    hot_names = {l for l, _ in site.producers} | {l + ":in" for l, _ in site.consumers}
    q, lo = hot_peaks(site, pk, specs)
    if q > QUIET_MAX:
        return "quiet peak %.0f of the split values above %.0f" % (q, QUIET_MAX)
    if lo < LOUD_MIN:
        return "loud peak %.0f of the split values below %.0f" % (lo, LOUD_MIN)
    for l, _ in site.producers:
        if float(pk[l][0]) > QUIET_MAX:
            return "quiet peak %.0f at producer %s" % (float(pk[l][0]), l)
    for name, v in pk.items():
        if name not in hot_names and float(v.max()) > QUIET_MAX:
            return "%s peaks at %.0f" % (name, float(v.max()))
    return None


# =====================================================================================================================================
# Launch rules restated (csrc/yn_api.hip run_network / run_unit_chain, the launchers of kernels_chain.hip, kernels_pipe.hip, kernels_stage.hip)
# =====================================================================================================================================
def xcd_grid(blocks):
    return (blocks + 7) & ~7


def npad(n):
    return (n + 31) // 32 * 32


def plane_stride(C):
    return ((((C + 7) >> 3) + 1) & ~1) * 8 + 8


def stage_maps(S):
    return [S // s for s in arch.STRIDES]


def unit_pipe_bm(bf, nw):
    return 32 * (nw // (2 if bf <= 64 else (4 if bf <= 128 else 8)))


def unit_pipe_lds(bf, W, bm):
    row = (bf * 4 + 15) // 16 * 16
    window = ((bm + 2 * W + 2) * bf * 4 + 8 + 15) & ~15
    return window + bm * row + 2 * bm * plane_stride(bf) * 2 + bm * 4 + 10 * bf * 4


def unit_pipe_grid(bf, M, W):
    """launch_unit_pipe: (NW, tiles, workgroups) of the form taken, None without one.  grid = xcd_grid(tiles) capped at 512 (four wavefronts) / 256
    (eight): a workgroup walks two tiles from tiles > cap"""
    if M % 8:
        return None
    for nw in ((8,) if bf > 128 else (4, 8)):
        bm = unit_pipe_bm(bf, nw)
        if unit_pipe_lds(bf, W, bm) <= (80 if nw == 4 else 160) * 1024:
            tiles = (M + bm - 1) // bm
            return nw, tiles, min(xcd_grid(tiles), 512 if nw == 4 else 256)
    return None


def stage_pipe_grid(bf, M, W, nunits):
    """launch_stage_pipe: (NW, tiles, workgroups); items = tiles x units are handed out by ticket, so SOME workgroup takes two from items > workgroups"""
    if bf not in (24, 48, 96, 116) or M % 8 or not 2 <= nunits <= 7:
        return None
    for nw in (4, 8):
        bm = 32 * (nw // (2 if bf <= 64 else 4))
        lds = (((bm + 2 * W + 2) * bf * 4 + 15) & ~15) + bm * bf * 4 + 2 * bm * plane_stride(bf) * 2 + bm * 4 + 14 * bf * 4 + 64 + 192
        if lds <= (80 if nw == 4 else 160) * 1024 and W + 1 <= bm:
            tiles = (M + bm - 1) // bm
            g = (768 if bf <= 48 else 384) if nw == 4 else 256
            return nw, tiles, min(g, tiles * nunits)
    return None


PW_PIPE_FORMS = {(116, 128): (4, 4), (116, 96): (4, 4), (58, 64): (4, 4), (96, 96): (4, 4), (48, 64): (4, 4), (24, 32): (4, 4), (24, 64): (4, 4),
                 (232, 256): (8, 1), (232, 96): (4, 2)}      # launch_pw_pipe: (K, Npad) -> (NW, OCC)


def pw_pipe_grid(K, N, M):
    """launch_pw_pipe: (tiles, workgroups): xcd_grid(tiles) capped at min(1024, 256 x OCC)"""
    form = PW_PIPE_FORMS.get((K, npad(N)))
    if form is None or M < 64:
        return None
    nw, occ = form
    wn = 1 if npad(N) <= 32 else (2 if npad(N) <= 64 else (4 if npad(N) <= 128 else 8))
    bm = 32 * (nw // wn)
    tiles = (M + bm - 1) // bm
    return tiles, min(xcd_grid(tiles), 1024, 256 * occ)


def down_unit_grid(B, H, W):
    """launch_down_unit on an H x W input map: 8 x 4 output tiles, xcd_grid(tiles) capped at 1024 walking workgroups"""
    tiles = B * ((H // 2 + 3) // 4) * ((W // 2 + 7) // 8)
    return tiles, min(xcd_grid(tiles), 1024)


def dwpw_group_grid(B, maps):
    """dwpw_group_grid: per level (tiles, workgroups) - ceil(tiles / 3) rounded up to 8, or, beyond 1024 resident slots, the fewest steps with which
    all levels fit"""
    tiles = [B * ((h + 3) // 4) * ((w + 7) // 8) for h, w in maps]
    TL = [(t + 7) >> 3 for t in tiles]
    wgs = [xcd_grid((t + 2) // 3) for t in tiles]
    if sum(wgs) > 1024:
        S = max((sum(tiles) + 1023) // 1024, 3)
        while sum(8 * ((tl + S - 1) // S) for tl in TL) > 1024:
            S += 1
        wgs = [min(w, 8 * ((tl + S - 1) // S)) for w, tl in zip(wgs, TL)]
    return list(zip(tiles, wgs))


def walk(tiles, grid):
    """the longest walk of a workgroup under the XCD-contiguous round-robin (unit_pipe_kernel, pw_pipe_kernel, down_unit_pipe_kernel,
    dwpw_pipe_block): XCD x owns tiles [x TX, (x + 1) TX), TX = ceil(tiles / 8); workgroup j of its grid / 8 takes tiles j, j + grid / 8, ..."""
    TX, step = (tiles + 7) >> 3, grid >> 3
    best = 0
    for x in range(8):
        n = max(0, min((x + 1) * TX, tiles) - x * TX)
        if n and step:
            best = max(best, (n + step - 1) // step)
    return best


# The persistent cases: kernel -> (backbone, S, B, the sites run there).  B is the smallest batch at S = 224 (the largest size the issue allows the
# small cases; maps 28 / 14 / 7) at which the kernel's launcher gives a workgroup two tiles (test_walk_lengths asserts both that it does and that B - 1,
# or the next smaller legal batch, does not).  unit_pipe_kernel needs M % 8 == 0: 196 B pixels at stage 3 - an even B.
PERSISTENT_S = 224
PERSISTENT = {
    # 1.0x stage 3, bf 116: BM 32, cap 512: 196 B / 32 > 512  <=>  B >= 84
    "unit_pipe_kernel": ("1.0x", 84, ("s3.1.b2.dw", "s3.1.out", "s3.7.b2.dw"), {"chain_pipe": 2, "stage_fuse": (0, False)}),
    # 1.0x stage 3: 6 units x ceil(196 B / 32) tiles > 384 workgroups  <=>  B >= 11 (odd B: M % 8 != 0) -> 12
    "stage_pipe_kernel": ("1.0x", 12, ("s3.1.b2.dw", "s3.4.b2.dw", "s3.4.out"), {"stage_fuse": (2, False)}),
    # stage 3 unit 1's pw1 (K = N = 116, Npad 128) as a launch of its own: BM 32, 1024 workgroups: 196 B / 32 > 1024  <=>  B >= 168
    "pw_pipe_kernel": ("1.0x", 168, ("s3.0.out",), {"down_fuse": False, "pw_config": "pipe"}),
    # stage 2's stride-2 unit: 28 tiles of 8 x 4 per image, 1024 workgroups  <=>  B >= 37
    "down_unit_pipe_kernel": ("1.0x", 37, ("stem", "s2.0.b2.dw", "s2.0.b1.dw"), {}),
    # heads' layers .0+.1 and .2+.3: ceil(tiles / 3) workgroups rounded up to 8, at every size: one image (28 + 8 + 2 tiles) already gives the stride-8
    # level's 16 workgroups two tiles each; B = 3 so that the loud image has three places (84 tiles, 32 workgroups: three tiles each)
    "dwpw_pipe_group_kernel": ("1.0x", 3, ("head1.0", "head1.2"), {}),
}


# ... and one large case that is no walk: from 2048 output pixels down2_kernel leaves unit 1's pw1 to a launch of its own and reports behind its second GEMM (the
# small cases run its chained form).  196 B > 2048  <=>  B >= 11; 12 shares stage_pipe_kernel's handle.
LARGE = {"down2_kernel": ("1.0x", 12, ("s3.0.b2.dw", "s3.0.b1.dw"), {})}


def persistent_walk(kernel, B, S=PERSISTENT_S):
    """the longest walk (tiles or items of one workgroup) the kernel's launcher gives at batch B, 0 where it does not launch"""
    m2, m3, m4 = stage_maps(S)
    if kernel == "unit_pipe_kernel":
        g = unit_pipe_grid(116, B * m3 * m3, m3)
        return walk(g[1], g[2]) if g else 0
    if kernel == "stage_pipe_kernel":
        g = stage_pipe_grid(116, B * m3 * m3, m3, arch.STAGE_REPEATS[1] - 2)
        return -(-g[1] * (arch.STAGE_REPEATS[1] - 2) // g[2]) if g else 0      # pigeonhole: items / workgroups, rounded up
    if kernel == "pw_pipe_kernel":
        g = pw_pipe_grid(116, 116, B * m3 * m3)
        return walk(*g) if g else 0
    if kernel == "down_unit_pipe_kernel":
        return walk(*down_unit_grid(B, S // 4, S // 4))
    if kernel == "dwpw_pipe_group_kernel":
        return max(walk(t, g) for t, g in dwpw_group_grid(B, [(m, m) for m in (m2, m3, m4)]))
    raise KeyError(kernel)


# =====================================================================================================================================
# Switch rows: for a site, every launch-switch combination that moves it into another kernel -> [(switches, route, [(record name, kernel prefix)])]
# route: "raw" = forward_raw, "infer" = yn_infer (the head-tail kernels only run there).  Every (record, kernel) pair must be in the profile records.
# switches: unit_chain, chain_pipe, stage_fuse (mode, publish_early), down_fuse, group_launch, tail_fuse, fuse_decode, pw_config (None = the
# heuristic split tile with the autotuner off, "pipe" = pw_pipe_kernel's index, an int = that index of the split family).
# =====================================================================================================================================
DEFAULTS = {"unit_chain": 1, "chain_pipe": 1, "stage_fuse": (1, False), "down_fuse": True, "group_launch": True, "tail_fuse": True, "fuse_decode": 1,
            "pw_config": None}
SPLIT = "gemm_split_kernel<"
# YN_PWS_CONFIGS (kernels_conv.hip), in index order: (WM, WN, NT, KC) of gemm_split_kernel; pw_pipe_kernel is the index behind them
SPLIT_CONFIGS = ((4, 1, 1, 32), (4, 1, 2, 32), (4, 1, 3, 32), (4, 1, 4, 32), (2, 2, 1, 32), (2, 2, 2, 32), (1, 4, 1, 32), (1, 4, 2, 32), (2, 2, 4, 32),
                 (2, 2, 1, 64), (2, 2, 2, 64), (1, 4, 1, 64), (4, 1, 1, 64), (1, 4, 1, 128))
N_SPLIT_CONFIGS = len(SPLIT_CONFIGS)


def split_kernel(i, K, N):
    """the symbol the profile records for index i of the split family on a K -> N pointwise conv (the last index: pw_pipe_kernel, where it has a form)"""
    if i < N_SPLIT_CONFIGS:
        return "gemm_split_kernel<%d,%d,%d,%d>" % SPLIT_CONFIGS[i]
    assert (K, npad(N)) in PW_PIPE_FORMS, (K, N)
    return "pw_pipe_kernel<%d,%d>" % (K, npad(N))


# ---- the operator-level cases of test_split_f16_range_guard_places (tests/test_gpu_parity.py) -------------------------------------------------------
# pointwise: K = 58 ends inside a 16-deep k-step (10 live columns of the last one), M = 333 ends inside every tile height of the family (32 ... 128 rows).
# pw_pipe_kernel takes a K that is no multiple of 4 only from the network's arena (launch_pw_pipe: in_slack), so it runs K = N = 116 (K % 16 = 4; 32-row
# tiles) - at M = 333 and at PW_WALK_M = 1025 tiles for its 1024 workgroups: the workgroup that takes tile 0 goes on to tile 128, so row 0 lies in a tile that
# is not the last of its walk.
PW_K, PW_N, PW_M, PW_PIPE_K, PW_WALK_M = 58, 58, 333, 116, 32 * 1024 + 13
# dense 3x3: one infer_op_cases.C3_CASES shape per conv3x3_split_kernel variant, and both resample modes for <1,1,9>
C3_PLACES = ("c3s-257tiles", "c3s-86tiles", "c3s-3tiles", "c3s-3tiles-rs", "c3s-w70", "c3s-w112")


def down_unit_covers(cin, bf):
    return cin == 24 and bf in (58, 24)


def unit_kernel(backbone, stage, S, B, last, sw):
    """the kernel a chained stride-1 unit of the small cases runs in (wide_cases.unit_pipe_form / unit_chain_form: the same restatement)"""
    import wide_cases as wc
    bf = arch.STAGE_CH[backbone][stage - 2] // 2
    m = stage_maps(S)[stage - 2]
    pipe = wc.unit_pipe_form(bf, B * m * m, m, last, sw.get("chain_pipe", 1))
    return pipe or wc.unit_chain_form(bf, B * m * m, False)


def rows(site, backbone, S, B, num_classes=20):
    """the switch rows of one site at one shape"""
    ch = arch.STAGE_CH[backbone]
    st, k = site.stage, site.unit
    out = []
    if site.kind == "stem":
        out.append(({}, "raw", [("backbone.stage2.0.unit", "down_unit_pipe_kernel<")]))
        out.append(({"down_fuse": False}, "raw", [("backbone.stage2.0.b2.pw1", SPLIT)]))
        # the whole split family on this GEMM (K = 24: one partial 16-deep k-step), pw_pipe_kernel included
        for c in range(N_SPLIT_CONFIGS):
            out.append(({"down_fuse": False, "pw_config": c}, "raw", [("backbone.stage2.0.b2.pw1", SPLIT)]))
        out.append(({"down_fuse": False, "pw_config": "pipe"}, "raw", [("backbone.stage2.0.b2.pw1", "pw_pipe_kernel<24,")]))
        return out
    if site.kind.startswith("down."):
        bf = ch[st - 2] // 2
        P = "backbone.stage%d.0" % st
        m = stage_maps(S)[st - 2]
        chained = st > 2 and B * m * m <= 2048               # run_network: down2_kernel also computes unit 1's pw1 up to 2048 output pixels
        fused = ("backbone.stage2.0.unit", "down_unit_pipe_kernel<") if st == 2 else (P + (".dw+pw2|b1+pw1n" if chained else ".dw+pw2|b1"), "down2_kernel<")
        if site.kind == "down.dw2":
            return [({}, "raw", [fused]), ({"down_fuse": False}, "raw", [(P + ".b2.pw2", SPLIT)])]
        if site.kind == "down.dw1":
            return [({}, "raw", [fused]), ({"down_fuse": False}, "raw", [(P + ".b1.pw", SPLIT)])]
        nxt = "backbone.stage%d.1.b2.pw1" % st
        out.append(({}, "raw", [(P + ".dw+pw2|b1+pw1n", "down2_kernel<")] if chained else [(nxt, SPLIT)]))
        out.append(({"down_fuse": False}, "raw", [(nxt, SPLIT)]))
        out.append(({"down_fuse": False, "pw_config": "pipe"}, "raw", [(nxt, "pw_pipe_kernel<%d," % bf)]))
        return out
    if site.kind in ("unit.dw", "unit.out"):
        R = arch.STAGE_REPEATS[st - 2]
        bf = ch[st - 2] // 2
        last = k == R - 1
        rec = "backbone.stage%d.%d.dw+pw2%s" % (st, k, "" if last else "+pw1n")
        m = stage_maps(S)[st - 2]
        out.append(({"chain_pipe": 0, "stage_fuse": (0, False)}, "raw", [(rec, "unit_chain2_kernel<")]))
        if unit_pipe_grid(bf, B * m * m, m):
            out.append(({"chain_pipe": 2, "stage_fuse": (0, False)}, "raw", [(rec, "unit_pipe_kernel<%d,%s," % (bf, "true" if last else "false"))]))
        if not last and stage_pipe_grid(bf, B * m * m, m, R - 2):
            for early in (False, True):
                out.append(({"stage_fuse": (2, early)}, "raw",
                            [("backbone.stage%d.1-%d.dw+pw2+pw1n" % (st, R - 2), "stage_pipe_kernel<%d," % bf)]))
        if site.kind == "unit.dw":
            out.append(({"unit_chain": 0}, "raw", [("backbone.stage%d.%d.b2.pw2" % (st, k), SPLIT)]))
        else:
            nxt = "backbone.stage%d.%d.b2.pw1" % (st, k + 1)
            out.append(({"unit_chain": 0}, "raw", [(nxt, SPLIT)]))
            out.append(({"unit_chain": 0, "pw_config": "pipe"}, "raw", [(nxt, "pw_pipe_kernel<%d," % bf)]))
        return out
    if site.kind == "stage.out":
        lat = "conv1x1_%d" % (st - 2)
        nxt = [("backbone.stage%d.0.b2.pw1" % (st + 1), SPLIT)] if st < 4 else []
        out.append(({}, "raw", [("conv1x1_*", "gemm_split_group_kernel<")] + nxt))
        out.append(({"group_launch": False}, "raw", [(lat, SPLIT)] + nxt))
        if (ch[st - 2], 96) in PW_PIPE_FORMS:
            out.append(({"group_launch": False, "pw_config": "pipe"}, "raw", [(lat, "pw_pipe_kernel<%d,96>" % ch[st - 2])]))
        return out
    if site.kind == "neck":
        return [({}, "raw", [(l, "conv3x3_split_kernel<") for l, _ in site.consumers if l.startswith("smooth_")])]
    h, j = site.stage, site.unit
    tail_ok = num_classes > 32                               # head_tail_ok: the grouped tail kernel exists for 32 < C <= 80
    if j == 0:
        out = [({}, "raw", [("head_det_*.0+1", "dwpw_pipe_group_kernel")]),
               ({"group_launch": False}, "raw", [("head_det_%d.1" % h, SPLIT)])]
        if pw_pipe_grid(96, 96, B * stage_maps(S)[h - 1] ** 2):      # (launch_pw_pipe takes 64 rows at the least)
            out.append(({"group_launch": False, "pw_config": "pipe"}, "raw", [("head_det_%d.1" % h, "pw_pipe_kernel<96,96>")]))
        return out
    if j == 2:
        out = [({}, "raw", [("head_det_*.2+3", "dwpw_pipe_group_kernel")]),
               ({"group_launch": False}, "raw", [("head_det_%d.3" % h, SPLIT)])]
        if tail_ok:
            out.append(({"fuse_decode": 2}, "infer", [("head_det_*.2+3+4+decode", "head_tail_group_kernel")]))
        return out
    out = [({}, "raw", [("head_det_*.4", "gemm_split_group_kernel<")]),
           ({"group_launch": False}, "raw", [("head_det_%d.4" % h, SPLIT)]),
           ({"tail_fuse": False, "fuse_decode": 2}, "infer", [("head_det_*.4+decode", "head_decode_group_kernel")]),
           ({"group_launch": False, "fuse_decode": 2}, "infer", [("head_det_%d.4+decode" % h, "head_decode_kernel")])]
    if tail_ok:
        out.append(({"fuse_decode": 2}, "infer", [("head_det_*.2+3+4+decode", "head_tail_group_kernel")]))
    return out


# the kernels the rows must reach between them (test_table_completeness)
KERNELS = ("gemm_split_kernel<", "gemm_split_group_kernel<", "conv3x3_split_kernel<", "down_unit_pipe_kernel<", "down2_kernel<", "unit_chain2_kernel<",
           "unit_pipe_kernel<", "stage_pipe_kernel<", "pw_pipe_kernel<", "dwpw_pipe_group_kernel", "head_tail_group_kernel", "head_decode_group_kernel",
           "head_decode_kernel")

# the small cases: (backbone, classes, S, B).  192 x 4: maps 48 / 24 / 12 / 6, every stage's M a multiple of 8 (unit_pipe_kernel and stage_pipe_kernel take it),
# stage 4's 144 pixels end in a ragged 32-row tile, stage 3's 576 stay below down2_kernel's 2048 (the chained form).  C = 80: the head-tail kernel.
SMALL = (("1.0x", 20, 192, 4), ("0.5x", 20, 192, 4), ("1.0x", 80, 128, 3))
