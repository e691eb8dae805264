"""tests/range_cases.py checked without a GPU: the site table is complete, the weight engineering heats exactly what it claims and nothing downstream,
the float64 oracle alone puts every site's peaks where the GPU test needs them, and the persistent cases really give a workgroup two tiles."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import infer_op_cases as ioc
import range_cases as rc
from yolo_nano_amd import arch, weights

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yolo-nano_amd", "csrc")
CASES = rc.SMALL + tuple((bb, 20, rc.PERSISTENT_S, B) for bb, B in sorted({(v[0], v[1]) for v in list(rc.PERSISTENT.values()) + list(rc.LARGE.values())}))


def _site_ids():
    seen, out = set(), []
    for bb, C, S, B in CASES:
        if (bb, C, S) in seen:
            continue
        seen.add((bb, C, S))
        out += [(bb, C, S, s.name) for s in rc.sites(bb)]
    return out


@functools.lru_cache(maxsize=None)
def _state(bb, C):
    return weights.make_state_dict(bb, C)


@functools.lru_cache(maxsize=None)
def _base(bb, C, S):
    return rc.peaks_of(_state(bb, C), bb, S, C)


def test_table_completeness():
    """Every occurrence of range_report( and of a tracking call in csrc/ is declared in rc.TRACKING for its file, and every splitting kernel is reached by a row."""
    reports = 0
    for fname in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, fname), errors="replace").read()
        n_rep = len(re.findall(r"range_report\(", src))
        n_trk = len(re.findall(r"range_track\(|split_store<|split2\(", src))
        if n_rep or n_trk or fname in rc.TRACKING:
            assert fname in rc.TRACKING, "%s splits activations (%d reports, %d tracking calls) and has no row in range_cases.TRACKING" % (fname, n_rep, n_trk)
            assert (n_rep, n_trk) == rc.declared_counts(fname), "%s: %d range_report( and %d tracking calls against %s declared" % (fname, n_rep, n_trk, rc.declared_counts(fname))
            if fname != "yn_split.h":
                reports += n_rep
    assert reports == rc.N_REPORT_SITES
    prefixes = set()
    for bb, C, S, B in CASES:
        for site in rc.sites(bb):
            for _, _, expect in rc.rows(site, bb, S, B, C):
                prefixes |= {k for _, k in expect}
    for v in list(rc.PERSISTENT.values()) + list(rc.LARGE.values()):
        assert all(any(s.name == n for s in rc.sites(v[0])) for n in v[2]), v
    for k in [k for k in ioc.C3_KERNELS if "split" in k] + [ioc.PW_FIRST_KERNEL[1]]:
        assert any(k.startswith(p) for p in prefixes), "no row reaches %s" % k
    for k in rc.KERNELS:
        assert any(p.startswith(k) for p in prefixes), "no row reaches %s" % k
    # the kernels of TRACKING are the kernels of KERNELS (a block function runs inside the kernel named behind the arrow)
    inside = {"gemm_split_tile": "gemm_split_kernel<", "dwpw_pipe_block": "dwpw_pipe_group_kernel", "head_tail_block": "head_tail_group_kernel"}
    for fname, table in rc.TRACKING.items():
        for kern, n_rep, _, _ in table:
            if n_rep and fname != "yn_split.h":
                assert any(p.startswith(inside.get(kern, kern)) for p in prefixes), kern


def test_provenance_follows_the_shuffle():
    """carriers() against TorchNet.block itself: mark channels of a unit's output with a one-hot activation, run the rest of the stage's wiring with
    identity convs, and see where the marks arrive."""
    from oracle.torch_port import TorchNet
    bb, st, unit = "1.0x", 3, 2
    C = arch.STAGE_CH[bb][st - 2]
    bf, R = C // 2, arch.STAGE_REPEATS[st - 2]
    net = TorchNet.__new__(TorchNet)
    seen = {}

    def conv(name, x):                                       # records which input channels are marked; returns zeros (an unmarked branch)
        seen[name] = sorted(int(c) for c in torch.nonzero(x[0, :, 0, 0]).flatten())
        return torch.zeros(x.shape[0], bf, 1, 1, dtype=x.dtype) if not name.endswith(".dw") else x

    net.conv = conv
    pos = rc.unit_positions(1, range(bf // 2))               # the lower half of b2.pw2's channels: they pass through the next unit
    x = torch.zeros(1, C, 1, 1, dtype=torch.float64)
    x[0, pos] = 1.0
    for k in range(unit + 1, R):
        x = net.block("backbone.stage%d.%d" % (st, k), x, 1)
    want = dict(rc.carriers(bb, st, unit, pos))
    for k in range(unit + 1, R):
        name = "backbone.stage%d.%d.b2.pw1" % (st, k)
        assert seen[name] == sorted(want.get(name, [])), name
    assert sorted(int(c) for c in torch.nonzero(x[0, :, 0, 0]).flatten()) == sorted(want["conv1x1_%d" % (st - 2)])
    assert want["backbone.stage%d.0.b2.pw1" % (st + 1)] == want["conv1x1_%d" % (st - 2)] == want["backbone.stage%d.0.b1.dw" % (st + 1)]
    # the upper half goes straight into the next unit's pw1 and no further: what the unit.out sites heat
    up = rc.carriers(bb, st, unit, rc.unit_positions(1, range(bf // 2, bf)))
    assert up == [("backbone.stage%d.%d.b2.pw1" % (st, unit + 1), [2 * j + 1 - bf for j in range(bf // 2, bf)])]


@pytest.mark.parametrize("bb,C,S,name", _site_ids())
def test_neutralisation_and_margins(bb, C, S, name):
    """Neutralisation: the float64 heads of the heated network equal those of the original to float64 round-off (relative 1e-9 of the head's largest
    value; worst ratio seen: 0.0 - both scalings are powers of two and every product is exact in float64, so the heated network computes the same
    bits).  Margins, by the float64 oracle on the state dict the GPU test loads: the quiet image's peak of what is split at most 32 752, the loud
    image's at least 131 008, every other layer's output and input at most 32 752 in both images.  f is a power of two, and the quiet peak
    sits in the upper half of what the guard lets pass, (16 376, 32 752]."""
    sd = _state(bb, C)
    site = rc.site_by_name(bb, name)
    specs = {s.name: s for s in arch.conv_specs(bb, C)}
    f, hot, pk, heads = rc.choose_f(sd, site, bb, S, C)
    assert 2.0 <= f <= 2.0 ** 14 and np.log2(f) == int(np.log2(f)), f
    for a, b in zip(heads, _base(bb, C, S)[1]):
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max()), "%s: the heated network is not the original downstream" % name
    bad = rc.margins(site, pk, specs)
    assert bad is None, "%s f %g: %s" % (name, f, bad)
    q, lo = rc.hot_peaks(site, pk, specs)
    assert q > rc.QUIET_MAX / 2, "%s: the quiet peak %.0f is not in the upper half of what the guard lets pass" % (name, q)
    # make_hot touched the producers' BatchNorm and the consumers' weights and nothing else
    changed = {k for k in sd if not np.array_equal(sd[k], hot[k])}
    allowed = {specs[l].bn + leaf for l, _ in site.producers for leaf in (".weight", ".bias")} | {specs[l].conv + ".weight" for l, _ in site.consumers}
    assert changed and changed <= allowed, changed - allowed


def test_operator_cases_name_the_kernels_they_mean():
    """range_cases.SPLIT_CONFIGS is YN_PWS_CONFIGS of kernels_conv.hip, C3_PLACES reaches every conv3x3_split_kernel variant, the pointwise shapes have the ragged
    edges their comment claims"""
    src = open(os.path.join(CSRC, "kernels_conv.hip")).read()
    macro = src[src.index("#define YN_PWS_CONFIGS(X)"):]
    macro = macro[:macro.index("struct SplitCfg")]
    assert tuple(tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", macro)) == rc.SPLIT_CONFIGS
    assert rc.split_kernel(0, rc.PW_K, rc.PW_N) == ioc.PW_FIRST_KERNEL[1] and rc.split_kernel(rc.N_SPLIT_CONFIGS, rc.PW_PIPE_K, rc.PW_PIPE_K) == "pw_pipe_kernel<116,128>"
    got = set()
    for case in rc.C3_PLACES:
        cin, cout, (B, H, W), exact, modes = ioc.C3_CASES[case]
        assert not exact
        got.add(ioc.c3_kernel(cin, cout, B, H, W, False))
        assert (B * H * W) % 128 != 0, case                  # a ragged last tile
    assert got == {k for k in ioc.C3_KERNELS if "split" in k}
    assert set(ioc.C3_CASES["c3s-3tiles-rs"][4]) == {1, 2}
    assert rc.PW_K % 16 and rc.PW_PIPE_K % 16 and rc.PW_PIPE_K % 4 == 0 and all(rc.PW_M % (32 * wm) for wm, _, _, _ in rc.SPLIT_CONFIGS)
    tiles, grid = rc.pw_pipe_grid(rc.PW_PIPE_K, rc.PW_PIPE_K, rc.PW_WALK_M)
    assert (tiles, grid) == (1025, 1024) and rc.walk(tiles, grid) == 2 and rc.walk(*rc.pw_pipe_grid(rc.PW_PIPE_K, rc.PW_PIPE_K, rc.PW_M)) == 1 and rc.PW_M % 32


def test_positions_and_batches():
    x = rc.batch(64, 5, loud_at=2)
    assert rc.positions(5) == [0, 2, 4] and rc.positions(4) == [0, 2, 3] and rc.positions(1) == [0]
    assert np.array_equal(x[0], x[1]) and np.array_equal(x[2], x[0] * np.float32(rc.LOUD)) and np.array_equal(x[3], x[4])
    pair = rc.oracle_pair(64)
    assert np.array_equal(pair[0], x[0]) and np.array_equal(pair[1], x[2])


def test_walk_lengths():
    """The persistent cases give a workgroup a walk of at least two tiles (items), and the next smaller batch the launcher takes does not - B is the smallest."""
    smaller = {"unit_pipe_kernel": 2, "stage_pipe_kernel": 2, "pw_pipe_kernel": 1, "down_unit_pipe_kernel": 1}      # M % 8 == 0 needs an even batch at 14 x 14
    for kern, (bb, B, names, sw) in rc.PERSISTENT.items():
        assert rc.persistent_walk(kern, B) >= 2, (kern, B, rc.persistent_walk(kern, B))
        if kern in smaller:
            w = rc.persistent_walk(kern, B - smaller[kern])
            assert w == 1, "%s: B = %d already walks %d tiles" % (kern, B - smaller[kern], w)
    # the walking rule itself: XCD-contiguous ranges, round-robin inside
    assert rc.walk(1036, 1024) == 2 and rc.walk(1024, 1024) == 1 and rc.walk(1183, 1024) == 2 and rc.walk(28, 16) == 2 and rc.walk(3, 8) == 1
    assert rc.down_unit_grid(13, 104, 104) == (1183, 1024)  # test_down_unit_is_bit_identical's 416 x 416 x 13
    # the tile that holds the loud image is not always the last of its workgroup's walk: with the loud image first, its tiles are each walk's first
    tiles, grid = rc.down_unit_grid(rc.PERSISTENT["down_unit_pipe_kernel"][1], 56, 56)
    assert tiles // 8 > grid // 8                            # XCD 0's range is longer than one round: tile 0's workgroup goes on to another tile
