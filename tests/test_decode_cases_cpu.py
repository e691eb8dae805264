"""tests/decode_cases.py checked without a GPU: its tables reach every decode_kernel<*, KMAX> and every head_decode*<NT, KMAX> instantiation and all
three front ends; its steered data reaches every regime (membership computed from the float64 reference, per wavefront grouping where the regime is
a property of a wavefront); its float64 reference agrees with the pinned oracle (oracle.score_decode, itself pinned to the reference project by
tests/test_oracle_golden.py); its steered head tail is exact; and few random candidates are near-ties that the class check has to excuse."""
import numpy as np
import pytest
import torch

import decode_cases as dc
from f64_bar import bar
from oracle import oracle as orc
from yolo_nano_amd import arch


def test_tables_reach_every_instantiation():
    assert {dc.kmax(C) for C, _ in dc.DECODE_CASES.values()} == set(dc.KMAX_ALL)
    for lo, hi in ((16, 17), (32, 33), (80, 81), (256, 257)):                # both sides of every boundary of launch_decode
        assert lo in dc.DECODE_C and hi in dc.DECODE_C and dc.kmax(lo) != dc.kmax(hi)
    assert dc.num_pred(96) == 567 and 567 % 16 != 0 and all(w % 8 and w % 4 for w in dc.maps(96)[1:])     # a partial last block; maps that fill no tile
    ran = set()
    for C, S in dc.HEAD_TAIL_CASES.values():
        for sw in dc.SWITCHES:
            ran.update(dc.front_end(C, S, *sw))
    want = {"head_tail_group_kernel<5>"} | {"%s<%d,%d>" % ((k,) + v) for k in ("head_decode_kernel", "head_decode_group_kernel") for v in dc.HEAD_DECODE_VARIANTS}
    want |= {dc.decode_kernel(C, False) for C in dc.HEAD_TAIL_C}
    assert ran == want, ran ^ want
    assert dc.head_decode_variant(37) == (1, 5) and dc.npad(37) == 128 and not dc.head_tail_ok(37) and dc.head_tail_ok(80)
    assert not dc.head_decode_supported(81) and dc.front_end(81, 96, 1, 2, 1) == ["decode_kernel<false,16>"]


def test_bn_identity_and_selection_tail_is_exact():
    """fl32(var + eps) == 1: gamma / sqrtf(var + eps) is exactly 1; and the float64 and float32 evaluations of the steered tail agree bit for bit,
    on values that are what the selection promises: raw[n] = activation[n mod 96] + bias[n]"""
    assert np.float32(dc.BN_ONE_VAR) + np.float32(arch.BN_EPS) == np.float32(1.0)
    for C, S in dc.HEAD_TAIL_CASES.values():
        lay = dc.selection_layers(C)
        for x in dc.steered_acts(C, S):
            assert x.min() >= 0 and x.max() <= 120 and np.array_equal(x * 8, np.round(x * 8))
            r64, r32 = dc.tail_ref(x, *lay, dtype=np.float64), dc.tail_ref(x, *lay, dtype=np.float32)
            assert r32.dtype == np.float32 and np.array_equal(r32.astype(np.float64), r64)
            n = np.arange(dc.A * (5 + C))
            assert np.array_equal(r64, x.astype(np.float64)[..., n % dc.NECK] + lay[5].astype(np.float64))


@pytest.mark.parametrize("case", list(dc.DECODE_CASES))
def test_steered_decode_data_reaches_every_regime(case):
    C, S = dc.DECODE_CASES[case]
    heads = dc.steered_heads(C, S)
    r64 = dc.decode_ref(heads, S, C)
    m = dc.regimes(r64, S, C, dc.CONF_STEERED, dc.wave_groups("decode", S))
    for name in dc.REGIMES:
        if name in m:
            assert m[name].any(), (case, name)
        else:
            assert C < 2 or (name == "tie_same_lane" and C <= 16), (case, name)
    assert dc.box_coverage(r64, S) == []
    # the engineered ties pass the threshold somewhere (the class check needs a class there)
    score = r64["score"].reshape(-1)
    for name in ("tie_same_lane", "tie_diff_lane", "tie_first_last", "all_equal", "near_inside", "near_outside", "near_at", "one_finite", "far"):
        if name in m:
            assert (m[name] & (score >= 2 * dc.CONF_STEERED)).any(), (case, name)


@pytest.mark.parametrize("case", list(dc.HEAD_TAIL_CASES))
def test_steered_tail_data_reaches_every_regime(case):
    C, S = dc.HEAD_TAIL_CASES[case]
    lay = dc.selection_layers(C)
    heads = [dc.tail_ref(x, *lay, dtype=np.float32) for x in dc.steered_acts(C, S)]
    r64 = dc.decode_ref(heads, S, C)
    for front in ("decode", "head_decode", "head_tail"):
        m = dc.regimes(r64, S, C, dc.CONF_STEERED, dc.wave_groups(front, S))
        for name in dc.HEAD_TAIL_REGIMES:
            if name == "tie_same_lane" and C <= 16:
                continue
            assert m[name].any(), (case, front, name)
    if dc.head_tail_ok(C):                                  # the three-candidates-per-round form of pass A: rounds that skip in part
        assert dc.tail_round_mixes(r64, S, dc.CONF_STEERED) > 0, case


@pytest.mark.parametrize("case", [k for k, v in dc.DECODE_CASES.items() if v[0] in (20, 80)])
def test_reference_equals_the_pinned_oracle(case):
    C, S = dc.DECODE_CASES[case]
    heads = dc.random_heads(C, S)
    r64, r32 = dc.decode_ref(heads, S, C), dc.decode_ref(heads, S, C, np.float32)
    assert r32["all_class"].dtype == np.float32 and r32["all_bbox"].dtype == np.float32
    for b in range(dc.B):
        bbox, cls = orc.score_decode([h[b].transpose(2, 0, 1) for h in heads], S, C, arch.MULTI_ANCHOR_SIZE, dc.A)
        for name, got in (("all_bbox", bbox), ("all_class", cls)):
            bar(name, "%s b%d" % (case, b), torch.from_numpy(got), torch.from_numpy(r64[name][b]), torch.from_numpy(r32[name][b]))
        sure = ~dc.near_tie_mask(r64, r32)[b]
        assert np.array_equal(cls.argmax(-1)[sure], r64["best"][b][sure])


@pytest.mark.parametrize("case", list(dc.DECODE_CASES) + list(dc.HEAD_TAIL_CASES))
def test_few_random_candidates_are_near_ties(case):
    """the candidates the class check excuses: float64 top-two class scores closer than twice the bar (each may move by one bar)"""
    if case in dc.DECODE_CASES:
        C, S = dc.DECODE_CASES[case]
        heads = dc.random_heads(C, S)
    else:
        C, S = dc.HEAD_TAIL_CASES[case]
        heads = dc.random_tail_heads(C, S)
    r64, r32 = dc.decode_ref(heads, S, C), dc.decode_ref(heads, S, C, np.float32)
    share = dc.near_tie_mask(r64, r32).mean()
    print("near ties %s: %.4f" % (case, share))
    assert share <= 0.01, (case, share)
