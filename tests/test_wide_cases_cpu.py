"""tests/wide_cases.py without a GPU: the shapes of tests/test_gpu_wide.py reach every row of the wide backbones' launch plan (by the restated rules; the
GPU cases then assert that the profile records ARE the plan), the restated thresholds are the ones the sources state, no wide width can reach a
persistent (pipe / stage) form, and the float64 TorchNet is the float32 one up to fp32 round-off, on square and on H != W inputs."""
import os
import re

import numpy as np
import torch

import wide_cases as wc
from yolo_nano_amd import arch, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo-nano_amd", "csrc")


def _flat(name):
    return re.sub(r"\s+", "", open(os.path.join(CSRC, name)).read())


def _plans(backbone, **kw):
    return {(H, W, B): wc.plan(backbone, H, W, B, **kw) for bb, H, W, B in wc.CASES if bb == backbone}


def _stage(want, st):
    return [(n, k) for n, k in want if n.startswith("backbone.stage%d." % st)]


def test_cases_hold_both_wide_backbones_and_the_control_at_every_shape():
    assert {bb for bb, _, _, _ in wc.CASES} == {"1.5x", "2.0x", "1.0x"}
    for bb in ("1.5x", "2.0x", "1.0x"):
        assert {c[1:] for c in wc.CASES if c[0] == bb} == set(wc.SHAPES), bb
    assert set(wc.SHAPES) >= {(64, 64, 2), (96, 96, 1), (160, 160, 3), (96, 160, 2)}
    big = [(H, W, B) for H, W, B in wc.SHAPES if B * (H // 16) * (W // 16) > wc.NEXT_PAYS_MAX]
    assert len(big) == 1 and big[0][2] * (big[0][0] // 16) * (big[0][1] // 16) < 1.1 * wc.NEXT_PAYS_MAX        # one shape past next_pays, and barely
    assert any(H != W for H, W, _ in wc.SHAPES)
    assert {3, 5} <= {H // 32 for H, _, _ in wc.SHAPES} and {6, 10} <= {H // 16 for H, _, _ in wc.SHAPES}          # odd stage-4 maps, stage-3 maps off the 4-pixel raster
    assert any(B * (H // 16) * (W // 16) % 32 for H, W, B in wc.SHAPES)                                        # a ragged 32-row tile at stage 3
    assert any(B > 1 and (H // 16) * (W // 16) < 32 for H, W, B in wc.SHAPES)                                  # a tile that spans two images
    bb, H, W, B = wc.BIG_EXACT
    assert bb == "2.0x" and (B * (H // 16) * (W // 16) + 63) // 64 == wc.CHAIN_BIG_TILES                       # the smallest batch of it at that size


def test_split_family_plan_reaches_every_row_of_the_table():
    p15, p20 = _plans("1.5x"), _plans("2.0x")
    for shape, want in p15.items():
        s2, s3, s4 = (_stage(want, st) for st in (2, 3, 4))
        # stage 2: pw1 + down2_kernel<1,4> with unit 1's pw1 chained in (8 x 8 ... 24 x 24 maps: always <= 2048 pixels except the big batch), then the 96-column chain
        H, W, B = shape
        chained2 = B * (H // 8) * (W // 8) <= wc.NEXT_PAYS_MAX
        assert s2[:2] == [("backbone.stage2.0.b2.pw1", wc.PW), ("backbone.stage2.0.dw+pw2|b1" + ("+pw1n" if chained2 else ""), "down2_kernel<1,4>")], shape
        assert [k for _, k in s2[-3:]] == ["unit_chain2_kernel<4,1,3,4,2>"] * 3 and len(s2) == (5 if chained2 else 6), shape
        # stage 3: pw1 + down2_kernel<2,4>, never chained (Npad 192 has no chain form): seven units of three launches
        assert s3[:2] == [("backbone.stage3.0.b2.pw1", wc.PW), ("backbone.stage3.0.dw+pw2|b1", "down2_kernel<2,4>")] and len(s3) == 2 + 7 * 3, shape
        assert {k for _, k in s3[2:]} == {wc.PW, "dwconv3x3_kernel<1,4,2>"}, shape
        # stage 4: cin 352: five launches; units of three launches
        assert [n.rsplit(".", 2)[1] + "." + n.rsplit(".", 1)[1] for n, _ in s4[:5]] == ["b1.dw", "b1.pw", "b2.pw1", "b2.dw", "b2.pw2"] and len(s4) == 5 + 3 * 3, shape
        assert want[-1] == ("conv1x1_*", "gemm_split_group_kernel")
    for shape, want in p20.items():
        H, W, B = shape
        s2, s3, s4 = (_stage(want, st) for st in (2, 3, 4))
        # stage 2: bf 122: five launches, the 2-channel depthwise variants in branch 2 and in the three unchained units
        assert [k for _, k in s2[:5]] == ["dwconv3x3_kernel<2,4,2>", wc.PW, wc.PW, "dwconv3x3_kernel<2,2,2>", wc.PW] and len(s2) == 5 + 3 * 3, shape
        assert [k for _, k in s2[5:]] == [wc.PW, "dwconv3x3_kernel<1,2,4>", wc.PW] * 3, shape
        # stage 3: down2_kernel<2,4> with the next pw1 up to 2048 pixels, without beyond; the 256-column chain either way
        chained = B * (H // 16) * (W // 16) <= wc.NEXT_PAYS_MAX
        assert s3[1] == ("backbone.stage3.0.dw+pw2|b1" + ("+pw1n" if chained else ""), "down2_kernel<2,4>"), shape
        assert [k for _, k in s3[-7:]] == ["unit_chain2_kernel<1,4,2,4,3>"] * 7 and len(s3) == (9 if chained else 10), shape
        assert s4[0][1] == "dwconv3x3_kernel<2,4,2>" and len(s4) == 5 + 3 * 3, shape
    all15 = set().union(*(wc.kernels(w) for w in p15.values()))
    all20 = set().union(*(wc.kernels(w) for w in p20.values()))
    assert all15 == {wc.PW, "down2_kernel<1,4>", "down2_kernel<2,4>", "unit_chain2_kernel<4,1,3,4,2>", "dwconv3x3_kernel<1,4,2>", "dwconv3x3_kernel<2,4,2>",
                     "gemm_split_group_kernel"}
    assert all20 == {wc.PW, "down2_kernel<2,4>", "unit_chain2_kernel<1,4,2,4,3>", "dwconv3x3_kernel<1,4,2>", "dwconv3x3_kernel<2,4,2>",
                     "dwconv3x3_kernel<1,2,4>", "dwconv3x3_kernel<2,2,2>", "gemm_split_group_kernel"}
    names20 = {n for w in p20.values() for n, _ in w}
    assert {"backbone.stage3.0.dw+pw2|b1", "backbone.stage3.0.dw+pw2|b1+pw1n"} <= names20                      # down2_kernel<2,4> with and without the next pw1
    names15 = {n for w in p15.values() for n, _ in w}
    assert {"backbone.stage2.0.dw+pw2|b1", "backbone.stage2.0.dw+pw2|b1+pw1n"} <= names15


def test_exact_family_plan_reaches_the_three_chain_tiles():
    p15, p20 = _plans("1.5x", exact=True), _plans("2.0x", exact=True)
    for want in list(p15.values()) + list(p20.values()):       # no stride-2 unit kernel, no grouped launch: five launches at every stage
        assert not any(k.startswith("down") for _, k in want) and [n for n, _ in want[-3:]] == ["conv1x1_0", "conv1x1_1", "conv1x1_2"]
        assert sum(n.endswith(".0.b1.dw") for n, _ in want) == 3
    assert {k for w in p15.values() for k in wc.kernels(w) if k.startswith("unit_chain")} == {"unit_chain_kernel<4,1,3,4>"}
    assert {k for w in p20.values() for k in wc.kernels(w) if k.startswith("unit_chain")} == {"unit_chain_kernel<1,4,2,4>"}
    bb, H, W, B = wc.BIG_EXACT
    big = wc.plan(bb, H, W, B, exact=True)
    assert {k for k in wc.kernels(big) if k.startswith("unit_chain")} == {"unit_chain_kernel<2,2,4,4>"}
    assert wc.unit_chain_form(244, 64 * 255, True) == "unit_chain_kernel<1,4,2,4>" and wc.unit_chain_form(244, 64 * 255 + 1, True) == "unit_chain_kernel<2,2,4,4>"


def test_switches_name_the_generic_launches_and_never_a_pipe_form():
    for bb in wc.WIDE:
        for exact in (False, True):
            for kw in ({}, {"down_fuse": False}, {"unit_chain": 0}, {"group_launch": False}, {"chain_pipe": 0}, {"chain_pipe": 2}):
                for _, H, W, B in [c for c in wc.CASES if c[0] == bb] + [wc.BIG_EXACT]:
                    want = wc.plan(bb, H, W, B, exact=exact, **kw)
                    assert not any(k.startswith(wc.PIPE_PREFIXES) for _, k in want), (bb, exact, kw)
                    if kw.get("down_fuse") is False:
                        assert not any(k.startswith("down") for _, k in want)
                    if kw.get("unit_chain") == 0:
                        assert not any(k.startswith("unit_chain") or n.endswith("+pw1n") for n, k in want)
                    if kw.get("group_launch") is False:
                        assert want[-1] == ("conv1x1_2", wc.PW)
        # the widths themselves: no persistent form is instantiated for any of them
        cin = 24
        for C in arch.STAGE_CH[bb]:
            bf = C // 2
            assert bf not in wc.UNIT_PIPE_WIDTHS and bf not in wc.STAGE_PIPE_WIDTHS
            for k, n in ((bf, bf), (cin, bf), (C, 96)):
                assert (k, wc.npad(n)) not in wc.PW_PIPE_FORMS, (bb, k, n)
            assert not wc.pw_ok("pw_pipe_kernel<%d,%d>" % (bf, wc.npad(bf)), False, bb)
            cin = C
    # the control does reach them: the same function is not blind to these forms
    ctl = set().union(*(wc.kernels(w) for w in _plans("1.0x").values()))
    assert any(k.startswith("unit_pipe_kernel<232,") for k in ctl) and "down_unit_pipe_kernel<24,58,true>" in ctl and "unit_chain2_kernel<1,4,1,4,4>" in ctl


def test_restated_rules_are_the_ones_the_sources_state():
    chain, api, pipe, form = _flat("kernels_chain.hip"), _flat("yn_api.hip"), _flat("kernels_pipe.hip"), _flat("yn_stage_form.h")
    for piece in ("if(a.Npad==64&&!v4)YN_UC2(2,2,1,2,4)if(a.Npad==64&&v4)YN_UC2(2,2,1,4,4)", "constexprintsmall_m=4096;",
                  "if(a.Npad==128&&v4&&a.M<=small_m)YN_UC2(1,4,1,4,4)if(a.Npad==128&&v4)YN_UC2(2,2,2,4,3)if(a.Npad==256&&v4)YN_UC2(1,4,2,4,3)",
                  "if(a.Npad==32&&v4)YN_UC2(4,1,1,4,4)if(a.Npad==96&&v4)YN_UC2(4,1,3,4,2)returnfalse;",
                  "constinttiles64=(a.M+63)/64;if(a.Npad==64&&!v4)YN_UC(2,2,1,2)if(a.Npad==64&&v4)YN_UC(2,2,1,4)if(a.Npad==128&&v4)YN_UC(2,2,2,4)",
                  "if(a.Npad==256&&v4){if(tiles64>=256)YN_UC(2,2,4,4)elseYN_UC(1,4,2,4)}if(a.Npad==32&&v4)YN_UC(4,1,1,4)if(a.Npad==96&&v4)YN_UC(4,1,3,4)",
                  "a.bf>=4&&a.cin>=4&&!(a.bf&3)&&!(a.cin&3)&&a.bf<=256&&a.cin<=256&&a.Npad>=a.bf&&a.Npad<=256",
                  'if(a.Npad<=128){set_last_kernel_name("down2_kernel<1,4>");', "constboolwidths=a.cin==24&&(a.bf==58||a.bf==24);"):
        assert piece in chain, piece
    for piece in ("constboolnext_pays=Mo<=32*64;", "if(use_down2&&next_pays&&STAGE_REP[si]>1&&run_unit_chain(", "constintmin_tiles=h->stage_fuse==2?1:256;",
                  "if(h->group_launch&&!exact(h)){"):
        assert piece in api, piece
    for piece in ("constintmin_tiles=a.bf>128?1:256;", "YN_UPW(232)", "YN_UPB(116)", "YN_UPB(58)", "YN_UPB(96)", "YN_UPB(48)", "YN_UPB(24)"):
        assert piece in pipe, piece
    assert re.findall(r"YN_UP[WB]\((\d+)\)", pipe) == [str(v) for v in wc.UNIT_PIPE_WIDTHS]
    assert [(int(k), int(n)) for k, n in re.findall(r"YN_PP\((\d+),(\d+),\d+,\d+\)", pipe)] == list(wc.PW_PIPE_FORMS)
    assert "if(bf!=24&&bf!=48&&bf!=96&&bf!=116)return{0,0,0,0};" in form and wc.STAGE_PIPE_WIDTHS == (24, 48, 96, 116)
    assert "constexprintplane_stride(intC){return((((C+7)>>3)+1)&~1)*8+8;}" in form
    assert (wc.NEXT_PAYS_MAX, wc.CHAIN_BIG_TILES) == (32 * 64, 256)


def test_float64_torchnet_is_the_float32_one_up_to_round_off():
    """dtype is the only difference; the default stays float32; forward_raw takes H != W as it stands (taps and heads of the right extents)"""
    from oracle.torch_port import TorchNet
    sd = weights.make_state_dict("1.5x", 20)
    n32, n64 = TorchNet(sd, "1.5x", 20), TorchNet(sd, "1.5x", 20, dtype=torch.float64)
    for H, W in ((64, 64), (64, 96)):
        x = np.random.RandomState(3).standard_normal((2, 3, H, W)).astype(np.float32)
        t32, h32 = n32.forward_taps(x)
        t64, h64 = n64.forward_taps(x)
        assert all(t.dtype == torch.float32 for t in t32 + h32) and all(t.dtype == torch.float64 for t in t64 + h64)
        for t, st, c in zip(t64, arch.STRIDES, arch.STAGE_CH["1.5x"]):
            assert tuple(t.shape) == (2, c, H // st, W // st)
        for a, b, st in zip(h32, h64, arch.STRIDES):
            assert tuple(b.shape) == (2, arch.head_channels(20, 3), H // st, W // st)
        for a, b in zip(t32 + h32, t64 + h64):
            scale = float(b.abs().max())
            err = float((a.double() - b).abs().max())
            assert 0.0 < err <= 2e-5 * scale and scale > 1.0, (err, scale)       # round-off of a few hundred fp32 operations deep, not a different network
        for a, b in zip(n32.forward_raw(x), h32):
            assert torch.equal(a, b)
    # H and W are not mixed up anywhere: the transposed input gives heads of the transposed extents
    xt = np.random.RandomState(4).standard_normal((1, 3, 64, 96)).astype(np.float32)
    a = n64.forward_raw(xt)
    b = n64.forward_raw(np.ascontiguousarray(xt.transpose(0, 1, 3, 2)))
    assert all(u.shape[2:] == v.shape[2:][::-1] for u, v in zip(a, b))


def test_training_tables_carry_the_wide_widths():
    """the case tables of tests/test_gpu_train_ops.py and the parameters of test_train_step_every_gradient_vs_oracle (GPU modules; importing them needs none)"""
    import test_gpu_train as tt
    import test_gpu_train_ops as t
    conv = t.CONV_CASES
    pw = {n: c for n, c in conv.items() if c[0] == t.PW}
    assert {(122, 122), (244, 244), (352, 352), (488, 488), (976, 96), (704, 96)} <= {(c[1], c[2]) for c in pw.values()}
    half = [c for c in pw.values() if c[1:3] == (122, 122)]
    assert any(c[5].get("x_ld") == 244 and c[5].get("x_off") == 122 and c[5].get("acc") == (0, 1) for c in half)
    for k in (244, 352, 488):                                # ragged M, more than one wgrad slice (launch_wgrad: at most ceil(M / 256) slices)
        M = [c[4][0] * c[4][1] * c[4][2] for c in pw.values() if c[1:3] == (k, k)]
        assert any(m > 256 and m % 32 for m in M), k
    dw = [c for c in conv.values() if c[0] == t.DW]
    assert {(c, s) for c in (122, 244, 352, 488) for s in (1, 2)} <= {(c[1], c[3]) for c in dw}
    assert any(c[1] in (122, 244, 352, 488) and c[3] == 2 and c[4][1] % 2 and c[4][2] % 2 for c in dw)
    bn = {(C, unit) for _, C, _, unit, _ in t.BN_CASES.values()}
    assert {(122, True)} | {(C, u) for C in (176, 244, 352, 488) for u in (False, True)} <= bn
    assert all(M <= 512 for M, C, _, _, _ in t.BN_CASES.values() if C in (122, 176, 244, 352, 488))
    assert {(k, t._wgrad_tile(co, ci)) for k, ci, co, *_ in pw.values()} == {(t.PW, tile) for tile in ((2, 2), (2, 4), (3, 3))}
    params = [m for m in tt.test_train_step_every_gradient_vs_oracle.pytestmark if m.name == "parametrize"][0].args[1]
    assert {("1.5x", 96, 20, 2), ("2.0x", 96, 20, 2)} <= set(params)
