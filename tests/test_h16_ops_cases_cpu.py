"""The case tables of tests/h16_op_cases.py reach every kernel variant that tests/test_gpu_train_h16_ops.py is there for (by the restated
dispatch rules; the GPU cases then assert that the named kernels are the ones that ran), and the restated constants and rules are the ones
csrc/kernels_h16.hip states."""
import os
import re

import h16_op_cases as hoc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "kernels_h16.hip")).read()
OPS = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "yn_train_h16_ops.inc")).read()


def _conv_records():
    out = {}
    for name in hoc.CONV_CASES:
        out[name] = hoc.conv_kernels(name)
    return out


def test_gemm_cases_reach_every_tile_width_and_statistics_form():
    rec = _conv_records()
    fwd = {r[0] for n, r in rec.items() if hoc.CONV_CASES[n][0] != hoc.DW}
    dx = {r[1] for n, r in rec.items() if hoc.CONV_CASES[n][0] != hoc.DW}
    for nt in (1, 2, 3, 4):                                  # every column-tile count, forward and input gradient, without statistics
        assert "hgemm_kernel<%d,1,0>" % nt in fwd, nt
        assert "hgemm_kernel<%d,1,0>" % nt in dx, nt
    assert "hgemm_kernel<3,9,0>" in fwd and "hgemm_kernel<3,9,0>" in dx            # the network's dense 3x3 (96 -> 96)
    stats = [hoc.gemm_stat_kernels(n) for n in hoc.GEMM_STAT_CASES]
    for nt in (1, 2, 3, 4):
        assert any(s[0] == "hgemm_kernel<%d,1,1>" % nt for s in stats), nt
        assert any(s[1] == "hgemm_kernel<%d,1,2>" % nt for s in stats), nt
    assert ["hgemm_kernel<3,9,1>", "hgemm_kernel<3,9,2>"] in stats
    assert any(hoc.GEMM_STAT_CASES[n][3] for n in hoc.GEMM_STAT_CASES)            # a two-plane layer below
    assert {hoc.GEMM_STAT_CASES[n][5] for n in hoc.GEMM_STAT_CASES} == {0, 1, 2}
    # rows on each side of the 128-row tile; accumulate both ways; a dx view
    pw = {n: c for n, c in hoc.CONV_CASES.items() if c[0] == hoc.PW}
    M = {B * H * W for _, _, _, _, (B, H, W), _ in pw.values()}
    assert {1, 7, 127, 129, 297, 513, 1025} <= M
    assert any(o.get("acc") == (0, 1) for *_, o in pw.values()) and any(o.get("plane") for *_, o in pw.values()) and any(o.get("bias") for *_, o in pw.values())
    assert any(B > 1 and H != W for _, _, _, _, (B, H, W), _ in pw.values())


def test_weight_gradient_cases_reach_every_kernel_and_the_clipped_slice_counts():
    want = {"hwgrad_kernel<%d>" % t for t in (1, 9)} | {"hwgrad2_kernel<%d,%s>" % (t, tk) for t in (1, 9) for tk in ("2,1", "1,2", "2,2")}
    seen, slices = set(), {}
    for name, (kind, cin, cout, stride, (B, H, W), opt) in hoc.CONV_CASES.items():
        if kind == hoc.DW:
            continue
        g = hoc.conv_geometry(name)
        seen.add(hoc.hwgrad_kernel(g["Np"], g["Cp"], g["taps"]).split("+")[0])
        slices[name] = hoc.hwgrad_choice(g["Mo"], g["Np"], g["Cp"], g["taps"], g["cap"] or hoc.PART_FLOATS)[2:]
        assert (g["cap"] or hoc.PART_FLOATS) >= g["unit"], name             # the entry refuses less than one copy
    assert seen == want
    assert slices["pw116-116-cap2"] == (2, 3) and slices["pw116-116-cap1"] == (1, 3)
    assert slices["pw464g-96-m1025"] == (3, 3) and slices["pw232g-116-m513"] == (2, 2) and slices["c3-96-96-m1353"] == (3, 3)
    # ragged last slices, and cuts that fall inside an image
    assert hoc.hwgrad_slice_rows(1025, 3) == 384 and 1025 - 2 * 384 == 257
    assert hoc.hwgrad_slice_rows(513, 2) == 320 and 320 % (9 * 19)
    assert hoc.hwgrad_slice_rows(1353, 3) == 512 and 512 % (11 * 41) and 1024 % (11 * 41)
    assert all(s[0] == 1 for n, s in slices.items() if hoc.conv_geometry(n)["Mo"] <= 512)


def test_depthwise_cases_reach_all_five_kernels_and_both_sum_grids():
    rec = _conv_records()
    dw = {n: c for n, c in hoc.CONV_CASES.items() if c[0] == hoc.DW}
    kernels = set()
    for n in dw:
        kernels.update(k for k in rec[n] if k.startswith("hdw"))
    stat = {}
    for n, (C, gapped, (B, H, W), st, act) in hoc.DW_STAT_CASES.items():
        stat[n] = hoc.hdw_choice(hoc.chan_map(C, gapped)[2], 1, B, H, W, st)
    kernels.update(k for k, _ in stat.values())
    assert {"hdw_run_kernel<0>", "hdw_run_kernel<1>", "hdw_run_kernel<2>", "hdw_kernel<1>", "hdw_kernel<2>", "hdw_dgrad_s2_kernel"} <= kernels
    for k in ("hdw_run_kernel<1>", "hdw_run_kernel<2>"):                    # NR = 1 and NR > 1 under statistics
        assert {nr for kk, nr in stat.values() if kk == k} == {1, 2}, k
    nr0 = {hoc.hdw_choice(hoc.conv_geometry(n)["Cp"], 1, *dw[n][4], 0)[1] for n in dw if dw[n][3] == 1 and hoc.conv_geometry(n)["Cp"] <= 256}
    assert nr0 == {1} and "hdw_run_kernel<0> with NR > 1" in hoc.UNREACHED      # named as unreached, with the reason
    assert {hoc.DW_STAT_CASES[n][4] for n in hoc.DW_STAT_CASES if hoc.DW_STAT_CASES[n][3] == 2} == {0, 1, 2}
    # the weight gradient: both strides, clipped and free G, G on each side of 64
    wg = {}
    for n, (kind, cin, cout, stride, (B, H, W), opt) in dw.items():
        if "dw" in opt.get("want", ("dw",)):
            g = hoc.conv_geometry(n)
            wg[n] = (stride,) + hoc.hdw_wgrad_choice(g["Cp"], cout, stride, B, H, W, g["cap"] or hoc.PART_FLOATS)
    for stride in (1, 2):
        mine = [v for v in wg.values() if v[0] == stride]
        assert any(v[2] < v[3] for v in mine) and any(v[2] == v[3] for v in mine), stride
        assert any(v[2] >= 64 for v in mine) and any(v[2] < 64 for v in mine), stride
    assert wg["dw232g-s1-cap"][2:] == (2, 3) and wg["dw232g-s2-cap"][2:] == (1, 2) and wg["dw232g-s1-g65"][2] == 65 and wg["dw232g-s2-g66"][2] == 66
    # shapes: W below / at / above the run of four, one-row images, one and three images, odd and even extents at stride 2, every channel map
    s1 = [c for c in dw.values() if c[3] == 1]
    assert {3, 4, 5, 8, 13} <= {W for *_, (B, H, W), _ in s1} and any(H == 1 for *_, (B, H, W), _ in s1) and {1, 3} <= {B for *_, (B, H, W), _ in s1}
    assert {24, 58, 116, 232, 96, 352} <= {c[1] for c in s1}
    assert {(5, 5), (7, 9), (8, 6)} <= {(H, W) for *_, s, (B, H, W), _ in dw.values() if s == 2}
    for stride in (1, 2):
        opts = [c[5] for c in dw.values() if c[3] == stride]
        assert any(o.get("plane") and o.get("acc") == (0, 1) for o in opts) and any(o.get("gapped") for o in opts), stride


def test_stem_pool_and_glue_cases_sit_on_both_sides_of_every_edge():
    rng = {n: hoc.stem_wgrad_ranges(*c) for n, c in hoc.STEM_CASES.items()}
    assert {B for B, _, _ in hoc.STEM_CASES.values()} == {1, 3} and {(32, 32), (34, 30), (33, 34), (64, 48)} == {(H, W) for _, H, W in hoc.STEM_CASES.values()}
    assert any(last == hoc.STEM_WGRAD_CHUNK for _, _, last in rng.values()) and any(last < hoc.STEM_WGRAD_CHUNK for _, _, last in rng.values())
    assert any(G > 1 for G, _, _ in rng.values()) and any(G == 1 for G, _, _ in rng.values())
    pooled = {n: B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) for n, (B, H, W) in hoc.POOL_CASES.items()}
    assert {(16, 16), (17, 15), (9, 11)} == {(H, W) for _, H, W in hoc.POOL_CASES.values()} and {1, 3} == {B for B, _, _ in hoc.POOL_CASES.values()}
    B, H, W = hoc.POOL_CASES["pool-16x16-b3"]
    per_image = pooled["pool-16x16-b3"] // B
    assert per_image < hoc.STEM_BLOCK < 2 * per_image and hoc.STEM_BLOCK % per_image      # a workgroup's 85 pixels end inside the second image
    assert any(B * H * W > hoc.STEM_BLOCK for B, H, W in hoc.POOL_CASES.values())           # the backward walks input pixels: several workgroups
    assert {1, 3, 4, 5} <= {M for M, _, _ in hoc.BN_CASES} and {12, 14, 24, 58, 116, 232} <= {C for _, C, _ in hoc.BN_CASES}
    assert {0, 1, 2} == {a for _, _, a in hoc.BN_CASES} and {1, 3, 4, 5} <= {M for M, _, _ in hoc.BN_UNIT_CASES}
    assert hoc.RESAMPLE_MODES == [0, 1, 2, 3] and all(hi == 2 * lo for hi, lo in hoc.RESAMPLE_SIZES)
    assert {(u, bf) for u, bf, _ in hoc.GATHER_CASES.values()} == {(u, bf) for u in ("even", "branch1", "copy") for bf in (58, 116)}
    assert {M for _, _, M in hoc.GATHER_CASES.values()} == {1, 1000}
    for bf in (58, 116):                                                                     # the plane boundary falls inside an octet of the source
        assert bf % 8 and hoc.gather_args("even", bf)["src_gap"] == hoc.r8(bf) - bf
    assert {1, 255, 257} <= set(hoc.FINISH_SIZES) and max(hoc.FINISH_SIZES) > hoc.FINISH_MAX_BLOCKS * 256


def test_restated_rules_are_the_ones_the_source_states():
    """The constants and rules are compared as text (white space aside): an edit of a launcher's rule has to be followed in h16_op_cases.py."""
    flat = re.sub(r"\s+", "", SRC)
    for piece in (
            "constexprintBM=128,BN=32*NT,KC=32,",                                             # hgemm_kernel's 128-row tile
            "if(n32%4==0)launch_hgemm_nt<4>(a,s);elseif(n32%3==0)launch_hgemm_nt<3>(a,s);elseif(n32%2==0)launch_hgemm_nt<2>(a,s);elselaunch_hgemm_nt<1>(a,s);",
            "constintTN=a.Np>64?2:1,TK=a.Kp>64?2:1;", "constintgn=(a.Np+64*TN-1)/(64*TN),gk=(a.Kp+64*TK-1)/(64*TK)*a.taps;",
            "constexprintwg_blocks=2048;", "intslices=wg_blocks/(gn*gk);if(slices>512)slices=512;", "constexprintslice_rows=512;",
            "if((long)slices*nk>(long)a.partial_cap)slices=(int)((long)a.partial_cap/nk);", "constintrows=(((a.M+slices-1)/slices)+MT-1)/MT*MT;",
            "if(a.stride==1&&a.Cp<=256){", "constlongruns=(long)a.B*a.H*((a.W+3)/4);", "constexprlonggtarget=256;", "constlongcap=a.st.acc?gtarget:4096;",
            "constintNR=(int)((nb1+cap-1)/cap);", "constexprintR=4;",
            "staticinthlanes_for(intCp){intl=1;while(l<(Cp>>3)&&l<256)l<<=1;returnl;}",
            "constexprintruns=4;longG=(npix+(256/OL)*runs-1)/((256/OL)*runs);constexprintgmax=2048;if(G>gmax)G=gmax;if((size_t)G*C*9>part_cap)G=(long)(part_cap/((size_t)C*9));",
            "(unsigned)(G>=64?16:1)", "constexprintC=24,PB=85;", "constexprintP=64,NX=7;", "longG=(npix+255)/256;",
            "longblocks=(n+255)/256;if(blocks>2048)blocks=2048;"):
        assert piece in flat, piece
    assert flat.count("constexprintC=24,PB=85;") == 2                                          # the fused forward and its backward
    assert (hoc.GEMM_TILE_ROWS, hoc.WG_BLOCKS, hoc.WG_SLICE_ROWS, hoc.WG_MAX_SLICES, hoc.DW_R, hoc.DW_GTARGET_STAT, hoc.DW_GTARGET, hoc.DW_WGRAD_GMAX,
            hoc.DW_WGRAD_RUNS, hoc.STEM_BLOCK, hoc.STEM_WGRAD_CHUNK, hoc.FINISH_MAX_BLOCKS) == (128, 2048, 512, 512, 4, 256, 4096, 2048, 4, 85, 64, 2048)
    assert "constexprsize_tHOP_PART_FLOATS=(size_t)4<<20;" in re.sub(r"\s+", "", OPS) and hoc.PART_FLOATS == 4 << 20
    assert "constexprintGRAD_SLOTS=8;" in re.sub(r"\s+", "", open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "yn_internal.h")).read()) and hoc.GRAD_SLOTS == 8


def test_every_launcher_names_its_kernel():
    """each launch_* of kernels_h16.hip stores the symbol it launches (profile records carry it)"""
    bodies = re.split(r"\n(?:static )?(?:template <int NT>\nstatic )?void (launch_\w+)\(", SRC)
    launchers = dict(zip(bodies[1::2], bodies[2::2]))
    assert len(launchers) >= 24
    for name, body in launchers.items():
        body = body.split("\n}\n")[0]
        if name == "launch_hgemm":                           # dispatches to launch_hgemm_nt, which names the kernel
            continue
        assert "hipLaunchKernelGGL" in body and "set_last_kernel_name(" in body, name
