"""CPU checks of the chip route (yolo_nano_amd.chips): the oracle (tests/chip_oracle.py) against the pieces it must agree
with - Resize.__call__'s letterbox arithmetic, ValTransforms, cv2's resize, the drawing oracle's coordinates -, the case table's reach,
refusal()'s messages, the names in the header / ctypes table / build list, and the kernels' resource usage."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import chip_cases as cc
import chip_oracle as orc
import draw_oracle
from oracle.preprocess import cv2_resize_linear_u8, letterbox_geometry, val_transforms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["yn_chip_batch", "yn_chip_create", "yn_chip_destroy", "yn_chip_status"]


@pytest.mark.parametrize("size", [8, 32, 416])
def test_letterbox_rule_is_resize_call(size):
    for sh in range(1, 65):
        for sw in range(1, 65):
            rw, rh, left, top = letterbox_geometry(sh, sw, size)[:4]
            assert orc.fit(sw, sh, size, size, orc.FIT_LETTERBOX) == (rw, rh, left, top), (sh, sw)


def test_f32_square_letterbox_chip_is_val_transforms():
    frame = cc.frame_pixels(1, 130, 90)
    for side in (32, 24):
        p = cc.params((side, side), orc.FIT_LETTERBOX, orc.F32)
        for x, y, sw, sh in ((5, 7, 40, 23), (60, 2, 17, 80), (3, 3, side, side), (10, 10, 2 * side, 2 * side), (0, 0, 50, 50), (100, 40, 1, 9)):
            why, rect = orc.examine(cc.box(x, y, x + sw - 1, y + sh - 1), (130, 90, 0, 0, 0, 0, 0), orc.PIXELS, p, cc.C, None)
            assert why == orc.CHIP and rect[:4] == (x, y, sw, sh)
            want = val_transforms(np.ascontiguousarray(frame[y:y + sh, x:x + sw]), side, cc.MEAN, cc.STD)[0]
            got = orc.render(frame, rect, p)
            assert got.dtype == np.float32 and got.shape == (3, side, side)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (side, x, y, sw, sh)


def test_u8_stretch_chip_is_cv2_resize():
    frame = cc.frame_pixels(2, 61, 47)
    for cw, ch in ((8, 8), (16, 8), (12, 20), (32, 32)):
        p = cc.params((cw, ch), orc.FIT_STRETCH, orc.U8)
        for x, y, sw, sh in ((0, 0, 61, 47), (7, 9, cw, ch), (7, 9, 2 * cw, 2 * ch), (20, 20, 1, 5), (30, 3, 9, 40)):
            why, rect = orc.examine(cc.box(x, y, x + sw - 1, y + sh - 1), (61, 47, 0, 0, 0, 0, 0), orc.PIXELS, p, cc.C, None)
            assert why == orc.CHIP
            assert np.array_equal(orc.render(frame, rect, p), cv2_resize_linear_u8(np.ascontiguousarray(frame[y:y + sh, x:x + sw]), (cw, ch)))


def test_coordinates_are_the_drawing_oracle_s():
    rng = np.random.RandomState(3)
    p = cc.params((8, 8), orc.FIT_STRETCH, orc.U8, min_score=-1.0)
    for w0, h0, space in ((61, 47, orc.LETTERBOX), (130, 37, orc.LETTERBOX), (64, 64, orc.PIXELS)):
        geom = cc.geometry(w0, h0, 96)
        recs = cc.random_recs(rng, 200, w0, h0)
        if space == orc.LETTERBOX:
            recs[:, :4] = np.sort(rng.uniform(0.0, 1.0, size=(200, 2, 2)), axis=1).reshape(200, 4)
        recs[:, 4] = rng.uniform(0.0, 1.0, size=200)              # the drawing oracle's '%.2f' digits need a score in 0..1
        prims = draw_oracle.select(recs, geom, space, -1.0, cc.C)[0]
        assert len(prims) == 200
        n = 0
        for r, (_, X1, Y1, X2, Y2, _) in zip(recs, prims):
            assert [int(v) for v in orc.map_box(r[:4], geom, space)] == [X1, Y1, X2, Y2]
            why, rect = orc.examine(r, geom, space, p, cc.C, None)
            if why == orc.CHIP:                                # no margin: the rectangle is the outlined box clipped to the frame
                n += 1
                assert rect[:4] == (max(X1, 0), max(Y1, 0), min(X2, w0 - 1) - max(X1, 0) + 1, min(Y2, h0 - 1) - max(Y1, 0) + 1)
        assert n > 50


def test_case_table_reaches_every_path():
    res = {c["name"]: cc.expected(c) for c in cc.CASES}
    reasons = {r[2] for v in res.values() for r in v["reasons"]}
    assert reasons == {orc.CHIP, orc.LOW_SCORE, orc.CLASS_OFF, orc.OVERFLOW, orc.UNREAD} | set(orc.SKIPS)
    assert {r[3] for v in res.values() for r in v["reasons"] if r[2] == orc.CHIP} == set(orc.MODES)
    why = lambda name: [r[2] for r in res[name]["reasons"]]
    m = why("modes_u8_stretch_8x8")
    assert m == [orc.CHIP] * 8 + [orc.SKIP_EMPTY] * 2 + [orc.CHIP]
    assert [r[3] for r in res["modes_u8_stretch_8x8"]["reasons"][:5]] == ["copy", "box", "linear", "linear", "linear"]
    assert res["modes_u8_stretch_8x8"]["rects"][4][2] == 1                                     # the 1-pixel-wide source
    assert res["modes_u8_stretch_8x8"]["rects"][7][:4] == [0, 0, 7, 7]                         # clipped at the corner
    assert res["modes_u8_stretch_8x8"]["rects"][8] == res["modes_u8_stretch_8x8"]["rects"][0]  # int() of fractional coordinates
    s = why("selection_u8_letterbox_16x8")
    assert s == [orc.SKIP_INVERTED] * 2 + [orc.SKIP_COORD] * 5 + [orc.LOW_SCORE, orc.CHIP, orc.LOW_SCORE] + [orc.SKIP_CLASS] * 4 + \
        [orc.CLASS_OFF] * 2 + [orc.CHIP] * 2 + [orc.SKIP_CLASS, orc.LOW_SCORE]
    assert res["selection_u8_letterbox_16x8"]["counters"] == (3, 12, 0, 0)
    # every side of the frame is crossed by a margin, and one margin stays inside
    rects = res["margin_f32_letterbox_16x8"]["rects"]
    assert rects[0][0] == 0 and rects[1][0] + rects[1][2] == 61 and rects[2][1] == 0 and rects[3][1] + rects[3][3] == 47
    assert rects[4][:4] == [20 - 9, 15 - 9, 11 + 18, 11 + 18]                                  # 6 + (11 * 250 + 500) // 1000 = 9
    assert why("min_side_u8_stretch_16x8") == [orc.CHIP, orc.SKIP_MIN_SIDE, orc.SKIP_MIN_SIDE, orc.SKIP_MIN_SIDE, orc.CHIP, orc.CHIP]
    assert why("fit_truncates_to_nothing") == [orc.SKIP_FIT, orc.SKIP_FIT, orc.SKIP_FIT, orc.SKIP_FIT, orc.CHIP, orc.CHIP]
    assert res["fit_truncates_to_nothing"]["rects"][0][4:] == [8, 1, 0, 3]
    fits = {(r[4] < 12, r[5] < 20) for r in res["aspects_u8_letterbox_12x20"]["rects"]}
    assert fits == {(True, False), (False, True), (False, False)}                              # tall, wide, equal
    assert res["empty_frame_between"]["offsets"][1] == res["empty_frame_between"]["offsets"][2] > 0
    assert res["empty_frame_between"]["offsets"][3] > res["empty_frame_between"]["offsets"][2]
    big = res["chunks_257_513"]
    assert [sum(1 for r in big["reasons"] if r[0] == b) for b in (0, 1)] == [257, 513]
    assert any(r[2] == orc.CHIP and r[0] == 0 and r[1] == 256 for r in big["reasons"]) or any(r[2] == orc.CHIP and r[0] == 1 and r[1] >= 257 + 512 for r in big["reasons"])
    assert big["counters"][0] > 300
    many = res["seventy_frames"]
    assert len(many["offsets"]) == 71 and many["offsets"][33] > 0 and many["offsets"][70] > many["offsets"][65] and many["counters"][2] == 0
    assert res["overflow_inside_a_frame"]["offsets"] == [0, 4, 6, 6] and res["overflow_inside_a_frame"]["counters"] == (6, 0, 6, 0)
    assert res["overflow_on_a_frame_boundary"]["offsets"] == [0, 4, 4, 4] and res["overflow_on_a_frame_boundary"]["counters"] == (4, 0, 8, 0)
    assert res["overflow_in_the_first_frame"]["offsets"] == [0, 1, 1, 1]
    assert res["short_record_buffer"]["offsets"] == [0, 4, 6, 6] and res["short_record_buffer"]["counters"] == (6, 0, 0, 0)
    assert res["short_record_buffer_on_a_boundary"]["offsets"] == [0, 4, 4, 4]
    assert res["total_zero"]["offsets"] == [0, 0, 0] and res["no_frames"]["offsets"] == [0]
    assert res["range_mark"]["offsets"] == [0, 0, 0, -1] and res["range_mark"]["counters"] == (0, 0, 0, 1)
    spaces = {c["space"] for c in cc.CASES}
    combos = {(c["params"]["cw"], c["params"]["ch"]) for c in cc.CASES}
    assert spaces == {orc.LETTERBOX, orc.PIXELS} and combos == {(8, 8), (16, 8), (12, 20), (32, 32)}
    assert {(c["params"]["fit"], c["params"]["format"]) for c in cc.CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {s for c in cc.CASES for s in c["shapes"]} >= {(61, 47), (64, 64), (130, 37)}
    assert len(res["letterbox_space_0"]["chips"]) > 5


REFUSALS = cc.REFUSALS


@pytest.mark.parametrize("kw,reason", REFUSALS)
def test_refusals(kw, reason):
    from yolo_nano_amd import capi, chips
    kw = dict(kw)
    kw.setdefault("out", "f32")
    nc, mc = kw.pop("num_classes", 20), kw.pop("max_chips", 1024)
    assert chips.refusal(nc, mc, chips.make_params(**kw)) == reason
    with pytest.raises(capi.YnError) as e:
        chips.ChipExtractor(num_classes=nc, max_chips=mc, **kw)
    assert str(e.value) == reason


def test_accepted_configurations_and_defaults():
    from yolo_nano_amd import chips
    assert chips.refusal(20, 1024, chips.make_params()) is None
    assert chips.refusal(1, 1, chips.make_params(size=(8, 8), margin=4.0, margin_px=4096, min_side=16384, out="u8", fill=(255, 0, 7))) is None
    assert chips.refusal(2000, 65536, chips.make_params(size=(1024, 1024), out="f32", fit="stretch")) is None
    p = chips.make_params(out="f32", margin=0.1249)
    assert p["margin_permille"] == 125 and p["fill"].dtype == np.float32
    assert np.array_equal(p["fill"], np.asarray(chips.DEFAULT_MEAN, np.float32) * np.float32(255))
    assert np.array_equal(chips.make_params(out="u8")["fill"], np.zeros(3, np.float32))


def test_unchip_boxes():
    from yolo_nano_amd import chips
    rect = [40, 10, 30, 60, 16, 32, 8, 0]                        # a 30x60 source in a 32x32 letterbox chip: rw 16, left 8
    got = chips.unchip_boxes([[0.25, 0.0, 0.75, 1.0], [0.5, 0.5, 0.5, 0.5]], rect, 32, 32)
    assert np.allclose(got, [[40, 10, 70, 70], [55, 40, 55, 40]])


def test_symbols_in_header_ctypes_table_and_build_list():
    from yolo_nano_amd import build, capi
    import yolo_nano_amd
    build.build()
    header = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (yn_chip_[a-z_]+)", exported))) == SYMBOLS
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in capi.SIGNATURES, s
    for word in ("yn_chip_params", "YN_CHIP_LETTERBOX", "YN_CHIP_STRETCH", "YN_CHIP_U8", "YN_CHIP_F32"):
        assert word in header, word
    assert ("kernels_chip.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert capi.load_library().yn_abi_version() == 2
    from yolo_nano_amd import chips
    assert yolo_nano_amd.ChipExtractor is chips.ChipExtractor and yolo_nano_amd.unchip_boxes is chips.unchip_boxes
    assert ctypes_size(chips.ChipParams) == 17 * 4


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def test_chip_kernels_use_no_scratch():
    """From the built library's gfx950 code objects (the .note metadata the loader uses, as tests/test_isa_cpu.py reads it)."""
    from yolo_nano_amd import build, capi
    build.build()
    blob = open(capi.LIB_PATH, "rb").read()
    found = {}
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob):
        o = m.start()
        n = struct.unpack_from("<Q", blob, o + 24)[0]
        q = o + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            q += 24
            triple = blob[q:q + tl]
            q += tl
            co = blob[o + off:o + off + size]
            if b"gfx950" not in triple or not size or b"chip_resample_kernel" not in co:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
                f.write(co)
            try:
                txt = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name]).decode()
            finally:
                os.unlink(f.name)
            cur = {}
            for ln in txt.splitlines():
                k = re.match(r"\s+(?:- )?\.(\w+):\s+(.*)", ln)
                if not k:
                    continue
                cur[k.group(1)] = k.group(2).strip().strip("'")
                if k.group(1) == "wavefront_size":              # the last key of a kernel's entry
                    if "name" in cur:
                        found[cur["name"]] = cur
                    cur = {}
    mine = {k: v for k, v in found.items() if re.search(r"chip_(select|scan|resample)_kernel", k) and not k.endswith(".kd")}
    assert len(mine) == 3, sorted(found)
    for k, v in mine.items():
        assert int(v["private_segment_fixed_size"]) == 0, (k, v)
        assert int(v["vgpr_count"]) <= 64, (k, v)              # eight waves per SIMD stay possible
