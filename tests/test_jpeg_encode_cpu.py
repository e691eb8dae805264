"""CPU checks of the JPEG writer (yolo_nano_amd.jpeg): the numpy oracle against the files PIL wrote (stored in
tests/golden/jpeg_encode.npz by tests/golden/gen_jpeg_encode.py; nothing here needs PIL), the library's host half (yn_jpeg_header,
yn_jpeg_quant_tables: no GPU needed) against those files, and the stored files read back through yn_jpeg_coefficients against the
oracle's coefficient stage."""
import hashlib
import json
import os

import numpy as np
import pytest

import jpeg_enc_oracle as enc
import jpeg_oracle as orc
from yolo_nano_amd import jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "jpeg_encode.npz")


@pytest.fixture(scope="module")
def lib():
    from yolo_nano_amd import build, capi
    build.build()
    return capi.load_library()


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("jpeg_encode.npz")
    bench = None
    out = []
    for m in json.loads(str(g["meta"])):
        if m["frame"] == "bench":
            if bench is None:
                bench = orc.decode(open(os.path.join(HERE, "golden", "jpeg_bench.jpg"), "rb").read())
            frame = bench
        else:
            frame = g["frame_" + m["frame"]]
        out.append(dict(m, bgr=frame, data=g["file_" + m["name"]].tobytes() if m["stored"] else None))
    return out


@pytest.fixture(scope="module")
def encoded(cases):
    return {c["name"]: enc.encode(c["bgr"], c["quality"], c["sampling"]) for c in cases}


def test_fixture_holds_every_kind_and_stays_small(cases):
    assert os.path.getsize(NPZ) < 1_000_000
    names = " ".join(c["name"] for c in cases)
    for size in ("1x1", "7x5", "8x8", "16x16", "17x33", "33x17", "40x56", "100x75"):
        for sub in ("444", "422", "420"):
            assert any(c["name"].startswith(size + "_") and "_%s_" % sub in c["name"] for c in cases), (size, sub)
    for word in ("8x2048_", "2048x8_", "bench_", "noise", "ramp", "flat", "blocks", "checker", "q1", "q30", "q75", "q95", "q100"):
        assert word in names, word
    assert all((c["bgr"].shape[1], c["bgr"].shape[0]) == (c["w"], c["h"]) for c in cases)
    assert [c["bgr"].shape for c in cases if c["frame"] == "bench"][0] == (480, 640, 3)
    assert all(c["stored"] == (c["length"] <= 65536) for c in cases)
    st = [c["stats"] for c in cases]                          # the coverage the issue asks of the cases
    assert max(x["stuffed"] for x in st) >= 100 and max(x["zrl"] for x in st) >= 50
    assert max(x["dc_cat"] for x in st) == 11 and max(x["ac_cat"] for x in st) == 10
    assert any(x["dummy_right"] and x["dummy_below"] for x in st)
    assert any(1 <= x["fill_bits"] <= 7 for x in st) and any(x["fill_bits"] == 0 for x in st)


def test_oracle_equals_every_stored_file(cases, encoded):
    for c in cases:
        got, stats = encoded[c["name"]]
        assert len(got) == c["length"] and hashlib.md5(got).hexdigest() == c["md5"], c["name"]
        if c["stored"]:
            assert got == c["data"], c["name"]
        assert stats == c["stats"], c["name"]


def test_header_and_quant_tables_equal_the_stored_files(lib, cases, encoded):
    for c in cases:
        data = c["data"]
        if data is None:                                      # stored as length + MD5: the oracle's bytes, once they have that MD5
            data = encoded[c["name"]][0]
            assert len(data) == c["length"] and hashlib.md5(data).hexdigest() == c["md5"], c["name"]
        assert jpeg.header(c["w"], c["h"], c["quality"], c["sampling"]) == data[:623], c["name"]
        qt = jpeg.quant_tables(c["quality"])
        for t, at in ((0, 25), (1, 94)):                      # the DQT payloads: 64 bytes in zigzag order behind FF DB 00 43 Tq
            assert data[at - 5:at - 1] == b"\xff\xdb\x00\x43" and data[at - 1] == t
            assert bytes(int(qt[t, orc.ZIGZAG[k]]) for k in range(64)) == data[at:at + 64], (c["name"], t)
        assert np.array_equal(qt, enc.quant_tables(c["quality"]))
    for q in range(1, 101):
        assert np.array_equal(jpeg.quant_tables(q), enc.quant_tables(q)), q
    assert jpeg.header(16384, 1, 1, "4:4:4") == enc.header(16384, 1, 1, "4:4:4")


def test_header_and_quant_tables_refuse_bad_arguments(lib):
    for q in (0, 101, -5):
        with pytest.raises(ValueError):
            jpeg.quant_tables(q)
        with pytest.raises(ValueError):
            jpeg.header(8, 8, q)
    for w, h in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        with pytest.raises(ValueError):
            jpeg.header(w, h)
    with pytest.raises(ValueError):
        jpeg.header(8, 8, 95, "4:1:1")
    assert lib.yn_jpeg_header(8, 8, 95, 3, np.zeros(623, np.uint8).ctypes.data) == 1
    assert lib.yn_jpeg_header(8, 8, 95, 2, None) == 1 and lib.yn_jpeg_quant_tables(50, None) == 1


def test_stored_files_parse_to_the_oracles_coefficients(lib, cases):
    for c in cases:
        if not c["stored"]:
            continue
        want = enc.coefficients(c["bgr"], c["quality"], c["sampling"])
        got = jpeg.coefficients(c["data"])
        assert got["status"] == jpeg.OK, (c["name"], got["reason"])
        assert np.array_equal(got["grid"], want["grid"]) and np.array_equal(got["qt"], want["qt"]), c["name"]
        for a, b in zip(got["coef"], want["coef"]):
            assert np.array_equal(a, b), c["name"]
