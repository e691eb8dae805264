"""CPU checks of the JPEG route (yolo_nano_amd.jpeg): the numpy oracle against the stored PIL pixels, the library's host
half (yn_jpeg_info, yn_jpeg_coefficients: no GPU needed) against the oracle, exactly, its refusals, its behaviour on truncated files, and a
stand-alone sanitizer build of csrc/yn_jpeg_host.h fed every prefix and 2000 corruptions of every stored file."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_oracle as orc
from yolo_nano_amd import jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NPZ = os.path.join(HERE, "golden", "jpeg.npz")


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("jpeg.npz")
    meta = json.loads(str(g["meta"]))
    return [dict(m, data=g["file_" + m["name"]].tobytes(), pix=g.get("pix_" + m["name"])) for m in meta]


@pytest.fixture(scope="module")
def lib():
    from yolo_nano_amd import build, capi
    build.build()
    return capi.load_library()


def _bgr(pix):
    return pix if pix.ndim == 3 else np.repeat(pix[..., None], 3, -1)


def test_fixture_holds_every_kind_and_stays_small(cases):
    assert os.path.getsize(NPZ) < 300_000
    ok = [c for c in cases if c["status"] == "ok"]
    names = " ".join(c["name"] for c in cases)
    for size in ("1x1", "8x8", "9x17", "31x33", "17x40", "48x64", "50x35"):
        assert size + "_" in names, size
    for size in ("1x1", "9x17", "31x33", "17x40", "50x35"):
        for sub in ("444", "422", "420"):
            assert "%s_%s_" % (size, sub) in names, (size, sub)
    for word in ("smooth", "noise", "edge", "q5", "q30", "q75", "q95", "q100", "opt", "rst3", "rstrow", "gray", "dqt16"):
        assert any(word in c["name"].split("_") for c in ok), word
    assert sorted(c["tags"][0] for c in cases if c["status"] == "unsupported") == ["cmyk", "progressive"]


def test_oracle_equals_the_stored_pixels(cases):
    for c in cases:
        if c["status"] == "ok":
            assert np.array_equal(orc.decode(c["data"]), _bgr(c["pix"])), c["name"]
        else:
            with pytest.raises(orc.Unsupported):
                orc.decode(c["data"])


def test_info_agrees_with_the_oracle(lib, cases):
    for c in cases:
        m = jpeg.info(c["data"])
        if c["status"] != "ok":
            continue
        o = orc.coefficients(c["data"])
        assert (m["w"], m["h"], m["components"], m["h_samp"], m["v_samp"], m["restart_interval"], m["sof"], m["status"]) == \
               (o["w"], o["h"], o["nc"], o["hs"], o["vs"], o["restart"], o["sof"], jpeg.OK), c["name"]
        assert (m["h"], m["w"]) == c["pix"].shape[:2]
        assert jpeg.coefficient_count(m) == sum(x.size for x in o["coef"])
    assert any(jpeg.info(c["data"])["restart_interval"] for c in cases) and any(jpeg.info(c["data"])["components"] == 1 for c in cases)


def test_coefficients_equal_the_oracle(lib, cases):
    for c in cases:
        if c["status"] != "ok":
            continue
        mine, o = jpeg.coefficients(c["data"]), orc.coefficients(c["data"])
        assert mine["status"] == jpeg.OK and mine["reason"] == "", c["name"]
        assert np.array_equal(mine["qt"], o["qt"]) and mine["qt"].dtype == o["qt"].dtype, c["name"]
        assert np.array_equal(mine["grid"], o["grid"]), c["name"]
        assert len(mine["coef"]) == len(o["coef"])
        for a, b in zip(mine["coef"], o["coef"]):
            assert a.dtype == np.int16 and a.shape == b.shape and np.array_equal(a, b), c["name"]


def test_sixteen_bit_tables_hold_the_same_values(lib, cases):
    c = [c for c in cases if "dqt16" in c["tags"]][0]
    assert b"\xff\xdb" in c["data"] and c["data"][c["data"].index(b"\xff\xdb") + 4] >> 4 == 1
    assert jpeg.coefficients(c["data"])["qt"].max() > 0


def test_refusals_are_unsupported_with_a_reason(lib, cases):
    seen = 0
    for c in cases:
        if c["status"] != "unsupported":
            continue
        m = jpeg.info(c["data"])
        assert m["status"] == jpeg.UNSUPPORTED and m["reason"], c["name"]
        r = jpeg.coefficients(c["data"])
        assert r["status"] == jpeg.UNSUPPORTED and r["reason"], c["name"]
        seen += 1
    assert seen == 2
    assert "progressive" in jpeg.info([c for c in cases if "progressive" in c["tags"]][0]["data"])["reason"]
    assert "4 components" in jpeg.info([c for c in cases if "cmyk" in c["tags"]][0]["data"])["reason"]


def test_a_small_buffer_is_too_large_not_an_overrun(lib, cases):
    import ctypes
    c = [c for c in cases if c["name"].startswith("31x33_420")][0]
    need = jpeg.coefficient_count(jpeg.info(c["data"]))
    buf = np.full(need, 0x5A5A, dtype=np.int16)
    blob = np.frombuffer(c["data"], np.uint8)
    st = ctypes.c_int()
    rc = lib.yn_jpeg_coefficients(blob.ctypes.data, blob.size, buf.ctypes.data, need - 64, None, None, ctypes.byref(st))
    assert rc == st.value == jpeg.TOO_LARGE and str(need) in lib.yn_jpeg_reason(None, 0).decode()
    assert (buf == 0x5A5A).all()


def test_every_prefix_gives_a_status(lib, cases):
    """Every proper prefix of three files (restarts; 4:2:0 with optimised tables; grayscale): a non-OK status with a reason, or a clean OK
    with the full file's coefficients (only the EOI marker may be missing), never a crash."""
    picks = [[c for c in cases if "restart" in c["tags"]][0], [c for c in cases if "optimize" in c["tags"]][0], [c for c in cases if c["gray"]][0]]
    for c in picks:
        full = jpeg.coefficients(c["data"])
        accepted = 0
        for n in range(len(c["data"])):
            r = jpeg.coefficients(c["data"][:n])
            if r["status"] == jpeg.OK:
                accepted += 1
                assert all(np.array_equal(a, b) for a, b in zip(r["coef"], full["coef"])), (c["name"], n)
            else:
                assert r["status"] in (jpeg.CORRUPT, jpeg.UNSUPPORTED) and r["reason"], (c["name"], n)
        assert accepted <= 2, (c["name"], accepted)


def test_broken_syntax_is_corrupt(lib, cases):
    c = [c for c in cases if c["name"].startswith("31x33_420_noise_q30")][0]
    d = bytearray(c["data"])
    sof = d.index(b"\xff\xc0")
    zero_w = bytes(d[:sof + 7]) + b"\x00\x00" + bytes(d[sof + 9:])
    assert jpeg.info(zero_w)["status"] == jpeg.CORRUPT
    no_dht = bytes(d[:d.index(b"\xff\xc4")]) + bytes(d[d.index(b"\xff\xda"):])
    m = jpeg.info(no_dht)
    assert m["status"] == jpeg.CORRUPT and "never defined" in m["reason"]
    twelve = bytes(d[:sof + 4]) + b"\x0c" + bytes(d[sof + 5:])
    assert jpeg.info(twelve)["status"] == jpeg.UNSUPPORTED
    r = [c for c in cases if "restart" in c["tags"]][0]
    e = bytearray(r["data"])
    at = e.index(b"\xff\xd1")
    e[at + 1] = 0xD3
    out = jpeg.coefficients(bytes(e))
    assert out["status"] == jpeg.CORRUPT and "restart" in out["reason"]
    assert jpeg.info(b"")["status"] == jpeg.CORRUPT and jpeg.info(b"\xff\xd8\xff")["status"] == jpeg.CORRUPT


def test_host_half_is_clean_under_sanitizers(cases, tmp_path):
    """csrc/yn_jpeg_host.h on its own (no HIP, no python): every prefix and 2000 seeded single-byte corruptions of every stored file under
    the address and undefined-behaviour sanitizers, in a child process."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I", os.path.join(ROOT, "yolo-nano_amd", "csrc"), os.path.join(HERE, "jpeg_host_check.cpp"), "-o", exe])
    blob = str(tmp_path / "files.bin")
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<I", len(c["data"])))
            f.write(c["data"])
    out = subprocess.run([exe, blob], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ok" in out.stdout and "%d files" % len(cases) in out.stdout


def test_package_exports_the_decoder():
    import yolo_nano_amd
    assert yolo_nano_amd.JPEGDecoder is jpeg.JPEGDecoder and yolo_nano_amd.imread is jpeg.imread and yolo_nano_amd.imread_batch is jpeg.imread_batch
