"""CPU checks of the device entropy mode of the JPEG decoder (yn_jpeg_entropy): the Python restatement of the subsequence
fixed point against the serial decoder, the library's copy pass (yn_jpeg_scan_prepare: no GPU needed) against a numpy unstuffing, and a
stand-alone sanitizer build of the decode core the kernels compile (csrc/yn_jpeg_huff.h) fed every prefix and 2000 corruptions of every
stored file.  Every comparison is equality: the host stage is exact."""
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_entropy_oracle as ent
import jpeg_oracle as orc
from yolo_nano_amd import jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BITS = (32, 64, 1024)


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("jpeg.npz")
    meta = json.loads(str(g["meta"]))
    return [dict(m, data=g["file_" + m["name"]].tobytes()) for m in meta]


@pytest.fixture(scope="module")
def good(cases):
    return [c for c in cases if c["status"] == "ok"]


@pytest.fixture(scope="module")
def bench():
    with open(os.path.join(HERE, "golden", "jpeg_bench.jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    from yolo_nano_amd import build, capi
    build.build()
    return capi.load_library()


def _check_fixed_point(name, data, want):
    for sb in BITS:
        fp = ent.fixed_point(data, sb)
        assert fp["converged"] and fp["rounds"] <= fp["subseqs"], (name, sb, fp["rounds"], fp["subseqs"])
        assert all(e is not None for e in fp["ends"]), (name, sb)
        assert np.array_equal(fp["states"], ent.serial(data, sb)), (name, sb)
        got = ent.place(data, fp["states"], sb)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), (name, sb)
    return fp


def test_fixed_point_equals_the_serial_decoder_on_every_case(good):
    assert len(good) >= 50
    jumped = 0
    for c in good:
        _check_fixed_point(c["name"], c["data"], orc.coefficients(c["data"])["coef"])
        st = ent.fixed_point(c["data"], 32)["states"]
        jumped += int((st[1:, 0] >= st[:-1, 0] // 32 * 32 + 64).sum())      # a symbol that jumped a whole 32-bit subsequence
    assert jumped > 0


def test_fixed_point_equals_the_serial_decoder_on_the_bench_file(bench):
    fp = _check_fixed_point("bench", bench, orc.coefficients(bench)["coef"])
    assert fp["subseqs"] == 798 and fp["rounds"] <= 16                    # at 1024 bits


def test_too_few_rounds_do_not_converge(bench):
    fp = ent.fixed_point(bench, 1024, max_rounds=1)
    assert not fp["converged"] and fp["rounds"] == 1


def _numpy_unstuff(data, scan_pos):
    """The scan up to the first marker that is no restart marker, without FF00 stuffing and without the restart markers."""
    d = np.frombuffer(data, np.uint8)[scan_pos:]
    ff = np.flatnonzero(d[:-1] == 0xFF)
    nxt = d[ff + 1]
    stop = ff[(nxt != 0) & ~((nxt >= 0xD0) & (nxt <= 0xD7))]
    d = d[:stop[0]] if len(stop) else d
    ff = np.flatnonzero(d[:-1] == 0xFF)
    keep = np.ones(len(d), bool)
    keep[ff[d[ff + 1] == 0] + 1] = False
    rst = ff[(d[ff + 1] >= 0xD0) & (d[ff + 1] <= 0xD7)]
    keep[rst] = False
    keep[rst + 1] = False
    return d[keep].tobytes()


def test_scan_prepare_equals_numpy_and_the_oracle(lib, good, bench):
    for name, data in [(c["name"], c["data"]) for c in good] + [("bench", bench)]:
        r = jpeg.scan_prepare(data)
        f, scan, segs = ent.prepare(data)
        assert r["status"] == jpeg.OK and not r["host"], name
        assert r["scan"] == _numpy_unstuff(data, f["scan"]) == scan, name
        assert [tuple(int(v) for v in s) for s in r["segments"]] == segs and r["expected"] == len(segs), name


def test_restart_fixtures_have_the_expected_segments(lib, good):
    rst3 = [c for c in good if c["name"] == "48x64_420_noise_q75_rst3"][0]
    row = [c for c in good if c["name"] == "50x35_422_noise_q75_rstrow"][0]
    for c in (rst3, row):
        m = jpeg.info(c["data"])
        mw, mh = -(-m["w"] // (8 * m["h_samp"])), -(-m["h"] // (8 * m["v_samp"]))
        interval, mcus = m["restart_interval"], mw * mh
        assert interval == (3 if c is rst3 else mw) and mcus > 2 * interval
        r = jpeg.scan_prepare(c["data"])
        assert len(r["segments"]) == -(-mcus // interval) == r["expected"] and not r["host"]
        assert [int(s[1]) for s in r["segments"]] == list(range(0, mcus, interval))
        assert int(r["segments"][0][0]) == 0 and all(np.diff(r["segments"][:, 0]) > 0)


def test_damaged_restart_markers_mark_the_file_host(lib, good):
    c = [c for c in good if c["name"] == "48x64_420_noise_q75_rst3"][0]
    at = c["data"].index(b"\xff\xd1", c["data"].index(b"\xff\xda"))
    for patch in (b"\xff\xd3", b"\xff\xd0", b"\x12\xd1", b"\xff\xd9"):       # misnumbered twice, damaged, turned into EOI
        e = c["data"][:at] + patch + c["data"][at + 2:]
        r = jpeg.scan_prepare(e)
        assert r["status"] == jpeg.OK and r["host"], patch
        assert jpeg.coefficients(e)["status"] == jpeg.CORRUPT
    fill = c["data"][:at] + b"\xff\xff\xff" + c["data"][at:]                 # fill bytes in front of a marker are legal
    r = jpeg.scan_prepare(fill)
    assert not r["host"] and r["scan"] == jpeg.scan_prepare(c["data"])["scan"]
    assert np.array_equal(r["segments"], jpeg.scan_prepare(c["data"])["segments"])
    extra = c["data"][:-2] + b"\xff\xd3" + c["data"][-2:]                     # a restart marker behind the last segment ends the scan
    r = jpeg.scan_prepare(extra)
    assert not r["host"] and r["scan"] == jpeg.scan_prepare(c["data"])["scan"]


def test_refused_files_and_small_buffers(lib, cases):
    import ctypes
    for c in cases:
        if c["status"] != "ok":
            r = jpeg.scan_prepare(c["data"])
            assert r["status"] == jpeg.UNSUPPORTED and r["reason"] and r["scan"] == b""
    c = [c for c in cases if c["name"].startswith("31x33_420_noise_q30")][0]
    blob = np.frombuffer(c["data"], np.uint8)
    out = np.full(blob.size, 0x5A, np.uint8)
    segs = np.zeros((1, 2), np.int32)
    info4 = np.zeros(4, np.int32)
    rc = lib.yn_jpeg_scan_prepare(blob.ctypes.data, blob.size, out.ctypes.data, 16, segs.ctypes.data, 1, info4.ctypes.data)
    assert rc == jpeg.TOO_LARGE and "bytes" in lib.yn_jpeg_reason(None, 0).decode() and (out == 0x5A).all()


def test_decode_core_is_clean_under_sanitizers(cases, tmp_path):
    """csrc/yn_jpeg_huff.h and the copy pass of csrc/yn_jpeg_host.h on their own (no HIP, no python), under a serial scheduler: every prefix
    and 2000 seeded single-byte corruptions of every stored file, at 32 and 1024 bits per subsequence, under the address and
    undefined-behaviour sanitizers, in a child process.  Every input gives the host's coefficients or the mark "host"."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_huff_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I", os.path.join(ROOT, "yolo-nano_amd", "csrc"), os.path.join(HERE, "jpeg_huff_check.cpp"), "-o", exe])
    blob = str(tmp_path / "files.bin")
    with open(blob, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<I", len(c["data"])))
            f.write(c["data"])
    out = subprocess.run([exe, blob], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    ok = sum(c["status"] == "ok" for c in cases)
    assert out.stdout.startswith("%d files (%d sound ones decoded by the device route)" % (len(cases), ok)) and out.stdout.rstrip().endswith(": ok")


NEW_ENTRIES = ("yn_jpeg_entropy", "yn_jpeg_entropy_stats", "yn_jpeg_device_coefficients", "yn_jpeg_entropy_states", "yn_jpeg_scan_prepare",
               "yn_jpeg_entropy_timing")


def test_header_and_ctypes_table_agree_on_the_new_entries(lib):
    from yolo_nano_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolonano_hip.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, "%s is not declared in yolonano_hip.h" % name
        assert name in capi.SIGNATURES, "%s is missing from capi.SIGNATURES" % name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(capi.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert lib.yn_abi_version() == 2


def test_decoder_arguments_are_checked_before_any_device_is_touched():
    with pytest.raises(ValueError, match="entropy"):
        jpeg.JPEGDecoder(entropy="gpu")
