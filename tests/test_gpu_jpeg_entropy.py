"""GPU checks of the device entropy mode of the JPEG decoder (yn_jpeg_entropy).  The oracle throughout is the host stage
(yn_jpeg_coefficients, the stored pixels, the decoder in its default mode), which is exact: every comparison here is equality."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import jpeg_entropy_oracle as ent

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BENCH = os.path.join(HERE, "golden", "jpeg_bench.jpg")


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("jpeg.npz")
    out = []
    for m in json.loads(str(g["meta"])):
        pix = g.get("pix_" + m["name"])
        if pix is not None and pix.ndim == 2:
            pix = np.repeat(pix[..., None], 3, -1)
        out.append(dict(m, data=g["file_" + m["name"]].tobytes(), pix=pix))
    return out


@pytest.fixture(scope="module")
def good(cases):
    return [c for c in cases if c["status"] == "ok"]


@pytest.fixture(scope="module")
def bench():
    with open(BENCH, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def host_dec():
    from yolo_nano_amd import jpeg
    d = jpeg.JPEGDecoder(max_batch=64, threads=4)
    yield d
    d.close()


def _same(frame, pix):
    return frame.dtype == torch.uint8 and tuple(frame.shape) == pix.shape and np.array_equal(frame.cpu().numpy(), pix)


def _subseqs(data, sb):
    f, scan, segs = ent.prepare(data)
    return len(ent.spans(scan, segs, sb))


@pytest.mark.parametrize("bits", [32, 64, None])
def test_every_case_alone_equals_the_host_stage(good, host_dec, bits):
    from yolo_nano_amd import jpeg
    assert len(good) >= 50
    handle = host_dec._h()
    for c in good:
        sb = bits or 1024
        n = _subseqs(c["data"], sb)
        d = jpeg.JPEGDecoder(max_batch=1, threads=1, staging_bytes=1 << 16, handle=handle, entropy="device", subseq_bits=bits, max_rounds=n)
        (f,) = d.batch([c["data"]])
        assert _same(f, c["pix"]), c["name"]
        st = d.entropy_stats()
        assert st["host_files"] == 0 and st["device_files"] == 1 and st["subseqs_last"] == n and 1 <= st["rounds_last"] <= n, (c["name"], st)
        want = jpeg.coefficients(c["data"])["coef"]
        got = d.device_coefficients(0, jpeg.info(c["data"]))
        assert len(got) == len(want) and all(a.dtype == np.int16 and np.array_equal(a, b) for a, b in zip(got, want)), c["name"]
        fp = ent.fixed_point(c["data"], sb)
        assert np.array_equal(d.entropy_states(0), fp["states"]) and st["rounds_last"] == fp["rounds"], c["name"]
        d.close()


def test_bench_file_at_the_defaults(bench, host_dec):
    from yolo_nano_amd import jpeg
    want = host_dec.batch([bench])[0]
    d = jpeg.JPEGDecoder(max_batch=4, threads=2, handle=host_dec._h(), entropy="device")
    got = d.batch([bench, bench])
    st = d.entropy_stats()
    assert st["host_files"] == 0 and st["device_files"] == 2 and st["subseqs_last"] == 2 * 798, st
    assert 2 * st["rounds_last"] <= 64, st                       # the default bound leaves a margin of at least two
    ref = jpeg.coefficients(bench)["coef"]
    for i in range(2):
        assert torch.equal(got[i], want)
        coef = d.device_coefficients(i, jpeg.info(bench))
        assert all(np.array_equal(a, b) for a, b in zip(coef, ref))
    digest = str(np.load(os.path.join(HERE, "golden", "jpeg.npz"))["bench_md5"])
    assert hashlib.md5(got[1].cpu().numpy().tobytes()).hexdigest() == digest
    t = d.entropy_timing()
    assert set(t) == {"upload_ms", "clear_ms", "first_ms", "sync_ms", "write_ms", "dc_ms", "decodes_per_subseq"} and t["first_ms"] > 0 and t["sync_ms"] > 0 and t["decodes_per_subseq"] >= 1
    assert set(d.timing()) == {"host_ms", "h2d_ms", "kernel_ms"}
    d.close()


def _frames():
    g = torch.Generator().manual_seed(7)
    noise = torch.randint(0, 256, (128, 160, 3), generator=g, dtype=torch.uint8)
    flat = torch.full((128, 160, 3), 128, dtype=torch.uint8)
    half = flat.clone()
    half[:, 80:] = noise[:, 80:]
    return [("flat gray 4:2:0", flat, 95, "4:2:0"), ("noise q95 4:4:4", noise, 95, "4:4:4"), ("half flat half noise", half, 90, "4:2:0")]


def test_frames_of_the_package_encoder(host_dec):
    """Flat gray: a block is a handful of bits, so a subsequence ends over a hundred blocks (the block prefix); noise at q95: long codes."""
    from yolo_nano_amd import jpeg
    d = jpeg.JPEGDecoder(max_batch=4, threads=2, handle=host_dec._h(), entropy="device")
    for name, frame, q, samp in _frames():
        blob = jpeg.imencode(frame.cuda(), quality=q, sampling=samp)
        want = host_dec.batch([blob])[0]
        (got,) = d.batch([blob])
        assert torch.equal(got, want), name
        assert d.entropy_stats()["host_files"] == 0, name
        ref = jpeg.coefficients(blob)["coef"]
        assert all(np.array_equal(a, b) for a, b in zip(d.device_coefficients(0, jpeg.info(blob)), ref)), name
        st = d.entropy_states(0)
        if name.startswith("flat"):
            assert np.diff(st[:, 3]).max() > 100, name
    d.close()


def _compare_with_host(dev, host, blobs, shapes):
    """One decode_into call each: statuses, reasons and frames (refused ones untouched) must be equal."""
    fa = [torch.full(s, 0xA5, dtype=torch.uint8, device="cuda") for s in shapes]
    fb = [torch.full(s, 0xA5, dtype=torch.uint8, device="cuda") for s in shapes]
    sa, na = host.decode_into(blobs, fa)
    sb, nb = dev.decode_into(blobs, fb)
    torch.cuda.synchronize()
    assert na == nb and [int(x) for x in sa] == [int(x) for x in sb]
    for i in range(len(blobs)):
        assert host.reason(i) == dev.reason(i), i
        assert torch.equal(fa[i], fb[i]), i
        if sa[i]:
            assert bool((fb[i] == 0xA5).all()), i
    return sa


def test_one_call_of_everything_mixed(cases, good, host_dec):
    from yolo_nano_amd import jpeg
    bad = [c for c in cases if c["status"] != "ok"]
    batch = good[:20] + bad + good[20:]
    shapes = [c["pix"].shape if c["pix"] is not None else (16, 16, 3) for c in batch]
    d = jpeg.JPEGDecoder(max_batch=64, threads=4, handle=host_dec._h(), entropy="device")
    st = _compare_with_host(d, host_dec, [c["data"] for c in batch], shapes)
    assert [int(s) for s in st] == [jpeg.OK if c["status"] == "ok" else jpeg.UNSUPPORTED for c in batch]
    stats = d.entropy_stats()
    assert stats["device_files"] == len(good) and stats["host_files"] == 0
    small = jpeg.JPEGDecoder(max_batch=7, threads=2, handle=host_dec._h(), entropy="device")      # the same in chunks of 7
    _compare_with_host(small, host_dec, [c["data"] for c in batch], shapes)
    frames = small.batch([c["data"] for c in good])
    assert all(_same(f, c["pix"]) for f, c in zip(frames, good))
    small.close()
    d.close()


def test_too_few_rounds_fall_back_to_the_host(bench, host_dec):
    from yolo_nano_amd import capi, jpeg
    want = host_dec.batch([bench])[0]
    d = jpeg.JPEGDecoder(max_batch=2, threads=2, handle=host_dec._h(), entropy="device", max_rounds=1)
    (got,) = d.batch([bench])
    st = d.entropy_stats()
    assert st["host_files"] == 1 and st["device_files"] == 0 and st["rounds_last"] == 1
    assert torch.equal(got, want)
    with pytest.raises(capi.YnError, match="host decoder"):
        d.device_coefficients(0, jpeg.info(bench))
    d.close()


def test_damaged_scans_equal_the_host_mode(good, host_dec):
    """64 seeded single-byte corruptions inside the scan of a restart file and of a 4:4:4 file, two calls of 64 (the bounds of the device
    code on such input are proven on the host first: tests/test_jpeg_entropy_cpu.py)."""
    from yolo_nano_amd import jpeg
    d = jpeg.JPEGDecoder(max_batch=64, threads=4, handle=host_dec._h(), entropy="device")
    for name in ("48x64_420_noise_q75_rst3", "31x33_444_noise_q30"):
        c = [c for c in good if c["name"] == name][0]
        rng = np.random.RandomState(len(name))
        sos = c["data"].index(b"\xff\xda")
        scan0 = sos + 2 + ((c["data"][sos + 2] << 8) | c["data"][sos + 3])
        blobs = []
        for _ in range(64):
            e = bytearray(c["data"])
            e[int(rng.randint(scan0, len(e) - 2))] = int(rng.randint(0, 256))
            blobs.append(bytes(e))
        st = _compare_with_host(d, host_dec, blobs, [c["pix"].shape] * 64)
        assert 0 < int((np.asarray(st) == jpeg.OK).sum()) and d.entropy_stats()["device_files"] > 0, name
    d.close()


def test_back_to_back_batches_and_memory(good):
    from yolo_nano_amd import capi, jpeg
    lib = capi.load_library()

    def live():
        blocks, nbytes = ctypes.c_int64(), ctypes.c_int64()
        assert lib.yn_live_device_memory(ctypes.byref(blocks), ctypes.byref(nbytes)) == 0
        return int(blocks.value), int(nbytes.value)

    warm = jpeg.JPEGDecoder(max_batch=2, threads=1, staging_bytes=1 << 16)
    h = warm._h()
    before = live()
    d = jpeg.JPEGDecoder(max_batch=32, threads=2, staging_bytes=1 << 20, handle=h, entropy="device")
    assert live()[0] > before[0] + 3                              # the scans, tables and result words on top of the host mode's three blocks
    a, b, c = good[:20], good[20:45][::-1], good[10:30]
    fa = d.batch([x["data"] for x in a])                          # three batches over the two staging slots
    fb = d.batch([x["data"] for x in b])
    fc = d.batch([x["data"] for x in c])
    for part, frames in ((a, fa), (b, fb), (c, fc)):
        for x, f in zip(part, frames):
            assert _same(f, x["pix"]), x["name"]
    assert d.entropy_stats()["device_files"] == 65 and d.entropy_stats()["host_files"] == 0
    d.close()
    assert live() == before
    warm.close()


def test_setter_refuses_values_out_of_range(host_dec):
    from yolo_nano_amd import jpeg
    for kw in (dict(subseq_bits=48), dict(subseq_bits=-32), dict(max_rounds=-1), dict(subseq_bits=1 << 21)):
        with pytest.raises(ValueError, match="yn_jpeg_entropy"):
            jpeg.JPEGDecoder(max_batch=2, threads=1, staging_bytes=1 << 16, handle=host_dec._h(), entropy="device", **kw)
    assert host_dec.entropy_stats() == {"device_files": 0, "host_files": 0, "rounds_last": 0, "subseqs_last": 0}
