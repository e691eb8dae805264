"""GPU checks of the JPEG writer (yn_jpeg_enc_* / yn_jpeg_encode_*): the files the device writes equal the files PIL
(libjpeg-turbo) wrote from the same pixels, byte for byte - stored in tests/golden/jpeg_encode.npz by tests/golden/gen_jpeg_encode.py;
nothing here needs PIL.  Files above 64 KB are stored as length + MD5."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import jpeg_enc_oracle as enc_orc
import jpeg_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases(golden):
    from yolo_nano_amd import jpeg
    g = golden("jpeg_encode.npz")
    bench = jpeg.imread(os.path.join(HERE, "golden", "jpeg_bench.jpg"))      # pinned to PIL's pixels by tests/test_gpu_jpeg.py
    assert hashlib.md5(bench.cpu().numpy().tobytes()).hexdigest() == str(golden("jpeg.npz")["bench_md5"])
    dev = {}
    out = []
    for m in json.loads(str(g["meta"])):
        if m["frame"] not in dev:
            dev[m["frame"]] = bench if m["frame"] == "bench" else torch.from_numpy(g["frame_" + m["frame"]]).cuda()
        out.append(dict(m, key=m["frame"], frame=dev[m["frame"]], data=g["file_" + m["name"]].tobytes() if m["stored"] else None))
    return out


@pytest.fixture(scope="module")
def encoder():
    from yolo_nano_amd import jpeg
    e = jpeg.JPEGEncoder(max_batch=8)
    yield e
    e.close()


def _same(blob, c):
    return len(blob) == c["length"] and hashlib.md5(blob).hexdigest() == c["md5"] and (c["data"] is None or blob == c["data"])


def _explain(e, i, c, blob):
    """Which stage differs: the coefficients of image i of the encoder's last chunk against the oracle's, then the first differing byte."""
    want = enc_orc.coefficients(c["frame"].cpu().numpy(), c["quality"], c["sampling"])["coef"]
    got = e.coefficients(i)
    stage = "entropy stage (the coefficients are equal)"
    for k, (a, b) in enumerate(zip(got, want)):
        if a.shape != b.shape or not np.array_equal(a, b):
            bad = np.argwhere(a != b)[0] if a.shape == b.shape else None
            stage = "pixel stage: component %d, first differing (block row, block column, coefficient) %s" % (k, bad)
            break
    ref = c["data"] if c["data"] is not None else enc_orc.encode(c["frame"].cpu().numpy(), c["quality"], c["sampling"])[0]
    first = next((k for k in range(min(len(blob), len(ref))) if blob[k] != ref[k]), min(len(blob), len(ref)))
    return "%s: %s; %d bytes against %d, first differing byte %d" % (c["name"], stage, len(blob), len(ref), first)


def test_every_case_alone_is_exact(encoder, cases):
    assert len(cases) >= 60
    for c in cases:
        (blob,) = encoder.batch([c["frame"]], quality=c["quality"], sampling=c["sampling"])
        assert _same(blob, c), _explain(encoder, 0, c, blob)


@pytest.mark.parametrize("sampling", ["4:2:0", "4:2:2", "4:4:4"])
def test_one_call_of_mixed_sizes_in_two_chunks(cases, sampling):
    from yolo_nano_amd import jpeg
    for q in (95, 100):
        pick = [c for c in cases if c["sampling"] == sampling and c["quality"] == q]
        assert len(pick) >= 3 and len({(c["w"], c["h"]) for c in pick}) >= 3
        e = jpeg.JPEGEncoder(max_batch=(len(pick) + 1) // 2, quality=q, sampling=sampling)      # two chunks, each a mix of sizes
        assert len(pick) > e.max_batch >= 2 and len(pick) - e.max_batch >= 2
        blobs = e.batch([c["frame"] for c in pick])
        assert len(blobs) == len(pick)
        for c, blob in zip(pick, blobs):
            assert _same(blob, c), c["name"]
        e.close()


def test_one_object_across_growth_and_at_full_capacity():
    """The per-block buffers grow by doubling from 2^14 blocks, and the scan keeps one sum per 2048 blocks plus the total: a call that fills
    the capacity exactly (a whole number of tiles) after a smaller one sized the buffers, then one block group more, which grows them."""
    from yolo_nano_amd import jpeg
    rng = np.random.RandomState(3)
    y, x = np.mgrid[0:512, 0:1024]
    full = np.stack([(x // 4 + y) % 256, (x + y // 2) % 256, rng.randint(0, 256, (512, 1024))], -1).astype(np.uint8)      # 4096 MCUs of 16x8 at 4:2:2
    tiny = rng.randint(0, 256, (8, 8, 3)).astype(np.uint8)
    want_full, want_tiny = enc_orc.encode(full, 75, "4:2:2")[0], enc_orc.encode(tiny, 75, "4:2:2")[0]
    dfull, dtiny = torch.from_numpy(full).cuda(), torch.from_numpy(tiny).cuda()
    e = jpeg.JPEGEncoder(max_batch=4, quality=75, sampling="4:2:2")
    assert e.batch([dtiny]) == [want_tiny]                    # sizes the buffers: 2^14 blocks
    assert e.batch([dfull]) == [want_full]                    # 16384 blocks = 8 whole tiles = the capacity
    assert e.batch([dtiny, dfull, dtiny]) == [want_tiny, want_full, want_tiny]      # 16392 blocks: the buffers grow
    assert e.batch([dfull]) == [want_full] and e.guard_intact()
    e.close()


def test_fetch_follows_the_last_accepted_batch(encoder, cases):
    from yolo_nano_amd import capi, jpeg
    fresh = jpeg.JPEGEncoder(max_batch=2, handle=encoder._h())
    assert fresh.fetch() == []                                # nothing encoded yet
    c = [x for x in cases if x["name"].startswith("40x56_noise_420")][0]
    fresh.encode([c["frame"]], quality=c["quality"], sampling=c["sampling"])
    with pytest.raises(capi.YnError, match="quality 0 outside"):
        fresh.encode([c["frame"]], quality=0)                 # refused: the batch before it is still there
    (blob,) = fresh.fetch()
    assert _same(blob, c)
    assert np.array_equal(fresh.coefficients(0)[0], enc_orc.coefficients(c["frame"].cpu().numpy(), c["quality"], c["sampling"])["coef"][0])
    fresh.close()


def test_the_stream_is_cleared_on_every_call(encoder, cases):
    by = {c["name"]: c for c in cases}
    dense, sparse, flat = by["100x75_noise_444_q100"], by["100x75_ramp_444_q75"], by["100x75_flat_444_q95"]
    for c in (dense, flat, sparse, flat, dense):              # a sparse stream after a dense one: stale bits would be ORed in
        (blob,) = encoder.batch([c["frame"]], quality=c["quality"], sampling=c["sampling"])
        assert _same(blob, c), c["name"]


def test_a_small_buffer_fails_the_fetch_and_writes_nothing_out_of_bounds(cases):
    from yolo_nano_amd import capi, jpeg
    by = {c["name"]: c for c in cases}
    big, tiny = by["100x75_noise_444_q100"], by["8x8_noise_444_q95"]
    assert big["length"] > 16384
    for stream_bytes, frames, bad in ((4096, [big], 0),                                   # the unstuffed stream has no place
                                      (big["length"] - 8, [big], 0),                      # the stream has, the file has not
                                      (4096, [tiny, big, tiny], 1)):
        small = jpeg.JPEGEncoder(max_batch=4, quality=100, sampling="4:4:4", stream_bytes=stream_bytes)
        small.encode([c["frame"] for c in frames])
        with pytest.raises(capi.YnError, match=r"image %d does not fit: the batch needs \d+ output bytes" % bad) as info:
            small.fetch()
        needed = int(str(info.value).split("needs ")[1].split(" ")[0])
        assert needed > stream_bytes and needed >= big["length"] - big["stats"]["stuffed"] and "the encoder has %d" % stream_bytes in str(info.value)
        assert needed == big["length"] or stream_bytes == 4096                            # exact once the stream had room
        assert small.guard_intact()
        small.close()
    small = jpeg.JPEGEncoder(max_batch=4, quality=100, sampling="4:4:4", stream_bytes=4096)
    blobs = small.batch([big["frame"], big["frame"]])         # the Python layer recreates the object with enough room
    assert small.stream_bytes >= 2 * big["length"] and all(_same(b, big) for b in blobs) and small.guard_intact()
    # the caller's buffer: cap below offsets[n]
    small.encode([big["frame"], big["frame"]])
    h = small._h()
    offsets = np.zeros(3, dtype=np.int64)
    host = np.full(big["length"] + 64, 0xA5, dtype=np.uint8)
    assert small.lib.yn_jpeg_encode_fetch(h.h, small.e, offsets.ctypes.data, host.ctypes.data, big["length"] + 10) == 1
    msg = small.lib.yn_last_error(h.h).decode()
    assert "image 1 does not fit the caller's buffer" in msg and str(2 * big["length"]) in msg
    assert list(offsets) == [0, big["length"], 2 * big["length"]] and bool((host == 0xA5).all())
    small.close()


def test_every_refusal_is_raised_by_name(encoder, cases):
    from yolo_nano_amd import capi
    h, lib = encoder._h(), encoder.lib
    f = cases[0]["frame"]
    ptrs = (ctypes.c_void_p * 9)(*([f.data_ptr()] * 9))
    geom = np.array([[f.shape[1], f.shape[0]]] * 9, dtype=np.int32)

    def call(n, p, g, q, s):
        rc = lib.yn_jpeg_encode_batch(h.h, encoder.e, n, ctypes.cast(p, ctypes.c_void_p) if p is not None else None, g.ctypes.data if g is not None else None, q, s)
        return rc, lib.yn_last_error(h.h).decode()

    assert call(1, ptrs, geom, 95, 2)[0] == 0
    for args, words in (((1, None, geom, 95, 2), "null argument"), ((1, ptrs, None, 95, 2), "null argument"), ((-1, ptrs, geom, 95, 2), "negative batch"),
                        ((9, ptrs, geom, 95, 2), "9 images, the encoder was made for 8"), ((1, ptrs, geom, 0, 2), "quality 0 outside 1..100"),
                        ((1, ptrs, geom, 101, 2), "quality 101 outside 1..100"), ((1, ptrs, geom, 95, 3), "unknown sampling 3"),
                        ((1, ptrs, geom, 95, -1), "unknown sampling -1")):
        rc, msg = call(*args)
        assert rc == 1 and words in msg, (args[0], args[3], args[4], msg)
    holes = (ctypes.c_void_p * 3)(f.data_ptr(), f.data_ptr(), None)
    rc, msg = call(3, holes, geom, 95, 2)
    assert rc == 1 and "image 2 has no frame" in msg
    for side in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-3, 8)):
        g = geom.copy()
        g[1] = side
        rc, msg = call(3, ptrs, g, 95, 2)
        assert rc == 1 and "image 1 is %d x %d: a side outside 1..16384" % side in msg, msg
    g = geom.copy()
    g[1] = g[2] = (16384, 16384)                              # 2 x 12.6 M blocks at 4:4:4: beyond what one call stages
    rc, msg = call(3, ptrs, g, 95, 0)
    assert rc == 1 and "image 2 brings the batch to" in msg and "worst case" in msg, msg
    with pytest.raises(capi.YnError, match="quality 0 outside"):
        encoder.batch([f], quality=0)
    with pytest.raises(ValueError, match="4:1:1"):
        encoder.batch([f], sampling="4:1:1")
    with pytest.raises(ValueError, match="frame 0 is not"):
        encoder.batch([f.float()])
    # the object still works, and an empty batch is no error
    assert call(0, None, None, 95, 2)[0] == 0
    offsets = np.full(1, -1, dtype=np.int64)
    assert lib.yn_jpeg_encode_fetch(h.h, encoder.e, offsets.ctypes.data, None, 0) == 0 and offsets[0] == 0
    assert encoder.batch([]) == []
    c = cases[0]
    assert _same(encoder.batch([c["frame"]], quality=c["quality"], sampling=c["sampling"])[0], c)


def test_round_trip_through_the_decoder(cases):
    from yolo_nano_amd import jpeg
    pick = [c for c in cases if c["stored"] and c["w"] * c["h"] <= 7500 and c["name"].split("_")[0] in ("7x5", "33x17", "40x56", "100x75")][::4]
    assert len(pick) >= 5
    for c in pick:
        blob = jpeg.imencode(c["frame"], quality=c["quality"], sampling=c["sampling"])
        assert _same(blob, c), c["name"]
        assert np.array_equal(jpeg.imread(blob).cpu().numpy(), orc.decode(c["data"])), c["name"]


def test_painted_frames_go_to_disk_as_imencode_writes_them(tmp_path, cases):
    from yolo_nano_amd import draw, jpeg
    by = {c["key"]: c for c in cases}
    frames = [by["100x75_ramp"]["frame"].clone(), by["40x56_noise"]["frame"].clone()]
    before = [f.clone() for f in frames]
    rec = torch.tensor([[10, 10, 60, 50, 0.9, 0], [30, 20, 90, 70, 0.8, 1], [4, 6, 30, 40, 0.7, 1]], dtype=torch.float32).cuda()
    vis = draw.Visualizer(["person", "dog"])
    vis.batch(frames, rec, torch.tensor([0, 2, 3], dtype=torch.int32).cuda(), None, pixels=True)
    assert not torch.equal(frames[0], before[0]) and not torch.equal(frames[1], before[1])
    paths = [str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg")]
    jpeg.imwrite(paths[0], frames[0])
    assert open(paths[0], "rb").read() == jpeg.imencode(frames[0])
    jpeg.imwrite_batch(paths, frames, quality=75)
    for p, f in zip(paths, frames):
        blob = open(p, "rb").read()
        assert blob == jpeg.imencode(f, quality=75) and blob[:2] == b"\xff\xd8" and blob[-2:] == b"\xff\xd9"
        assert blob == enc_orc.encode(f.cpu().numpy(), 75, "4:2:0")[0]


def test_close_returns_the_device_memory(cases):
    from yolo_nano_amd import jpeg
    lib = jpeg.capi.load_library()

    def live():
        blocks, nbytes = ctypes.c_int64(), ctypes.c_int64()
        assert lib.yn_live_device_memory(ctypes.byref(blocks), ctypes.byref(nbytes)) == 0
        return int(blocks.value), int(nbytes.value)

    warm = jpeg.JPEGEncoder(max_batch=2, stream_bytes=1 << 16)      # the bare handle behind it is made once, before the count
    h = warm._h()
    before = live()
    e = jpeg.JPEGEncoder(max_batch=8, stream_bytes=1 << 20, handle=h)
    during = live()
    assert during[0] > before[0] and during[1] >= before[1] + (2 << 20)
    c = cases[5]
    assert _same(e.batch([c["frame"]], quality=c["quality"], sampling=c["sampling"])[0], c)
    assert live()[0] == during[0] + 4                         # the per-block buffers came with the first frames
    e.close()
    assert live() == before
    warm.close()
