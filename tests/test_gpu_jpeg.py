"""GPU checks of the JPEG route (yn_jpeg_*): the frames the device writes equal the pixels PIL (libjpeg-turbo) decoded
from the same files, byte for byte - stored in tests/golden/jpeg.npz by tests/golden/gen_jpeg.py; nothing here needs PIL."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("jpeg.npz")
    out = []
    for m in json.loads(str(g["meta"])):
        pix = g.get("pix_" + m["name"])
        if pix is not None and pix.ndim == 2:
            pix = np.repeat(pix[..., None], 3, -1)                 # grayscale: cv2.imread's default flag gives the samples three times
        out.append(dict(m, data=g["file_" + m["name"]].tobytes(), pix=pix))
    return out


@pytest.fixture(scope="module")
def good(cases):
    return [c for c in cases if c["status"] == "ok"]


@pytest.fixture(scope="module")
def dec():
    from yolo_nano_amd import jpeg
    d = jpeg.JPEGDecoder(max_batch=32, threads=4)
    yield d
    d.close()


def _same(frame, pix):
    return frame.dtype == torch.uint8 and tuple(frame.shape) == pix.shape and np.array_equal(frame.cpu().numpy(), pix)


def test_every_case_alone_is_exact(dec, good):
    assert len(good) >= 50
    for c in good:
        (f,) = dec.batch([c["data"]])
        assert f.is_cuda and _same(f, c["pix"]), c["name"]


def test_one_call_of_mixed_sizes_and_samplings(dec, good):
    frames = dec.batch([c["data"] for c in good])                 # more than max_batch: two chunks
    assert len(good) > dec.max_batch
    for c, f in zip(good, frames):
        assert _same(f, c["pix"]), c["name"]
    pick = (good[::-1] * 2)[:33]                                  # n = 33 with max_batch = 32: the second chunk holds one image
    frames = dec.batch([c["data"] for c in pick])
    for c, f in zip(pick, frames):
        assert _same(f, c["pix"]), c["name"]
    assert dec.batch([]) == []


def test_refused_files_in_the_middle_leave_their_frames_alone(dec, cases, good):
    from yolo_nano_amd import jpeg
    prog = [c for c in cases if "progressive" in c["tags"]][0]
    cut = [c for c in good if c["name"].startswith("48x64_420_noise")][0]
    m = jpeg.info(cut["data"])
    sos = cut["data"].index(b"\xff\xda")
    truncated = cut["data"][:sos + (len(cut["data"]) - sos) // 2]
    batch = good[:5] + [dict(prog, pix=np.zeros((48, 64, 3), np.uint8))] + good[5:9] + [dict(cut, data=truncated)] + good[9:14]
    bad = {5: jpeg.UNSUPPORTED, 10: jpeg.CORRUPT}
    frames = [torch.full(c["pix"].shape, 0xA5, dtype=torch.uint8, device="cuda") for c in batch]
    assert (m["h"], m["w"]) == tuple(frames[10].shape[:2])
    status, failed = dec.decode_into([c["data"] for c in batch], frames)
    assert failed == 2 and [int(s) for s in status] == [bad.get(i, jpeg.OK) for i in range(len(batch))]
    assert "progressive" in dec.reason(5) and dec.reason(10) and dec.reason(0) == ""
    for i, (c, f) in enumerate(zip(batch, frames)):
        if i in bad:
            assert bool((f == 0xA5).all()), i
        else:
            assert _same(f, c["pix"]), c["name"]
    with pytest.raises(ValueError, match="JPEG 5 is unsupported"):
        dec.batch([c["data"] for c in batch])
    out = dec.batch([c["data"] for c in batch], errors="none")
    assert [i for i, f in enumerate(out) if f is None] == [5, 10] and _same(out[11], batch[11]["pix"])


def test_back_to_back_batches_reuse_the_staging_slots(dec, good):
    a, b, c = good[:20], good[20:45][::-1], good[10:30]
    fa = dec.batch([x["data"] for x in a])                        # no synchronisation in between: three batches over two slots
    fb = dec.batch([x["data"] for x in b])
    fc = dec.batch([x["data"] for x in c])
    for part, frames in ((a, fa), (b, fb), (c, fc)):
        for x, f in zip(part, frames):
            assert _same(f, x["pix"]), x["name"]


def test_bench_image_has_the_recorded_digest(dec, golden):
    from yolo_nano_amd import jpeg
    path = os.path.join(HERE, "golden", "jpeg_bench.jpg")
    want = str(golden("jpeg.npz")["bench_md5"])
    f = jpeg.imread(path)
    assert tuple(f.shape) == (480, 640, 3) and hashlib.md5(f.cpu().numpy().tobytes()).hexdigest() == want
    fs = jpeg.imread_batch([path, open(path, "rb").read()])
    assert all(hashlib.md5(x.cpu().numpy().tobytes()).hexdigest() == want for x in fs)
    t = dec.timing()
    assert set(t) == {"host_ms", "h2d_ms", "kernel_ms"} and all(v >= 0 for v in t.values())


def test_a_batch_beyond_the_staging_fails_before_anything_is_written(good):
    from yolo_nano_amd import capi, jpeg
    big = [c for c in good if c["name"].startswith("48x64_420")][:2]
    need = sum(2 * jpeg.coefficient_count(jpeg.info(c["data"])) for c in big)
    small = jpeg.JPEGDecoder(max_batch=4, threads=1, staging_bytes=need - 128)
    frames = [torch.full(c["pix"].shape, 0xA5, dtype=torch.uint8, device="cuda") for c in big]
    with pytest.raises(capi.YnError, match=str(need)):
        small.decode_into([c["data"] for c in big], frames)
    torch.cuda.synchronize()
    assert all(bool((f == 0xA5).all()) for f in frames)
    out = small.batch([c["data"] for c in big])                   # the Python layer recreates the object with enough staging
    assert small.staging_bytes >= need and all(_same(f, c["pix"]) for f, c in zip(out, big))
    small.close()


def test_val_transforms_take_the_decoded_frames(dec, good):
    from yolo_nano_amd import ValTransforms
    pick = [c for c in good if c["pix"].shape[0] >= 8 and c["pix"].shape[1] >= 8][:12]
    vt = ValTransforms(416)
    frames = dec.batch([c["data"] for c in pick])
    x_dev, s_dev, o_dev = vt.batch(frames)
    x_np, s_np, o_np = vt.batch([c["pix"] for c in pick])
    assert torch.equal(x_dev, x_np)
    assert all(np.array_equal(a, b) for a, b in zip(s_dev, s_np)) and all(np.array_equal(a, b) for a, b in zip(o_dev, o_np))


def test_destroy_returns_the_device_memory(good):
    import ctypes
    from yolo_nano_amd import capi, jpeg
    lib = capi.load_library()

    def live():
        blocks, nbytes = ctypes.c_int64(), ctypes.c_int64()
        assert lib.yn_live_device_memory(ctypes.byref(blocks), ctypes.byref(nbytes)) == 0
        return int(blocks.value), int(nbytes.value)

    warm = jpeg.JPEGDecoder(max_batch=2, threads=1, staging_bytes=1 << 16)      # the bare handle behind it is made once, before the count
    h = warm._h()
    before = live()
    d = jpeg.JPEGDecoder(max_batch=8, threads=2, staging_bytes=1 << 20, handle=h)
    during = live()
    assert during[0] == before[0] + 3 and during[1] >= before[1] + (1 << 20) + (1 << 19)
    assert _same(d.batch([good[3]["data"]])[0], good[3]["pix"])
    d.close()
    assert live() == before
    warm.close()
