"""Generate tests/golden/jpeg_encode.npz: frames and the JPEG files PIL (libjpeg-turbo) writes from them, the expected output of
yn_jpeg_encode_* and of tests/jpeg_enc_oracle.py.  Needs PIL; the tests do not.

    python tests/golden/gen_jpeg_encode.py

Every case is checked here: jpeg_enc_oracle.encode == Image.fromarray(rgb).save(b, "JPEG", quality=q, subsampling=s) byte for byte, and
the coverage conditions at the end hold (they are asserted from the oracle's statistics: change the inputs, not the conditions).

jpeg_encode.npz:  meta   a JSON list of {name, w, h, quality, sampling ("4:4:4" | "4:2:2" | "4:2:0"), frame, length, md5, stored, stats}
                  frame_<key>  uint8 [h, w, 3] BGR; the key "bench" is not stored: it is what jpeg_bench.jpg decodes to
                  file_<name>  uint8 [length], for the cases with stored = true (files up to 64 KB); the others have length + MD5 only
"""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_enc_oracle as enc  # noqa: E402
import jpeg_oracle  # noqa: E402

PIL_SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
rng = np.random.RandomState(25)


def synth(w, h, kind):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        a = rng.randint(0, 256, (h, w, 3))
    elif kind == "ramp":
        a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], -1)
    elif kind == "flat":
        a = np.ones((h, w, 1), int) * np.array([31, 200, 117])
    elif kind == "blocks":                                   # 8x8 blocks alternating 0 and 255: DC differences of category 11
        a = ((((x // 8) + (y // 8)) % 2) * 255)[..., None] * np.ones(3, int)
    elif kind == "checker":                                  # a one-pixel checkerboard: the largest AC coefficient
        a = (((x + y) % 2) * 255)[..., None] * np.ones(3, int)
    else:
        raise ValueError(kind)
    return a.astype(np.uint8)


def pil_file(bgr, quality, sampling):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(b, "JPEG", quality=quality, subsampling=PIL_SUB[sampling])
    return b.getvalue()


def main():
    frames, plan = {}, []

    def frame(w, h, kind):
        key = "%dx%d_%s" % (w, h, kind)
        if key not in frames:
            frames[key] = synth(w, h, kind)
        return key

    small = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (33, 17), (40, 56), (100, 75)]
    qualities = [1, 30, 75, 95, 100]
    k = 0
    for (w, h) in small:
        for s in ("4:2:0", "4:2:2", "4:4:4"):
            plan.append((frame(w, h, "noise"), qualities[k % 5], s))
            plan.append((frame(w, h, "ramp"), qualities[(k + 2) % 5], s))
            k += 1
    for (w, h) in ((8, 2048), (2048, 8)):                    # one MCU column, one MCU row
        plan.append((frame(w, h, "noise"), 75, "4:2:0"))
        plan.append((frame(w, h, "ramp"), 95, "4:2:2"))
        plan.append((frame(w, h, "flat"), 95, "4:2:0"))
    plan.append((frame(2048, 8, "noise"), 100, "4:4:4"))     # the stuffed bytes
    plan.append((frame(100, 75, "noise"), 30, "4:2:0"))      # the ZRL symbols
    plan.append((frame(100, 75, "noise"), 100, "4:4:4"))     # a dense stream, a sparse one and a flat one of one size
    plan.append((frame(100, 75, "ramp"), 75, "4:4:4"))
    for (w, h) in ((40, 56), (100, 75)):
        for s in ("4:2:0", "4:2:2", "4:4:4"):
            plan.append((frame(w, h, "flat"), 95, s))
    for (w, h, s) in ((2048, 8, "4:4:4"), (40, 56, "4:2:0"), (33, 17, "4:2:2")):
        plan.append((frame(w, h, "blocks"), 100, s))
    for (w, h, s) in ((40, 56, "4:4:4"), (40, 56, "4:2:0"), (17, 33, "4:2:2")):
        plan.append((frame(w, h, "checker"), 100, s))
    bench = jpeg_oracle.decode(open(os.path.join(HERE, "jpeg_bench.jpg"), "rb").read())
    assert bench.shape == (480, 640, 3)
    assert np.array_equal(bench, np.asarray(Image.open(os.path.join(HERE, "jpeg_bench.jpg")))[..., ::-1])
    frames["bench"] = bench
    plan += [("bench", 95, "4:2:0"), ("bench", 30, "4:4:4"), ("bench", 75, "4:2:2")]

    meta, out = [], {}
    for key, q, s in plan:
        bgr = frames[key]
        name = "%s_%s_q%d" % (key, s.replace(":", ""), q)
        if name in [m["name"] for m in meta]:
            continue
        want = pil_file(bgr, q, s)
        got, stats = enc.encode(bgr, q, s)
        assert got == want, name
        assert want[:enc.HEADER_BYTES] == enc.header(bgr.shape[1], bgr.shape[0], q, s)
        stored = len(want) <= 65536
        if stored:
            out["file_" + name] = np.frombuffer(want, np.uint8)
        meta.append(dict(name=name, w=int(bgr.shape[1]), h=int(bgr.shape[0]), quality=q, sampling=s, frame=key, length=len(want),
                         md5=hashlib.md5(want).hexdigest(), stored=stored, stats=stats))
    for key, a in frames.items():
        if key != "bench":
            out["frame_" + key] = a

    st = [m["stats"] for m in meta]
    assert max(x["stuffed"] for x in st) >= 100
    assert max(x["zrl"] for x in st) >= 50
    assert max(x["dc_cat"] for x in st) == 11
    assert max(x["ac_cat"] for x in st) == 10
    assert any(x["dummy_right"] and x["dummy_below"] for x in st)
    assert any(1 <= x["fill_bits"] <= 7 for x in st) and any(x["fill_bits"] == 0 for x in st)

    path = os.path.join(HERE, "jpeg_encode.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(meta), "cases,", sum(not m["stored"] for m in meta), "as length + MD5")
    print("stuffed", max(x["stuffed"] for x in st), "zrl", max(x["zrl"] for x in st))


if __name__ == "__main__":
    main()
