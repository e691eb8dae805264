"""Generate tests/golden/jpeg.npz and tests/golden/jpeg_bench.jpg: JPEG files written by PIL (libjpeg-turbo) with the pixels PIL decodes
from them, the expected output of yn_jpeg_* and of tests/jpeg_oracle.py.  Needs PIL; the tests do not.

    python tests/golden/gen_jpeg.py [path/to/reference]     (default: $YN_REFERENCE, else ../reference beside the repository)

Every case is checked here: jpeg_oracle.decode == PIL byte for byte, and the refusal cases raise.  When the reference checkout is present
its img_files/coco-val/*.jpg are checked the same way; nothing of them is stored.

jpeg.npz:  meta   a JSON list of {name, status ("ok" | "unsupported"), gray, tags}
           file_<name>  uint8 [bytes]     pix_<name>  uint8 [h, w, 3] BGR (RGB reversed), [h, w] for the grayscale file (mode L)
           bench_md5    MD5 of the BGR pixels PIL decodes from jpeg_bench.jpg
"""
import glob
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
import jpeg_oracle  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("YN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
rng = np.random.RandomState(7)


def synth(h, w, kind):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], -1)
    elif kind == "noise":
        a = rng.randint(0, 256, (h, w, 3))
    else:
        a = (((x // 3 + y // 5) % 2) * 255)[..., None] * np.ones(3, int)
        a[..., 1] = 255 - a[..., 1]
        a[..., 2] = rng.randint(0, 256, (h, w))
    return a.astype(np.uint8)


def encode(arr, quality, sub=None, **kw):
    b = io.BytesIO()
    if sub is not None:
        kw["subsampling"] = sub
    (arr if isinstance(arr, Image.Image) else Image.fromarray(arr)).save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def pil_bgr(data):
    im = Image.open(io.BytesIO(data))
    if im.mode == "L":
        return np.asarray(im)
    assert im.mode == "RGB", im.mode
    return np.ascontiguousarray(np.asarray(im)[..., ::-1])


def dqt16(data):
    """The same file with every 8-bit quantisation table rewritten as 16-bit entries (Pq = 1, same values)."""
    out, p = bytearray(data[:2]), 2
    while True:
        m, L = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + L]
        if m == 0xDB:
            body, i = bytearray(), 0
            while i < len(seg):
                assert seg[i] >> 4 == 0
                body.append(0x10 | (seg[i] & 15))
                for v in seg[i + 1:i + 65]:
                    body += bytes([0, v])
                i += 65
            out += bytes([0xFF, 0xDB, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
        else:
            out += data[p:p + 2 + L]
        p += 2 + L
        if m == 0xDA:
            return bytes(out + data[p:])


def bench_image():
    """640x480 of photo-like density: gradients, band-limited texture, a little sensor noise, hard edges."""
    r = np.random.RandomState(11)
    h, w = 480, 640
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([80 + 100 * x / w + 30 * np.sin(y / 37.0), 60 + 120 * y / h + 25 * np.cos(x / 23.0), 140 - 60 * (x + y) / (w + h)], -1)
    for _ in range(40):
        fx, fy, ph, amp = r.uniform(0.02, 0.9), r.uniform(0.02, 0.9), r.uniform(0, 6.28), r.uniform(2, 9)
        img += (amp * np.sin(fx * x + fy * y + ph))[..., None] * r.uniform(0.3, 1.0, 3)
    img += r.normal(0, 5.0, (h, w, 1)) + r.normal(0, 2.0, (h, w, 3))
    for _ in range(25):
        x0, y0, bw, bh = r.randint(0, w - 40), r.randint(0, h - 40), r.randint(10, 160), r.randint(10, 120)
        img[y0:y0 + bh, x0:x0 + bw] = 0.35 * img[y0:y0 + bh, x0:x0 + bw] + r.uniform(0, 170, 3)
    return np.clip(img, 0, 255).astype(np.uint8)


def main():
    cases = []                                             # (name, bytes, status, tags)
    subs = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}
    for (h, w) in [(1, 1), (8, 8), (9, 17), (31, 33), (17, 40), (48, 64), (50, 35)]:
        for tag, sub in subs.items():
            if (h, w) in ((8, 8), (48, 64)) and tag != "420":      # the even sizes once: the file stays under 300 KB
                continue
            for kind, q in [("smooth", 75), ("noise", 30), ("edge", 95)]:
                cases.append(("%dx%d_%s_%s_q%d" % (h, w, tag, kind, q), encode(synth(h, w, kind), q, sub), "ok", []))
    cases.append(("31x33_420_noise_q100", encode(synth(31, 33, "noise"), 100, "4:2:0"), "ok", []))
    cases.append(("31x33_420_noise_q5", encode(synth(31, 33, "noise"), 5, "4:2:0"), "ok", []))
    cases.append(("48x64_420_edge_q85_opt", encode(synth(48, 64, "edge"), 85, "4:2:0", optimize=True), "ok", ["optimize"]))
    cases.append(("48x64_420_noise_q75_rst3", encode(synth(48, 64, "noise"), 75, "4:2:0", restart_marker_blocks=3), "ok", ["restart"]))
    cases.append(("50x35_422_noise_q75_rstrow", encode(synth(50, 35, "noise"), 75, "4:2:2", restart_marker_rows=1), "ok", ["restart"]))
    cases.append(("31x33_gray_noise_q80", encode(synth(31, 33, "noise")[..., 0], 80), "ok", ["gray"]))
    cases.append(("17x40_420_smooth_q75_dqt16", dqt16(encode(synth(17, 40, "smooth"), 75, "4:2:0")), "ok", ["dqt16"]))
    cases.append(("48x64_420_smooth_q75_progressive", encode(synth(48, 64, "smooth"), 75, "4:2:0", progressive=True), "unsupported", ["progressive"]))
    cmyk = Image.frombytes("CMYK", (16, 16), np.concatenate([synth(16, 16, "smooth"), synth(16, 16, "noise")[..., :1]], -1).tobytes())
    cases.append(("16x16_cmyk_q75", encode(cmyk, 75), "unsupported", ["cmyk"]))
    out, meta = {}, []
    for name, data, status, tags in cases:
        entry = dict(name=name, status=status, gray="gray" in tags, tags=tags)
        out["file_" + name] = np.frombuffer(data, np.uint8)
        if status == "ok":
            px = pil_bgr(data)
            mine = jpeg_oracle.decode(data)
            want = px if px.ndim == 3 else np.repeat(px[..., None], 3, -1)
            assert np.array_equal(mine, want), "oracle != PIL on %s" % name
            out["pix_" + name] = px
        else:
            try:
                jpeg_oracle.decode(data)
            except jpeg_oracle.Unsupported:
                pass
            else:
                raise AssertionError("the oracle accepted %s" % name)
        meta.append(entry)
    assert Image.open(io.BytesIO(cases[-1][1])).mode == "CMYK"
    assert dict(Image.open(io.BytesIO(cases[-3][1])).quantization) == dict(Image.open(io.BytesIO(encode(synth(17, 40, "smooth"), 75, "4:2:0"))).quantization)
    bench = encode(bench_image(), 90, "4:2:0")
    assert 100_000 <= len(bench) <= 150_000, len(bench)
    px = pil_bgr(bench)
    assert np.array_equal(jpeg_oracle.decode(bench), px), "oracle != PIL on the bench image"
    open(os.path.join(HERE, "jpeg_bench.jpg"), "wb").write(bench)
    out["bench_md5"] = np.array(hashlib.md5(px.tobytes()).hexdigest())
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "jpeg.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 300_000, os.path.getsize(path)
    print("%d cases, %d bytes of npz, bench %d bytes" % (len(cases), os.path.getsize(path), len(bench)))
    photos = sorted(glob.glob(os.path.join(REF, "img_files", "coco-val", "*.jpg")))
    for p in photos:
        data = open(p, "rb").read()
        assert np.array_equal(jpeg_oracle.decode(data), pil_bgr(data)), "oracle != PIL on %s" % os.path.basename(p)
    print("reference photos checked: %d" % len(photos))


if __name__ == "__main__":
    main()
