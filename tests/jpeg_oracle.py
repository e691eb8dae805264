"""Baseline JPEG decode restated in numpy, for the tests of yn_jpeg_* (DESIGN 24): marker parser, bit-at-a-time Huffman decoder,
libjpeg's integer inverse DCT (jidctint: JDCT_ISLOW), its "fancy" chroma upsampling and its YCbCr -> RGB tables as closed forms.
Written from those rules, not from any decoder's source; tests/golden/gen_jpeg.py asserts that it equals PIL (libjpeg-turbo) byte for
byte on every stored case.  Slow on purpose: one bit per step, one block per step.

    coefficients(data) -> dict(w, h, nc, hs, vs, restart, sof, coef=[int16 [bh, bw, 64] per component], qt=uint16 [3, 64], grid=int32 [3, 2])
    decode(data)       -> uint8 [h, w, 3] BGR (a one-component file gives its samples three times, as cv2.imread's default flag)

Unsupported(ValueError) is raised for files the library refuses by design, Corrupt(ValueError) for broken ones."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Unsupported(ValueError):
    pass


class Corrupt(ValueError):
    pass


class _Bits:
    def __init__(self, d, p):
        self.d, self.p, self.acc, self.n = d, p, 0, 0

    def bit(self):
        if self.n == 0:
            if self.p >= len(self.d):
                raise Corrupt("the entropy-coded data ends early")
            b = self.d[self.p]
            if b == 0xFF:
                if self.p + 1 < len(self.d) and self.d[self.p + 1] == 0:
                    self.p += 2
                else:
                    raise Corrupt("the entropy-coded data ends early")
            else:
                self.p += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def get(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def restart(self, m):
        self.n = 0
        if self.p + 1 >= len(self.d) or self.d[self.p] != 0xFF or self.d[self.p + 1] != 0xD0 + m:
            raise Corrupt("a restart marker is missing or misnumbered")
        self.p += 2


def _huffman(counts, syms):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = syms[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _symbol(bits, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise Corrupt("a code that is not in the table")


def _extend(v, s):
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def parse(data):
    """The markers up to the scan -> a dict (w, h, nc, comps, q, hd, ha, restart, sof, scan)."""
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Corrupt("no SOI marker")
    p, q, hd, ha, ri, frame = 2, {}, {}, {}, 0, None
    while True:
        if p + 4 > len(d) or d[p] != 0xFF:
            raise Corrupt("a marker was expected")
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        L = (d[p + 2] << 8) | d[p + 3]
        if L < 2 or p + 2 + L > len(d):
            raise Corrupt("a segment runs past the end of the file")
        seg = d[p + 4:p + 2 + L]
        if m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise Unsupported("sample precision is not 8 bits")
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc not in (1, 3):
                raise Unsupported("%d components" % nc)
            comps = [dict(id=seg[6 + 3 * i], h=seg[7 + 3 * i] >> 4, v=seg[7 + 3 * i] & 15, tq=seg[8 + 3 * i]) for i in range(nc)]
            if nc == 1:
                comps[0]["h"] = comps[0]["v"] = 1
            elif [(c["h"], c["v"]) for c in comps[1:]] != [(1, 1), (1, 1)] or (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)):
                raise Unsupported("sampling factors")
            frame = dict(w=W, h=H, nc=nc, comps=comps, sof=m)
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise Unsupported("progressive JPEG" if m == 0xC2 else "SOF marker %02X" % m)
        elif m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                i += 1
                t = np.zeros(64, np.int64)
                for k in range(64):
                    if pq:
                        t[ZIGZAG[k]] = (seg[i] << 8) | seg[i + 1]
                        i += 2
                    else:
                        t[ZIGZAG[k]] = seg[i]
                        i += 1
                q[tq] = t
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                n = sum(counts)
                (ha if tc else hd)[th] = _huffman(counts, list(seg[i + 17:i + 17 + n]))
                i += 17 + n
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if frame is None:
                raise Corrupt("a scan before the frame header")
            if seg[0] != frame["nc"]:
                raise Unsupported("several scans")
            for i, c in enumerate(frame["comps"]):
                c["td"], c["ta"] = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
            frame.update(q=q, hd=hd, ha=ha, restart=ri, scan=p + 2 + L)
            return frame
        p += 2 + L


def coefficients(data):
    f = parse(data)
    d, W, H, comps = bytes(data), f["w"], f["h"], f["comps"]
    hm, vm = comps[0]["h"], comps[0]["v"]
    mw, mh = -(-W // (8 * hm)), -(-H // (8 * vm))
    coef = [np.zeros((mh * c["v"], mw * c["h"], 64), np.int64) for c in comps]
    pred = [0] * len(comps)
    bits, rst = _Bits(d, f["scan"]), 0
    for mcu in range(mw * mh):
        if f["restart"] and mcu and mcu % f["restart"] == 0:
            bits.restart(rst)
            rst = (rst + 1) & 7
            pred = [0] * len(comps)
        my, mx = divmod(mcu, mw)
        for ci, c in enumerate(comps):
            for v in range(c["v"]):
                for h in range(c["h"]):
                    blk = coef[ci][my * c["v"] + v, mx * c["h"] + h]
                    s = _symbol(bits, f["hd"][c["td"]])
                    if s > 11:
                        raise Corrupt("a DC category above 11")
                    pred[ci] = ((pred[ci] + _extend(bits.get(s), s) + 32768) & 0xFFFF) - 32768
                    blk[0] = pred[ci]
                    k = 1
                    while k < 64:
                        rs = _symbol(bits, f["ha"][c["ta"]])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            if k > 64:
                                raise Corrupt("a zero run past coefficient 63")
                            continue
                        if s > 10:
                            raise Corrupt("an AC category above 10")
                        k += r
                        if k > 63:
                            raise Corrupt("a run past coefficient 63")
                        blk[ZIGZAG[k]] = _extend(bits.get(s), s)
                        k += 1
    qt = np.zeros((3, 64), np.uint16)
    grid = np.zeros((3, 2), np.int32)
    for ci, c in enumerate(comps):
        qt[ci] = f["q"][c["tq"]]
        grid[ci] = coef[ci].shape[:2]
    return dict(w=W, h=H, nc=f["nc"], hs=hm, vs=vm, restart=f["restart"], sof=f["sof"], coef=[c.astype(np.int16) for c in coef], qt=qt, grid=grid)


def idct(c):
    """c int64 [..., 8, 8] dequantised coefficients -> samples 0..255: columns first (descale 11), then rows (descale 18, + 128, clamp)."""
    def one_d(x, shift):                   # along axis -2
        x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., i, :] for i in range(8)]
        z1 = (x2 + x6) * 4433
        t2, t3 = z1 - x6 * 15137, z1 + x2 * 6270
        t0, t1 = (x0 + x4) << 13, (x0 - x4) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = x7, x5, x3, x1
        z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
        z5 = (z3 + z4) * 9633
        a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
        r = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
        return np.stack([(v + (1 << (shift - 1))) >> shift for v in r], -2)
    w = one_d(c, 11)
    o = one_d(np.swapaxes(w, -1, -2), 18)
    return np.clip(np.swapaxes(o, -1, -2) + 128, 0, 255)


def _triangle(a, r_even, r_odd, shift):
    """Horizontal 2x: out[2c] = (3 a[c] + a[c-1] + r_even) >> shift, out[2c+1] = (3 a[c] + a[c+1] + r_odd) >> shift, ends repeated."""
    o = np.zeros((a.shape[0], 2 * a.shape[1]), np.int64)
    prev = np.concatenate([a[:, :1], a[:, :-1]], 1)
    nxt = np.concatenate([a[:, 1:], a[:, -1:]], 1)
    o[:, 0::2] = (3 * a + prev + r_even) >> shift
    o[:, 1::2] = (3 * a + nxt + r_odd) >> shift
    return o


def decode(data):
    f = coefficients(data)
    W, H = f["w"], f["h"]
    full = []
    for ci in range(f["nc"]):
        c = f["coef"][ci].astype(np.int64) * f["qt"][ci].astype(np.int64)
        x = idct(c.reshape(c.shape[0], c.shape[1], 8, 8))
        plane = x.transpose(0, 2, 1, 3).reshape(x.shape[0] * 8, x.shape[1] * 8)
        fh, fv = (1, 1) if ci == 0 else (f["hs"], f["vs"])
        dw, dh = -(-W // fh), -(-H // fv)
        plane = plane[:dh, :dw]                                # the padding of the block grid is never a neighbour
        if (fh, fv) == (1, 1):
            u = plane
        elif dw <= 2:                                          # libjpeg: plain replication for such narrow planes
            u = np.repeat(np.repeat(plane, fv, 0), fh, 1)
        elif (fh, fv) == (2, 1):
            u = _triangle(plane, 1, 2, 2)
        else:
            up = np.concatenate([plane[:1], plane[:-1]], 0)
            down = np.concatenate([plane[1:], plane[-1:]], 0)
            sums = np.zeros((2 * dh, dw), np.int64)
            sums[0::2], sums[1::2] = 3 * plane + up, 3 * plane + down
            u = _triangle(sums, 8, 7, 4)
        full.append(u[:H, :W])
    if f["nc"] == 1:
        return np.repeat(full[0][..., None], 3, -1).astype(np.uint8)
    y, cb, cr = full[0], full[1] - 128, full[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)
