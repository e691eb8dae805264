"""Baseline JPEG encode restated in numpy, for the tests of yn_jpeg_enc_* / yn_jpeg_encode_* (DESIGN 25): libjpeg's rgb_ycc_convert, its
edge expansion and chroma downsampling, jfdctint (JDCT_ISLOW), quantisation, jccoefct's dummy blocks, Annex K Huffman coding, byte
stuffing and the 623-byte header.  Written from those rules, not from any encoder's source; tests/golden/gen_jpeg_encode.py asserts that
encode() equals the file PIL (libjpeg-turbo) writes, byte for byte, on every stored case.

    quant_tables(quality)                    -> uint16 [2, 64] natural order (jpeg_set_quality(q, TRUE))
    header(w, h, quality, sampling)          -> the 623 bytes up to and including the SOS segment
    coefficients(bgr, quality, sampling)     -> dict(coef=[int16 [bh, bw, 64] natural order per component, MCU-padded grid], qt uint16 [3, 64],
                                                     grid int32 [3, 2], dummy=(blocks beyond the right edge, blocks beyond the bottom edge))
    encode(bgr, quality=95, sampling="4:2:0") -> (file bytes, stats)     stats: stuffed, zrl, dc_cat, ac_cat, dummy_right, dummy_below, fill_bits

sampling is "4:4:4", "4:2:2" or "4:2:0" (or PIL's 0, 1, 2)."""
import numpy as np

from jpeg_oracle import ZIGZAG

SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2)}

# Annex K.1, in the zigzag order a DQT segment stores
BASE_Q = [[16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51, 56, 55, 64, 72,
           92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99],
          [17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99] + [99] * 48]
# Annex K.3: (class << 4 | id, the 16 code counts, the symbols)
DHT = [
    (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], "000102030405060708090a0b"),
    (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
     "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
     "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
     "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], "000102030405060708090a0b"),
    (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
     "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
     "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
     "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
]
HEADER_BYTES = 623


def quant_tables(quality):
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    out = np.zeros((2, 64), np.uint16)
    for t in range(2):
        for k in range(64):
            out[t, ZIGZAG[k]] = min(max((BASE_Q[t][k] * scale + 50) // 100, 1), 255)
    return out


def _codes(counts, syms):
    """symbol -> (code, length), the canonical assignment of Annex C."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[syms[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def _code_arrays():
    out = []
    for _, counts, syms in DHT:
        code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
        for s, (c, n) in _codes(counts, list(bytes.fromhex(syms))).items():
            code[s], length[s] = c, n
        out.append((code, length))
    return out          # DC0, AC0, DC1, AC1


def header(w, h, quality, sampling):
    hs, vs = SAMPLINGS[sampling]
    qt = quant_tables(quality)
    b = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        b += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(qt[t, ZIGZAG[k]]) for k in range(64))
    b += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, counts, syms in DHT:
        body = bytes([tc]) + bytes(counts) + bytes.fromhex(syms)
        b += b"\xff\xc4" + bytes([(len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
    b += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(b) == HEADER_BYTES
    return bytes(b)


def _fdct_1d(d, first):
    """jfdctint's pass along the last axis: int64 [..., 8] -> [..., 8]."""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    n = 11 if first else 15
    z1 = (t12 + t13) * 4433
    o[2], o[6] = descale(z1 + t13 * 6270, n), descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def _edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def coefficients(bgr, quality, sampling):
    hs, vs = SAMPLINGS[sampling]
    bgr = np.asarray(bgr)
    H, W = bgr.shape[:2]
    B, G, R = [bgr[..., i].astype(np.int64) for i in range(3)]
    planes = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
              (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
              (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16]
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
    qt2 = quant_tables(quality)
    coef, grid = [], np.zeros((3, 2), np.int32)
    dummy_right = dummy_below = 0
    for ci, p in enumerate(planes):
        ch, cv = (hs, vs) if ci == 0 else (1, 1)
        fh, fv = hs // ch, vs // cv                                    # how far this component is downsampled
        wib, hib = -(-W * ch // (8 * hs)), -(-H * cv // (8 * vs))      # the blocks that hold image samples
        p = _edge(p, -(-H // fv) * fv, wib * 8 * fh)                   # rule 1, and the first half of rule 2
        if (fh, fv) == (2, 2):
            bias = np.tile([1, 2], p.shape[1] // 4)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif (fh, fv) == (2, 1):
            bias = np.tile([0, 1], p.shape[1] // 4)
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        p = _edge(p, hib * 8, wib * 8) - 128                           # the second half of rule 2, the level shift
        blocks = p.reshape(hib, 8, wib, 8).transpose(0, 2, 1, 3)
        f = _fdct_1d(blocks, True)                                     # rows
        f = _fdct_1d(f.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)      # columns
        q = qt2[min(ci, 1)].astype(np.int64).reshape(8, 8) * 8
        real = np.sign(f) * ((np.abs(f) + (q >> 1)) // q)
        full = np.zeros((mh * cv, mw * ch, 8, 8), np.int64)
        full[:hib, :wib] = real
        if (mh * cv, mw * ch) != (hib, wib):                           # rule 3: dummy blocks, in the block order of an MCU
            for my in range(mh):
                for mx in range(mw):
                    prev = None
                    for v in range(cv):
                        for h in range(ch):
                            by, bx = my * cv + v, mx * ch + h
                            if by >= hib or bx >= wib:
                                full[by, bx] = 0
                                full[by, bx, 0, 0] = prev
                                dummy_right += bx >= wib
                                dummy_below += by >= hib
                            prev = full[by, bx, 0, 0]
        coef.append(full.reshape(mh * cv, mw * ch, 64).astype(np.int16))
        grid[ci] = (mh * cv, mw * ch)
    return dict(coef=coef, qt=np.stack([qt2[0], qt2[1], qt2[1]]), grid=grid, dummy=(int(dummy_right), int(dummy_below)), hs=hs, vs=vs, mw=mw, mh=mh)


def scan_order(c):
    """The coefficient stage in the order of the stream: int64 [blocks, 64] zigzag, and each block's component."""
    hs, vs, mw, mh = c["hs"], c["vs"], c["mw"], c["mh"]
    parts, comp = [], []
    for ci, a in enumerate(c["coef"]):
        ch, cv = (hs, vs) if ci == 0 else (1, 1)
        a = a.astype(np.int64)[..., ZIGZAG].reshape(mh, cv, mw, ch, 64).transpose(0, 2, 1, 3, 4).reshape(mh * mw, cv * ch, 64)
        parts.append(a)
        comp += [ci] * (cv * ch)
    zz = np.concatenate(parts, 1)
    return zz.reshape(-1, 64), np.tile(np.array(comp), mh * mw)


def _bit_length(a):
    n = np.zeros(a.shape, np.int64)
    a = a.copy()
    while a.any():
        n += a > 0
        a >>= 1
    return n


def entropy(zz, comp):
    """Blocks in scan order -> (unstuffed bytes, bits used, stats).  Every (block, position) gets its code bits and their length, as the
    device does; the stream is their concatenation."""
    dc0, ac0, dc1, ac1 = _code_arrays()
    N = zz.shape[0]
    chroma = comp > 0
    v = zz.copy()
    for ci in range(3):                                               # DC differences per component, in scan order
        idx = np.nonzero(comp == ci)[0]
        dc = zz[idx, 0]
        v[idx, 0] = dc - np.concatenate([[0], dc[:-1]])
    size = _bit_length(np.abs(v))
    extra = np.where(v < 0, v - 1, v) & ((1 << size) - 1)
    code, length = np.zeros((N, 64), np.int64), np.zeros((N, 64), np.int64)
    # DC
    code[:, 0] = np.where(chroma, dc1[0][size[:, 0]], dc0[0][size[:, 0]])
    length[:, 0] = np.where(chroma, dc1[1][size[:, 0]], dc0[1][size[:, 0]])
    # AC: the run of a non-zero coefficient is the distance to the previous non-zero one (position 0 counts as one)
    pos = np.arange(64)[None, :]
    nz = v != 0
    nz[:, 0] = True
    last = np.maximum.accumulate(np.where(nz, pos, 0), 1)
    prev = np.concatenate([np.zeros((N, 1), np.int64), last[:, :-1]], 1)
    run = pos - prev - 1
    ac = nz.copy()
    ac[:, 0] = False
    sym = ((run & 15) << 4) | size
    ch2 = np.broadcast_to(chroma[:, None], (N, 64))
    code[ac] = np.where(ch2, ac1[0][sym], ac0[0][sym])[ac]
    length[ac] = np.where(ch2, ac1[1][sym], ac0[1][sym])[ac]
    zrl = np.where(ac, run >> 4, 0)
    zc, zl = np.where(ch2, ac1[0][0xF0], ac0[0][0xF0]), np.where(ch2, ac1[1][0xF0], ac0[1][0xF0])
    eob = v[:, 63] == 0
    code[eob, 63] = np.where(chroma, ac1[0][0], ac0[0][0])[eob]
    length[eob, 63] = np.where(chroma, ac1[1][0], ac0[1][0])[eob]
    # pieces in stream order: up to three ZRL codes, the code, the extra bits
    piece_code = np.stack([zc, zc, zc, code, extra], -1)
    piece_len = np.stack([zl * (zrl > 0), zl * (zrl > 1), zl * (zrl > 2), length, np.where(nz, size, 0)], -1)
    piece_code, piece_len = piece_code.reshape(-1), piece_len.reshape(-1)
    keep = piece_len > 0
    piece_code, piece_len = piece_code[keep], piece_len[keep]
    total = int(piece_len.sum())
    start = np.cumsum(piece_len) - piece_len
    which = np.repeat(np.arange(piece_len.size), piece_len)
    j = np.arange(total) - start[which]
    bits = ((piece_code[which] >> (piece_len[which] - 1 - j)) & 1).astype(np.uint8)
    fill = (-total) % 8
    raw = np.packbits(np.concatenate([bits, np.ones(fill, np.uint8)]))
    stats = dict(zrl=int(zrl.sum()), dc_cat=int(size[:, 0].max()), ac_cat=int(np.where(ac, size, 0).max()), fill_bits=int(fill), bits=total)
    return raw, stats


def stuff(raw):
    ff = np.nonzero(raw == 0xFF)[0]
    return np.insert(raw, ff + 1, 0), int(ff.size)


def encode(bgr, quality=95, sampling="4:2:0"):
    bgr = np.asarray(bgr)
    c = coefficients(bgr, quality, sampling)
    zz, comp = scan_order(c)
    raw, stats = entropy(zz, comp)
    body, stuffed = stuff(raw)
    stats.update(stuffed=stuffed, dummy_right=c["dummy"][0], dummy_below=c["dummy"][1])
    return header(bgr.shape[1], bgr.shape[0], quality, sampling) + body.tobytes() + b"\xff\xd9", stats
