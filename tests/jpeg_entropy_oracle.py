"""The subsequence fixed point of the device entropy mode restated on top of jpeg_oracle, for the tests of yn_jpeg_entropy.

    prepare(data)            -> (frame, scan, segments): jpeg_oracle.parse's dict, the entropy-coded data without byte stuffing and restart
                                markers, [(first byte, first MCU)] per restart segment (markers in order, as jpeg_oracle's restart())
    serial(data, sb)         -> the states a serial decoder is in when it crosses each subsequence's first bit: int [n, 4] = bit, unit in
                                the MCU, zigzag index, blocks finished before
    fixed_point(data, sb)    -> dict(states int [n, 4] as above, rounds, decodes, ends): every subsequence but a segment's first starts at
                                its own first bit with u = 0, k = 0; end states go to the successor; whoever's start changed decodes again
    place(data, states, sb)  -> [int16 [bh, bw, 64] per component]: one more decode from `states`, AC values and DC differences stored by
                                block count, then the DC sums per component and restart segment (16-bit wrap-around)

A state is (bit, u, k).  A symbol is only taken when all of it lies inside its restart segment; a decode that meets what jpeg_oracle calls
Corrupt has no end state (None).  Slow on purpose, like jpeg_oracle."""
import numpy as np

import jpeg_oracle as orc


def prepare(data):
    f = orc.parse(data)
    d, p, out, segs, rst = bytes(data), f["scan"], bytearray(), [(0, 0)], 0
    mw, mh = -(-f["w"] // (8 * f["comps"][0]["h"])), -(-f["h"] // (8 * f["comps"][0]["v"]))
    expect = -(-mw * mh // f["restart"]) if f["restart"] else 1
    while p < len(d):
        if d[p] != 0xFF:
            out.append(d[p]); p += 1
        elif p + 1 < len(d) and d[p + 1] == 0:
            out.append(0xFF); p += 2
        elif f["restart"] and len(segs) < expect and p + 1 < len(d) and d[p + 1] == 0xD0 + rst:
            segs.append((len(out), len(segs) * f["restart"])); rst = (rst + 1) & 7; p += 2
        else:
            break
    f.update(mcus=mw * mh, mw=mw, units=[ci for ci, c in enumerate(f["comps"]) for _ in range(c["h"] * c["v"])])
    return f, bytes(out), segs


def spans(scan, segs, sb):
    """[(first bit, limit, segment end, is the segment's first)] per subsequence."""
    out = []
    for s, (start, _) in enumerate(segs):
        end = 8 * (segs[s + 1][0] if s + 1 < len(segs) else len(scan))
        n = max(1, -(-(end - 8 * start) // sb))
        out += [(8 * start + j * sb, min(8 * start + (j + 1) * sb, end), end, j == 0) for j in range(n)]
    return out


def decode_span(f, scan, state, limit, seg_end, put=None):
    """From `state` while its bit < limit -> (end state or None, blocks finished)."""
    p, u, k = state
    U, nb = len(f["units"]), 0

    def bit(q):
        return (scan[q >> 3] >> (7 - (q & 7))) & 1 if q < 8 * len(scan) else 0

    while p < limit:
        c = f["comps"][f["units"][u]]
        table = f["ha"][c["ta"]] if k else f["hd"][c["td"]]
        code, sym, l = 0, None, 0
        while l < 16 and sym is None:
            code = (code << 1) | bit(p + l); l += 1
            sym = table.get((l, code))
        if sym is None:
            if p + 16 > seg_end:
                break
            return None, nb
        if p + l > seg_end:
            break
        r, s, done = (0, sym, False) if k == 0 else (sym >> 4, sym & 15, False)
        if k == 0:
            if s > 11:
                return None, nb
        elif s == 0:
            if r != 15:
                done = True
            elif k + 16 > 64:
                return None, nb
        elif s > 10 or k + r > 63:
            return None, nb
        if p + l + s > seg_end:
            break
        v = 0
        for i in range(s):
            v = (v << 1) | bit(p + l + i)
        if k == 0:
            if put:
                put(nb, 0, orc._extend(v, s))
            k = 1
        elif s == 0:
            k = k + 16 if not done else k
            done = done or k == 64
        else:
            k += r
            if put:
                put(nb, orc.ZIGZAG[k], orc._extend(v, s))
            k += 1
            done = k == 64
        p += l + s
        if done:
            k, u, nb = 0, (u + 1) % U, nb + 1
    return (p, u, k), nb


def serial(data, sb):
    f, scan, segs = prepare(data)
    sp, out, before = spans(scan, segs, sb), [], 0
    for i, (first, limit, seg_end, head) in enumerate(sp):
        state = (first, 0, 0) if head else end
        out.append(state + (before,))
        end, nb = decode_span(f, scan, state, limit, seg_end)
        assert end is not None
        before += nb
    return np.array(out, np.int64)


def fixed_point(data, sb, max_rounds=None):
    f, scan, segs = prepare(data)
    sp = spans(scan, segs, sb)
    n = len(sp)
    start = [(s[0], 0, 0) for s in sp]
    end, nblk = [None] * n, [0] * n
    dirty, rounds, decodes = list(range(n)), 0, 0
    while dirty and (max_rounds is None or rounds < max_rounds):
        rounds += 1
        for i in dirty:                                       # Jacobi: the decodes of a round do not see each other
            end[i], nblk[i] = decode_span(f, scan, start[i], sp[i][1], sp[i][2])
        decodes += len(dirty)
        nxt = []
        for i in dirty:
            if i + 1 < n and not sp[i + 1][3] and end[i] is not None and end[i] != start[i + 1]:
                start[i + 1] = end[i]
                nxt.append(i + 1)
        dirty = nxt
    before = np.concatenate([[0], np.cumsum(nblk)[:-1]]) if n else np.zeros(0)
    states = np.array([s + (int(b),) for s, b in zip(start, before)], np.int64)
    return dict(states=states, rounds=rounds, decodes=decodes, ends=end, converged=not dirty, subseqs=n)


def place(data, states, sb):
    f, scan, segs = prepare(data)
    sp = spans(scan, segs, sb)
    comps, U = f["comps"], len(f["units"])
    coef = [np.zeros((-(-f["mcus"] // f["mw"]) * c["v"], f["mw"] * c["h"], 64), np.int64) for c in comps]

    def block(g):
        mcu, u = divmod(g, U)
        my, mx = divmod(mcu, f["mw"])
        ci = f["units"][u]
        j = u - f["units"].index(ci)
        return coef[ci][my * comps[ci]["v"] + j // comps[ci]["h"], mx * comps[ci]["h"] + j % comps[ci]["h"]]

    for (first, limit, seg_end, _), (p, u, k, before) in zip(sp, states):
        def put(nb, pos, v, before=int(before)):
            if 0 <= before + nb < f["mcus"] * U:
                block(before + nb)[pos] = v
        decode_span(f, scan, (int(p), int(u), int(k)), limit, seg_end, put)
    pred = [0] * len(comps)
    for g in range(f["mcus"] * U):
        mcu, u = divmod(g, U)
        if u == 0 and (mcu % f["restart"] == 0 if f["restart"] else mcu == 0):
            pred = [0] * len(comps)
        ci = f["units"][u]
        pred[ci] = ((pred[ci] + int(block(g)[0]) + 32768) & 0xFFFF) - 32768
        block(g)[0] = pred[ci]
    return [c.astype(np.int16) for c in coef]
