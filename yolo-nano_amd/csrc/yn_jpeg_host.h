// yn_jpeg_host.h — the host half of the JPEG decode: marker parser and Huffman entropy decoder for baseline files, plain C++
// with no HIP, so that it compiles on its own (tests/jpeg_host_check.cpp builds it under the address and undefined-behaviour sanitizers).
// Output: int16 coefficients in natural (de-zigzagged) order, 64 per block, per component block-row-major over the MCU-padded block grid;
// everything after that (dequantisation, inverse DCT, upsampling, colour) is kernels_jpeg.hip.
// Every read of the input goes through a bounds check; nothing here trusts a length or an index found in the file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "yn_jpeg_huff.h"

namespace ynjpeg {

enum { JPEG_OK = 0, JPEG_UNSUPPORTED = 1, JPEG_CORRUPT = 2, JPEG_TOO_LARGE = 3 };
enum { MAX_SIDE = 16384 };       // per side: a larger frame is refused as too large (JPEG itself allows 65535)

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

enum { LOOK_BITS = 9 };

struct HuffTable {
    bool defined = false;
    uint8_t look_len[1 << LOOK_BITS];     // code length when the code fits the lookahead, else 0
    uint8_t look_sym[1 << LOOK_BITS];
    int32_t maxcode[18];                  // largest code of length l, -1 if none; [17] ends the slow path
    int32_t valoff[17];                   // vals index of the first code of length l, minus that code
    uint8_t vals[256];
};

struct Header {
    int w = 0, h = 0, nc = 0, sof = 0, restart = 0;
    int id[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    int hmax = 1, vmax = 1, mcus_w = 0, mcus_h = 0;
    int bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};        // block grid per component (MCU-padded)
    int64_t coef_off[3] = {0, 0, 0}, coef_total = 0; // in int16 elements
    int64_t scan_pos = 0;                             // first byte of the entropy-coded data
    bool qt_def[4] = {false, false, false, false};
    uint16_t qt[4][64];                               // natural order
    HuffTable dc[4], ac[4];
};

namespace detail {

inline int refuse(std::string& reason, int status, const char* text)
{
    reason = text;
    return status;
}

}  // namespace detail

inline int refuse_null(std::string& reason)
{
    reason = "null input";
    return JPEG_CORRUPT;
}

namespace detail {

// counts[16], then the symbols: canonical codes (ITU T.81 annex C), the lookahead and the slow path's tables.  false: the counts
// describe more codes than their lengths hold
inline bool build_huffman(HuffTable& t, const uint8_t* counts, const uint8_t* syms, int nsyms)
{
    memset(t.look_len, 0, sizeof t.look_len);
    memset(t.look_sym, 0, sizeof t.look_sym);
    memcpy(t.vals, syms, (size_t)nsyms);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        const int c = counts[l - 1];
        if (code + c > (1 << l)) return false;
        for (int i = 0; i < c; ++i, ++k, ++code) {
            if (l <= LOOK_BITS) {
                const int first = code << (LOOK_BITS - l), span = 1 << (LOOK_BITS - l);
                for (int j = 0; j < span; ++j) { t.look_len[first + j] = (uint8_t)l; t.look_sym[first + j] = syms[k]; }
            }
        }
        t.maxcode[l] = c ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.valoff[0] = 0; t.maxcode[0] = -1;
    t.defined = true;
    return true;
}

}  // namespace detail

// The markers up to and including the one SOS.  JPEG_OK: `H` describes a file the entropy decoder and the device pass take.
inline int parse(const uint8_t* d, int64_t n, Header& H, std::string& reason)
{
    using detail::refuse;
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return refuse(reason, JPEG_CORRUPT, "no SOI marker");
    int64_t p = 2;
    bool have_sof = false;
    for (;;) {
        if (p + 2 > n) return refuse(reason, JPEG_CORRUPT, "the file ends before its scan");
        if (d[p] != 0xFF) return refuse(reason, JPEG_CORRUPT, "a marker was expected");
        const int m = d[p + 1];
        if (m == 0xFF) { p += 1; continue; }                                   // fill byte
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { p += 2; continue; }       // stand-alone markers
        if (m == 0xD8) return refuse(reason, JPEG_CORRUPT, "a second SOI marker");
        if (m == 0xD9) return refuse(reason, JPEG_CORRUPT, "EOI before any scan");
        if (m == 0x00) return refuse(reason, JPEG_CORRUPT, "a marker was expected");
        if (p + 4 > n) return refuse(reason, JPEG_CORRUPT, "the file ends inside a segment header");
        const int64_t L = ((int64_t)d[p + 2] << 8) | d[p + 3];
        if (L < 2 || p + 2 + L > n) return refuse(reason, JPEG_CORRUPT, "a segment runs past the end of the file");
        const uint8_t* seg = d + p + 4;
        const int64_t len = L - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof) return refuse(reason, JPEG_CORRUPT, "a second frame header");
            if (len < 6) return refuse(reason, JPEG_CORRUPT, "short frame header");
            if (seg[0] != 8) return refuse(reason, JPEG_UNSUPPORTED, "sample precision is not 8 bits");
            H.h = (seg[1] << 8) | seg[2];
            H.w = (seg[3] << 8) | seg[4];
            const int nc = seg[5];
            if (H.w == 0 || H.h == 0) return refuse(reason, JPEG_CORRUPT, "a frame dimension is 0");
            if (nc == 0) return refuse(reason, JPEG_CORRUPT, "a frame of 0 components");
            if (nc != 1 && nc != 3) return refuse(reason, JPEG_UNSUPPORTED, nc == 4 ? "4 components (CMYK / YCCK)" : "neither 1 nor 3 components");
            if (len != 6 + 3 * nc) return refuse(reason, JPEG_CORRUPT, "frame header length");
            for (int i = 0; i < nc; ++i) {
                H.id[i] = seg[6 + 3 * i];
                H.hs[i] = seg[7 + 3 * i] >> 4;
                H.vs[i] = seg[7 + 3 * i] & 15;
                H.tq[i] = seg[8 + 3 * i];
                if (H.hs[i] < 1 || H.hs[i] > 4 || H.vs[i] < 1 || H.vs[i] > 4) return refuse(reason, JPEG_CORRUPT, "a sampling factor outside 1..4");
                if (H.tq[i] > 3) return refuse(reason, JPEG_CORRUPT, "a quantisation table number above 3");
            }
            if (nc == 1) {
                H.hs[0] = H.vs[0] = 1;             // a one-component scan is not interleaved: one block per MCU whatever the factors say
            } else {
                if (H.hs[1] != 1 || H.vs[1] != 1 || H.hs[2] != 1 || H.vs[2] != 1 ||
                    !((H.hs[0] == 1 && H.vs[0] == 1) || (H.hs[0] == 2 && H.vs[0] == 1) || (H.hs[0] == 2 && H.vs[0] == 2)))
                    return refuse(reason, JPEG_UNSUPPORTED, "sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2)");
            }
            if (H.w > MAX_SIDE || H.h > MAX_SIDE) return refuse(reason, JPEG_TOO_LARGE, "a side above 16384 pixels");
            H.nc = nc; H.sof = m;
            have_sof = true;
        } else if (m == 0xC2 || m == 0xC6) {
            return refuse(reason, JPEG_UNSUPPORTED, "progressive JPEG");
        } else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) {
            return refuse(reason, JPEG_UNSUPPORTED, "lossless JPEG");
        } else if (m == 0xC9 || m == 0xCA || m == 0xCC || m == 0xCD || m == 0xCE) {
            return refuse(reason, JPEG_UNSUPPORTED, "arithmetic coding");
        } else if (m == 0xC5) {
            return refuse(reason, JPEG_UNSUPPORTED, "hierarchical JPEG");
        } else if (m == 0xDB) {
            int64_t i = 0;
            while (i < len) {
                const int pq = seg[i] >> 4, t = seg[i] & 15;
                ++i;
                if (pq > 1 || t > 3) return refuse(reason, JPEG_CORRUPT, "quantisation table header");
                if (i + 64 * (pq + 1) > len) return refuse(reason, JPEG_CORRUPT, "short quantisation table");
                for (int k = 0; k < 64; ++k) {
                    H.qt[t][ZIGZAG[k]] = pq ? (uint16_t)((seg[i] << 8) | seg[i + 1]) : seg[i];
                    i += pq + 1;
                }
                H.qt_def[t] = true;
            }
        } else if (m == 0xC4) {
            int64_t i = 0;
            while (i < len) {
                if (i + 17 > len) return refuse(reason, JPEG_CORRUPT, "short Huffman table");
                const int tc = seg[i] >> 4, th = seg[i] & 15;
                if (tc > 1 || th > 3) return refuse(reason, JPEG_CORRUPT, "Huffman table header");
                int total = 0;
                for (int k = 0; k < 16; ++k) total += seg[i + 1 + k];
                if (total > 256 || i + 17 + total > len) return refuse(reason, JPEG_CORRUPT, "short Huffman table");
                if (!detail::build_huffman(tc ? H.ac[th] : H.dc[th], seg + i + 1, seg + i + 17, total))
                    return refuse(reason, JPEG_CORRUPT, "Huffman code lengths overflow");
                i += 17 + total;
            }
        } else if (m == 0xDD) {
            if (len != 2) return refuse(reason, JPEG_CORRUPT, "restart interval length");
            H.restart = (seg[0] << 8) | seg[1];
        } else if (m == 0xDA) {
            if (!have_sof) return refuse(reason, JPEG_CORRUPT, "a scan before the frame header");
            if (len < 1) return refuse(reason, JPEG_CORRUPT, "short scan header");
            const int ns = seg[0];
            if (ns != H.nc) return refuse(reason, JPEG_UNSUPPORTED, "several scans (the one scan must interleave all components)");
            if (len != 4 + 2 * ns) return refuse(reason, JPEG_CORRUPT, "scan header length");
            for (int i = 0; i < ns; ++i) {
                if (seg[1 + 2 * i] != H.id[i]) return refuse(reason, JPEG_UNSUPPORTED, "scan components out of frame order");
                H.td[i] = seg[2 + 2 * i] >> 4;
                H.ta[i] = seg[2 + 2 * i] & 15;
                if (H.td[i] > 3 || H.ta[i] > 3) return refuse(reason, JPEG_CORRUPT, "a Huffman table number above 3");
                if (!H.dc[H.td[i]].defined || !H.ac[H.ta[i]].defined) return refuse(reason, JPEG_CORRUPT, "a Huffman table is used but never defined");
                if (!H.qt_def[H.tq[i]]) return refuse(reason, JPEG_CORRUPT, "a quantisation table is used but never defined");
            }
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0)
                return refuse(reason, JPEG_UNSUPPORTED, "spectral selection or successive approximation in a sequential scan");
            H.scan_pos = p + 2 + L;
            break;
        }
        // APPn, COM, DNL and everything else: skipped by length
        p += 2 + L;
    }
    H.hmax = H.hs[0]; H.vmax = H.vs[0];
    H.mcus_w = (H.w + 8 * H.hmax - 1) / (8 * H.hmax);
    H.mcus_h = (H.h + 8 * H.vmax - 1) / (8 * H.vmax);
    int64_t off = 0;
    for (int c = 0; c < H.nc; ++c) {
        H.bw[c] = H.mcus_w * H.hs[c];
        H.bh[c] = H.mcus_h * H.vs[c];
        H.coef_off[c] = off;
        off += (int64_t)H.bw[c] * H.bh[c] * 64;
    }
    H.coef_total = off;
    return JPEG_OK;
}

namespace detail {

// Bits of the entropy-coded segment, most significant first.  FF00 is a stuffed FF; any other FFxx is a marker and is not consumed: zero
// bits are fed instead (as at the end of the input) and counted, so that a decoder that USED them can be told from one that only looked ahead.
struct BitReader {
    const uint8_t* d;
    int64_t n, p;
    uint64_t acc = 0;
    int bits = 0, pad = 0;
    BitReader(const uint8_t* data, int64_t len, int64_t pos) : d(data), n(len), p(pos) {}

    void fill()
    {
        while (bits <= 56) {
            unsigned b = 0;
            if (p < n && d[p] != 0xFF) {
                b = d[p]; p += 1;
            } else if (p + 1 < n && d[p + 1] == 0x00) {
                b = 0xFF; p += 2;
            } else {
                pad += 8;
            }
            acc = (acc << 8) | b;
            bits += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)((acc >> (bits - k)) & ((1u << k) - 1u)); }
    void skip(int k) { bits -= k; }
    unsigned get(int k)
    {
        const unsigned v = peek(k);
        bits -= k;
        return v;
    }
    bool overrun() const { return bits < pad; }
    // the byte position after the marker RSTm, or false
    bool restart(int m)
    {
        if (overrun()) return false;
        acc = 0; bits = 0; pad = 0;
        while (p + 1 < n && d[p] == 0xFF && d[p + 1] == 0xFF) p += 1;          // fill bytes
        if (p + 1 >= n || d[p] != 0xFF || d[p + 1] != 0xD0 + m) return false;
        p += 2;
        return true;
    }
};

// one Huffman symbol, -1: the next 16 bits are no code of the table.  At least 16 bits are in the reader.
inline int decode_symbol(BitReader& br, const HuffTable& t)
{
    const unsigned look = br.peek(LOOK_BITS);
    int l = t.look_len[look];
    if (l) {
        br.skip(l);
        return t.look_sym[look];
    }
    for (l = LOOK_BITS + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)br.peek(l);
        if (code <= t.maxcode[l]) {
            br.skip(l);
            return t.vals[(code + t.valoff[l]) & 255];
        }
    }
    return -1;
}

inline int extend(unsigned v, int s) { return v >= (1u << (s - 1)) ? (int)v : (int)v - (1 << s) + 1; }

}  // namespace detail

// The entropy-coded segment -> coef[H.coef_total] (cleared here).
inline int entropy_decode(const uint8_t* d, int64_t n, const Header& H, int16_t* coef, std::string& reason)
{
    using detail::refuse;
    memset(coef, 0, (size_t)H.coef_total * sizeof(int16_t));
    detail::BitReader br(d, n, H.scan_pos);
    uint16_t pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)H.mcus_w * H.mcus_h;
    int next_rst = 0;
    for (int64_t mcu = 0; mcu < mcus; ++mcu) {
        if (H.restart && mcu && mcu % H.restart == 0) {
            if (!br.restart(next_rst)) return refuse(reason, JPEG_CORRUPT, "a restart marker is missing or misnumbered");
            next_rst = (next_rst + 1) & 7;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int my = (int)(mcu / H.mcus_w), mx = (int)(mcu % H.mcus_w);
        for (int c = 0; c < H.nc; ++c) {
            const HuffTable& dct = H.dc[H.td[c]];
            const HuffTable& act = H.ac[H.ta[c]];
            for (int v = 0; v < H.vs[c]; ++v) {
                for (int hh = 0; hh < H.hs[c]; ++hh) {
                    int16_t* blk = coef + H.coef_off[c] + ((int64_t)(my * H.vs[c] + v) * H.bw[c] + (mx * H.hs[c] + hh)) * 64;
                    br.fill();
                    int s = detail::decode_symbol(br, dct);
                    if (s < 0) return refuse(reason, JPEG_CORRUPT, "a code that is not in the DC table");
                    if (s > 11) return refuse(reason, JPEG_CORRUPT, "a DC category above 11");
                    if (s) pred[c] = (uint16_t)(pred[c] + (unsigned)detail::extend(br.get(s), s));      // wraps in 16 bits, unsigned
                    memcpy(blk, &pred[c], sizeof(int16_t));
                    int k = 1;
                    while (k < 64) {
                        br.fill();
                        const int rs = detail::decode_symbol(br, act);
                        if (rs < 0) return refuse(reason, JPEG_CORRUPT, "a code that is not in the AC table");
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;                                                        // EOB
                            k += 16;
                            if (k > 64) return refuse(reason, JPEG_CORRUPT, "a zero run past coefficient 63");
                            continue;
                        }
                        if (s > 10) return refuse(reason, JPEG_CORRUPT, "an AC category above 10");
                        k += r;
                        if (k > 63) return refuse(reason, JPEG_CORRUPT, "a run past coefficient 63");
                        blk[ZIGZAG[k]] = (int16_t)detail::extend(br.get(s), s);
                        ++k;
                    }
                    if (br.overrun()) return refuse(reason, JPEG_CORRUPT, "the entropy-coded data ends early");
                }
            }
        }
    }
    return JPEG_OK;
}

// ---- the host's share of the device entropy mode --------------------------------------------------------------------------
struct ScanSegment {
    uint32_t start;                // first byte of the restart segment in the unstuffed scan
    int32_t first_mcu;
};

struct ScanInfo {
    int64_t bytes = 0;             // unstuffed bytes written
    int32_t segments = 0;
    bool host = false;             // scan_prepare cannot vouch for the file: it takes entropy_decode, which knows the status and the reason
};

enum { SCAN_MAX_BYTES = 1 << 28 };                // beyond that a bit position or a block count could leave 31 bits: the host decodes the file

inline int64_t scan_segments(const Header& H)     // the restart segments a whole scan has
{
    const int64_t mcus = (int64_t)H.mcus_w * H.mcus_h;
    return H.restart ? (mcus + H.restart - 1) / H.restart : 1;
}

// One pass over the entropy-coded data of a parsed file, the copy into the staging slot: byte stuffing goes (FF 00 -> FF), the restart
// markers go and leave the segment table, the copy stops at the first other marker or at the end of the data.  A restart marker counts
// when it is the next one of RST0..7 in order, after any number of FF fill bytes (the rules of BitReader::restart), and a segment is still
// missing.  out[cap] with cap >= n - H.scan_pos always suffices; segs[seg_cap] with seg_cap >= scan_segments(H) likewise.
inline void scan_prepare(const uint8_t* d, int64_t n, const Header& H, uint8_t* out, int64_t cap, ScanSegment* segs, int64_t seg_cap, ScanInfo& I)
{
    I = ScanInfo();
    const int64_t expect = scan_segments(H);
    if (seg_cap < 1 || H.scan_pos > n) { I.host = true; return; }
    int64_t p = H.scan_pos, o = 0, nseg = 1;
    int next_rst = 0;
    segs[0].start = 0; segs[0].first_mcu = 0;
    for (;;) {
        const uint8_t* ff = p < n ? (const uint8_t*)memchr(d + p, 0xFF, (size_t)(n - p)) : nullptr;
        const int64_t run = ff ? ff - (d + p) : n - p;
        if (o + run > cap || o + run >= SCAN_MAX_BYTES) { I.host = true; break; }
        if (run) memcpy(out + o, d + p, (size_t)run);
        o += run; p += run;
        if (p >= n) break;
        if (p + 1 < n && d[p + 1] == 0x00) {                                   // a stuffed FF
            if (o + 1 > cap) { I.host = true; break; }
            out[o++] = 0xFF; p += 2;
            continue;
        }
        int64_t q = p;
        while (q + 1 < n && d[q] == 0xFF && d[q + 1] == 0xFF) q += 1;          // fill bytes
        if (H.restart && nseg < expect && nseg < seg_cap && q + 1 < n && d[q] == 0xFF && d[q + 1] == 0xD0 + next_rst) {
            segs[nseg].start = (uint32_t)o; segs[nseg].first_mcu = (int32_t)(nseg * H.restart);
            ++nseg;
            next_rst = (next_rst + 1) & 7;
            p = q + 2;
            continue;
        }
        break;                                                                 // any other marker ends the scan
    }
    I.bytes = o; I.segments = (int32_t)nseg;
    if (nseg != expect) I.host = true;
}

inline void huff_table(const HuffTable& t, ynhuff::Table& o)
{
    memset(&o, 0, sizeof o);
    for (int i = 0; i < (1 << LOOK_BITS); ++i) o.look[i] = (uint16_t)(t.look_len[i] << 8 | t.look_sym[i]);
    memcpy(o.maxcode, t.maxcode, sizeof o.maxcode);
    memcpy(o.valoff, t.valoff, sizeof o.valoff);
    memcpy(o.vals, t.vals, sizeof o.vals);
}

inline void huff_geometry(const Header& H, const int64_t base, ynhuff::Geometry& G)
{
    G.L = H.hs[0] * H.vs[0]; G.U = G.L + (H.nc == 3 ? 2 : 0);
    G.hs = H.hs[0]; G.vs = H.vs[0]; G.mcus_w = H.mcus_w; G.restart = H.restart;
    G.blocks = (int32_t)((int64_t)H.mcus_w * H.mcus_h * G.U);
    for (int c = 0; c < 3; ++c) { G.bw[c] = H.bw[c]; G.coef_off[c] = base + H.coef_off[c]; }
}

// fn(i) for i in [0, n) on up to `threads` workers (the caller is one of them), one item at a time each
template <typename F>
inline void parallel_for(int n, int threads, F fn)
{
    if (threads > n) threads = n;
    if (threads <= 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
    };
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads - 1);
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

}  // namespace ynjpeg
