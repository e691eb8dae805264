// yn_jpeg_huff.h — the Huffman decode core of the device entropy mode, one text for the kernels (kernels_jpeg_huff.hip) and for
// the host check program (tests/jpeg_huff_check.cpp builds it under the address and undefined-behaviour sanitizers, with a serial scheduler).
//
// The input is a file's UNSTUFFED scan (ynjpeg::scan_prepare: FF00 -> FF, restart markers taken out, zero padded to whole 32-bit words), cut
// into restart segments and those into subsequences of `sb` bits.  A decoder state is (bit position in the file's scan, unit in the MCU u,
// zigzag index k).  decode_span() runs from a state up to a bit limit and either counts the blocks it finishes or also hands every
// coefficient to a sink.  The steps of the subsequence fixed point (sync_init / sync_pull / sync_decode / verify) work on one subsequence
// index each, so a thread per index (device) and a plain loop (host) schedule the same code.
//
// How "nothing is addressed by data" holds here: a word of the scan is read only below the file's word count (Stream::word gives 0 past
// it); table lookups are indexed by 9 bits, by a code length 10..16 and by (code + valoff) & 255; a coefficient is stored at
// block_offset(g) + zz[k & 63] with k < 64 checked and g = a count of finished blocks that the caller's sink checks against the file's
// block count.  Nothing else is indexed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YN_HD __host__ __device__ __forceinline__
#else
#define YN_HD inline
#endif

namespace ynhuff {

// a Huffman table as the decoders read it: the 9-bit lookahead (length << 8 | symbol, 0 = longer code) and the slow path of HuffTable
struct Table {
    uint16_t look[512];
    int32_t maxcode[18];
    int32_t valoff[17];
    uint8_t vals[256];
    uint8_t pad[4];
};
static_assert(sizeof(Table) == 1424 && sizeof(Table) % 16 == 0, "Table is copied to LDS in 32-bit words");

struct Segment {                   // a restart segment of one file
    uint32_t start;                // first byte in the file's unstuffed scan
    int32_t first_mcu;
    int32_t sub0;                  // its first subsequence, counted in the file
    int32_t pad;
};

struct Geometry {                  // where block g of a file goes: entropy_decode's addressing
    int32_t U, L;                  // blocks per MCU; of those, luma (hs * vs)
    int32_t hs, vs, mcus_w, restart;
    int32_t blocks;                // mcus * U
    int32_t bw[3];
    int64_t coef_off[3];           // int16 elements
};

YN_HD int component_of(int U, int L, int u) { return u < L ? 0 : u - L + 1; }

YN_HD int64_t block_offset(const Geometry& G, int32_t g)
{
    const int32_t mcu = g / G.U, u = g - mcu * G.U;
    const int32_t my = mcu / G.mcus_w, mx = mcu - my * G.mcus_w;
    if (u < G.L) {
        const int32_t v = u / G.hs, hh = u - v * G.hs;
        return G.coef_off[0] + ((int64_t)(my * G.vs + v) * G.bw[0] + (mx * G.hs + hh)) * 64;
    }
    const int c = u - G.L + 1;
    return G.coef_off[c] + ((int64_t)my * G.bw[c] + mx) * 64;
}

// ---- states --------------------------------------------------------------------------------------------------------------------------
// packed: bit position (40 bits) | u << 40 (3 bits) | k << 43 (7 bits); NONE: no state (an invalid decode publishes nothing); DIRTY: the
// start state changed and has not been decoded from yet
constexpr uint64_t NONE = 1ull << 62, DIRTY = 1ull << 63;
YN_HD uint64_t pack(int64_t p, int u, int k) { return (uint64_t)p | (uint64_t)u << 40 | (uint64_t)k << 43; }
YN_HD int64_t state_bit(uint64_t s) { return (int64_t)(s & ((1ull << 40) - 1)); }
YN_HD int state_u(uint64_t s) { return (int)(s >> 40) & 7; }
YN_HD int state_k(uint64_t s) { return (int)(s >> 43) & 127; }

struct Stream {
    const uint32_t* words;         // the scan as stored: bytes in file order
    int64_t nwords;
    YN_HD uint32_t word(int64_t i) const
    {
        if (i < 0 || i >= nwords) return 0;
        const uint32_t w = words[i];
        return (w << 24) | ((w & 0xff00u) << 8) | ((w >> 8) & 0xff00u) | (w >> 24);
    }
};

struct NoSink {
    YN_HD void put(int32_t, int, int) {}
};

static const uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};      // zigzag index -> natural index (host copy)

// The bits of one decode: three words of the scan in registers, the third loaded a word ahead of its use, so that a symbol waits for
// memory once per 32 bits at most (a load per symbol, whose address depends on the symbol before, made the decode wait for every one).
struct Reader {
    const Stream& S;
    int64_t wi;
    uint32_t a, b, c;
    YN_HD Reader(const Stream& s, int64_t p) : S(s), wi(p >> 5), a(s.word(p >> 5)), b(s.word((p >> 5) + 1)), c(s.word((p >> 5) + 2)) {}
    YN_HD uint32_t peek32(int64_t p)                       // bits p .. p + 31, most significant first
    {
        const int64_t i = p >> 5;
        if (i != wi) {
            if (i == wi + 1) { a = b; b = c; c = S.word(i + 2); }      // the usual step: a symbol has 27 bits at most
            else { a = S.word(i); b = S.word(i + 1); c = S.word(i + 2); }
            wi = i;
        }
        return (uint32_t)(((uint64_t)a << 32 | b) >> (32 - (int)(p & 31)));
    }
};

YN_HD int extend(uint32_t v, int s) { return v >= (1u << (s - 1)) ? (int)v : (int)v - (1 << s) + 1; }

// Decodes from (p, u, k) while p < limit; a symbol is taken only when all of it (code and value bits) lies below seg_end, the end of the
// restart segment: one that does not leaves the state where it is ("stuck").  tabs[2 c] / tabs[2 c + 1] are the DC / AC tables of
// component c.  *nblk receives the blocks finished; sink.put(blocks finished so far, zigzag index, value) every coefficient, the DC value
// being the DIFFERENCE to its predecessor.  Returns the end state, or NONE for what entropy_decode refuses: a code that is in no table, a
// DC category above 11, an AC size above 10, a run past coefficient 63.
template <typename Sink>
YN_HD uint64_t decode_span(const Stream& S, const Table* tabs, int U, int L, uint64_t from, int64_t limit, int64_t seg_end, int32_t* nblk, Sink& sink)
{
    int64_t p = state_bit(from);
    int u = state_u(from), k = state_k(from);
    int32_t nb = 0;
    *nblk = 0;
    if (u >= U || k > 63) return NONE;
    if (p >= limit) return pack(p, u, k);                  // the start lies beyond the subsequence's own end: the state passes through
    Reader R(S, p);
    while (p < limit) {
        const Table& T = tabs[2 * component_of(U, L, u) + (k ? 1 : 0)];
        const uint32_t win = R.peek32(p);
        const uint32_t e = T.look[win >> 23];
        int l = (int)(e >> 8), sym = (int)(e & 255);
        if (!l) {
            for (l = 10; l <= 16; ++l) {
                const int32_t code = (int32_t)(win >> (32 - l));
                if (code <= T.maxcode[l]) { sym = T.vals[(code + T.valoff[l]) & 255]; break; }
            }
            if (l > 16) {
                if (p + 16 > seg_end) break;               // bits of the next segment were part of the look: stuck, not refused
                return NONE;
            }
        }
        if (p + l > seg_end) break;
        int s, value = 0;
        bool done = false;
        if (k == 0) {
            s = sym;
            if (s > 11) return NONE;
            if (p + l + s > seg_end) break;
            if (s) value = extend((win << l) >> (32 - s), s);
            sink.put(nb, 0, value);
            k = 1;
        } else {
            const int r = sym >> 4;
            s = sym & 15;
            if (s == 0) {
                if (r != 15) {
                    done = true;                           // EOB
                } else {
                    k += 16;
                    if (k > 64) return NONE;
                    done = k == 64;
                }
            } else {
                if (s > 10) return NONE;
                if (k + r > 63) return NONE;
                if (p + l + s > seg_end) break;
                k += r;
                value = extend((win << l) >> (32 - s), s);
                sink.put(nb, k, value);
                ++k;
                done = k == 64;
            }
        }
        p += l + s;
        if (done) {
            k = 0;
            u = u + 1 == U ? 0 : u + 1;
            ++nb;
        }
    }
    *nblk = nb;
    return pack(p, u, k);
}

// ---- the subsequence fixed point of one file ------------------------------------------------------------------------------------------
struct Job {
    Stream S;
    const Table* tabs;             // 2 * components tables
    const Segment* segs;
    int32_t nseg, nsub, sb;        // sb: bits per subsequence, a multiple of 32
    int64_t scan_bits;             // 8 * the unstuffed bytes
    int32_t U, L, blocks;
    uint64_t* start;               // [nsub] the state subsequence i decodes from (| DIRTY)
    uint64_t* end;                 // [nsub] where that decode ended, or NONE
    int32_t* nblk;                 // [nsub] the blocks it finished
};

struct Span {
    int64_t first, limit, seg_end;
    int32_t seg;
    bool head, tail;               // first / last subsequence of its segment
};

YN_HD Span span_of(const Job& J, int32_t i)
{
    int32_t lo = 0, hi = J.nseg - 1;                       // the largest s with segs[s].sub0 <= i
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (J.segs[mid].sub0 <= i) lo = mid; else hi = mid - 1;
    }
    Span sp;
    sp.seg = lo;
    const int32_t j = i - J.segs[lo].sub0;
    const int32_t next = lo + 1 < J.nseg ? J.segs[lo + 1].sub0 : J.nsub;
    sp.seg_end = lo + 1 < J.nseg ? (int64_t)J.segs[lo + 1].start * 8 : J.scan_bits;
    sp.first = (int64_t)J.segs[lo].start * 8 + (int64_t)j * J.sb;
    sp.limit = sp.first + J.sb < sp.seg_end ? sp.first + J.sb : sp.seg_end;
    sp.head = j == 0;
    sp.tail = i + 1 == next;
    return sp;
}

// every subsequence begins at its first bit with u = 0, k = 0: true for the head of a segment, a guess for the others
YN_HD void sync_init(const Job& J, int32_t i)
{
    J.start[i] = pack(span_of(J, i).first, 0, 0) | DIRTY;
    J.end[i] = NONE;
    J.nblk[i] = 0;
}

// takes the predecessor's end state as the start state if it differs; true: subsequence i has to be decoded (again)
YN_HD bool sync_pull(const Job& J, int32_t i)
{
    uint64_t s = J.start[i];
    if (i > 0 && !span_of(J, i).head) {
        const uint64_t e = J.end[i - 1];
        if (e != NONE && e != (s & ~DIRTY)) { s = e | DIRTY; J.start[i] = s; }
    }
    return (s & DIRTY) != 0;
}

YN_HD int sync_decode(const Job& J, int32_t i)
{
    const uint64_t s = J.start[i];
    if (!(s & DIRTY)) return 0;
    const Span sp = span_of(J, i);
    NoSink none;
    int32_t nb = 0;
    J.end[i] = decode_span(J.S, J.tabs, J.U, J.L, s & ~DIRTY, sp.limit, sp.seg_end, &nb, none);
    J.nblk[i] = nb;
    J.start[i] = s & ~DIRTY;
    return 1;
}

enum { FLAG_ROUNDS = 1, FLAG_INVALID = 2, FLAG_PLACE = 4 };      // why a file goes to the host decoder

// after the fixed point, with before = the blocks finished by subsequences 0 .. i - 1: 0 if subsequence i is where entropy_decode would
// have it.  The segment heads pin every segment to its first MCU, the tails ask for a block boundary within the 7 padding bits of the
// segment's last byte, the last subsequence for the file's block count.
YN_HD int verify(const Job& J, int32_t i, int32_t before)
{
    const Span sp = span_of(J, i);
    const uint64_t s = J.start[i], e = J.end[i];
    if (e == NONE || (s & DIRTY)) return FLAG_INVALID;
    int bad = 0;
    if (before % J.U != state_u(s)) bad |= FLAG_PLACE;
    if (sp.head && before != J.segs[sp.seg].first_mcu * J.U) bad |= FLAG_PLACE;
    if (sp.tail && (state_k(e) != 0 || state_u(e) != 0 || sp.seg_end - state_bit(e) >= 8 || state_bit(e) > sp.seg_end)) bad |= FLAG_INVALID;
    if (i + 1 == J.nsub && before + J.nblk[i] != J.blocks) bad |= FLAG_PLACE;
    return bad;
}

// the sink of the write pass: block g = before + the blocks finished so far is stored only while 0 <= g < the file's block count
struct CoefSink {
    int16_t* coef;
    const Geometry* G;
    const uint8_t* zz;             // zigzag index -> natural index, 64 entries
    int32_t before, cur;
    int16_t* blk;
    YN_HD void put(int32_t nb, int k, int value)
    {
        if (nb != cur) {
            cur = nb;
            const int32_t g = before + nb;
            blk = (g >= 0 && g < G->blocks) ? coef + block_offset(*G, g) : nullptr;
        }
        if (blk) blk[zz[k & 63]] = (int16_t)value;
    }
};

// the write pass of subsequence i from its verified state
template <typename Sink>
YN_HD void write_span(const Job& J, int32_t i, Sink& sink)
{
    const Span sp = span_of(J, i);
    int32_t nb = 0;
    (void)decode_span(J.S, J.tabs, J.U, J.L, J.start[i] & ~DIRTY, sp.limit, sp.seg_end, &nb, sink);
}

// one file of a chunk as the kernels find it (filled by jpeg_decode_batch)
struct alignas(16) FileDesc {
    Geometry G;
    int64_t scan_off;              // bytes into the chunk's scan buffer, a multiple of 16
    int64_t scan_bytes;            // unstuffed; the buffer is zeroed up to the next multiple of 16
    int32_t seg0, nseg;            // its segments in the chunk's table
    int32_t sub0, nsub;            // its subsequences in the chunk's state arrays
    int32_t nc;
    int32_t tab[6];                // the chunk's table numbers: DC, AC of component 0, 1, 2
    int32_t pad;
};

struct FileResult {                // the per-file word the host reads back
    int32_t flag;                  // 0: the device's coefficients stand; else FLAG_ bits: the host decodes the file
    int32_t rounds, decodes, nsub;
};

}  // namespace ynhuff
