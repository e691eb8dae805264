// jpeg_huff_check.cpp — a stand-alone driver of the device entropy mode's decode core on the host (csrc/yn_jpeg_huff.h, with the copy pass
// of csrc/yn_jpeg_host.h in front), meant to be built with -fsanitize=address,undefined and run as a child process
// (tests/test_jpeg_entropy_cpu.py).  This is where the bounds of the device code are proven before a GPU sees a damaged file.
//
//     jpeg_huff_check FILES.bin
//
// FILES.bin: uint32 count, then per file uint32 length + the bytes (little endian).  Every stored file, every proper prefix of it and 2000
// seeded single-byte corruptions go through the steps the kernels run, one subsequence index at a time under a serial scheduler (init;
// rounds of pull, then decode; prefix sum; verify; write; DC sums), at 32 and at 1024 bits per subsequence.  Every buffer is a heap
// block of the exact size the device code may touch, so one element too far is a sanitizer report.  For every input the outcome must be the
// host decoder's coefficients, or the mark "host" (the file is left to entropy_decode); OK where the host refuses is an error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "yn_jpeg_host.h"

namespace {

std::atomic<long> g_device{0}, g_host{0}, g_rounds_max{0}, g_prefixes{0}, g_corruptions{0}, g_whole{0};

// true: `coef` holds what the device stage would leave; false: the file is marked "host"
bool device_route(const uint8_t* data, int64_t len, const ynjpeg::Header& H, int sb, std::vector<int16_t>& coef)
{
    using namespace ynhuff;
    const int64_t want = ynjpeg::scan_segments(H), cap = len - H.scan_pos;
    uint8_t* raw = (uint8_t*)malloc(cap ? (size_t)cap : 1);
    std::vector<ynjpeg::ScanSegment> ss((size_t)want);
    ynjpeg::ScanInfo I;
    ynjpeg::scan_prepare(data, len, H, raw, cap, ss.data(), want, I);
    bool ok = !I.host;
    if (ok) {
        const int64_t nwords = (I.bytes + 3) / 4;
        uint32_t* words = (uint32_t*)calloc(nwords ? (size_t)nwords : 1, 4);      // exactly the words of the scan, zero padded
        memcpy(words, raw, (size_t)I.bytes);
        std::vector<Segment> segs((size_t)I.segments);
        int64_t nsub = 0;
        for (int k = 0; k < I.segments; ++k) {
            const int64_t end = k + 1 < I.segments ? ss[(size_t)k + 1].start : I.bytes;
            const int64_t bits = (end - ss[(size_t)k].start) * 8;
            segs[(size_t)k].start = ss[(size_t)k].start; segs[(size_t)k].first_mcu = ss[(size_t)k].first_mcu; segs[(size_t)k].sub0 = (int32_t)nsub; segs[(size_t)k].pad = 0;
            nsub += bits > sb ? (bits + sb - 1) / sb : 1;
        }
        Table* tabs = (Table*)malloc(sizeof(Table) * 2 * (size_t)H.nc);
        for (int c = 0; c < H.nc; ++c) { ynjpeg::huff_table(H.dc[H.td[c]], tabs[2 * c]); ynjpeg::huff_table(H.ac[H.ta[c]], tabs[2 * c + 1]); }
        Geometry G;
        ynjpeg::huff_geometry(H, 0, G);
        uint64_t* start = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)nsub);
        uint64_t* end = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)nsub);
        int32_t* nblk = (int32_t*)malloc(sizeof(int32_t) * (size_t)nsub);
        int32_t* before = (int32_t*)malloc(sizeof(int32_t) * (size_t)nsub);
        Job J;
        J.S.words = words; J.S.nwords = nwords; J.tabs = tabs; J.segs = segs.data(); J.nseg = I.segments; J.nsub = (int32_t)nsub; J.sb = sb;
        J.scan_bits = I.bytes * 8; J.U = G.U; J.L = G.L; J.blocks = G.blocks; J.start = start; J.end = end; J.nblk = nblk;
        for (int32_t i = 0; i < J.nsub; ++i) sync_init(J, i);
        // Jacobi rounds as in the kernel: pull everything, then decode what is dirty.  Only the successor of a subsequence that was decoded
        // can become dirty, so after the first round the pulls are limited to those: the same schedule, without the no-op pulls.
        int flag = 0;
        long rounds = 0;
        std::vector<int32_t> work((size_t)J.nsub), next;
        for (int32_t i = 0; i < J.nsub; ++i) { work[(size_t)i] = i; (void)sync_pull(J, i); }
        while (!work.empty()) {
            if (rounds == J.nsub) { flag = FLAG_ROUNDS; break; }       // max_rounds = the subsequence count: a chain always gets there
            ++rounds;
            for (size_t w = work.size(); w-- > 0;) (void)sync_decode(J, work[w]);      // any order: a round's decodes do not see each other
            next.clear();
            for (int32_t i : work)
                if (i + 1 < J.nsub && sync_pull(J, i + 1)) next.push_back(i + 1);
            work.swap(next);
        }
        for (long seen = g_rounds_max; rounds > seen && !g_rounds_max.compare_exchange_weak(seen, rounds);) {}
        uint32_t sum = 0;
        for (int32_t i = 0; i < J.nsub; ++i) { before[i] = (int32_t)sum; sum += (uint32_t)nblk[i]; }
        for (int32_t i = 0; i < J.nsub; ++i) flag |= verify(J, i, before[i]);
        if (flag & FLAG_ROUNDS) { fprintf(stderr, "no fixed point within as many rounds as subsequences\n"); exit(1); }
        ok = flag == 0;
        if (ok) {
            int16_t* out = (int16_t*)calloc((size_t)H.coef_total ? (size_t)H.coef_total : 1, sizeof(int16_t));
            for (int32_t i = 0; i < J.nsub; ++i) {
                CoefSink sink;
                sink.coef = out; sink.G = &G; sink.zz = ZZ; sink.before = before[i]; sink.cur = -1; sink.blk = nullptr;
                write_span(J, i, sink);
            }
            const int32_t mcus = G.blocks / G.U;                       // DC differences -> values, in decode order per component
            uint16_t pred[3] = {0, 0, 0};
            for (int32_t g = 0; g < G.blocks; ++g) {
                const int32_t mcu = g / G.U, u = g % G.U;
                if (u == 0 && (G.restart ? mcu % G.restart == 0 : mcu == 0)) pred[0] = pred[1] = pred[2] = 0;
                const int c = component_of(G.U, G.L, u);
                int16_t* at = out + block_offset(G, g);
                uint16_t d;
                memcpy(&d, at, 2);
                pred[c] = (uint16_t)(pred[c] + d);
                memcpy(at, &pred[c], 2);
            }
            (void)mcus;
            coef.assign(out, out + H.coef_total);
            free(out);
        }
        free(before); free(nblk); free(end); free(start); free(tabs); free(words);
    }
    free(raw);
    return ok;
}

// both routes on one input; the host's status, and whether the device route took the file
int both(const uint8_t* data, int64_t len, std::vector<int16_t>& coef, const char* what, unsigned file, unsigned n)
{
    static thread_local ynjpeg::Header H;
    std::string reason;
    H = ynjpeg::Header();
    int st = ynjpeg::parse(data, len, H, reason);
    if (st != ynjpeg::JPEG_OK) return st;
    coef.assign((size_t)H.coef_total, 0);
    st = ynjpeg::entropy_decode(data, len, H, coef.data(), reason);
    for (int sb : {32, 1024}) {
        std::vector<int16_t> dev;
        if (device_route(data, len, H, sb, dev)) {
            ++g_device;
            if (st != ynjpeg::JPEG_OK) { fprintf(stderr, "file %u %s %u at %d bits: the device route accepts what the host refuses (%s)\n", file, what, n, sb, reason.c_str()); exit(1); }
            if (dev != coef) { fprintf(stderr, "file %u %s %u at %d bits: other coefficients than the host's\n", file, what, n, sb); exit(1); }
        } else {
            ++g_host;
        }
    }
    return st;
}

uint32_t rd32(FILE* f)
{
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short input\n"); exit(2); }
    return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

// one stored file: whole, every proper prefix, 2000 seeded single-byte corruptions
void one_file(uint32_t i, const std::vector<uint8_t>& file)
{
    const uint32_t len = (uint32_t)file.size();
    std::vector<int16_t> coef;
    std::vector<int16_t> dev;
    static thread_local ynjpeg::Header H;
    std::string reason;
    H = ynjpeg::Header();
    if (ynjpeg::parse(file.data(), len, H, reason) == ynjpeg::JPEG_OK) {       // a sound file must not be left to the host
        for (int sb : {32, 1024})
            if (!device_route(file.data(), len, H, sb, dev)) { fprintf(stderr, "file %u: a sound file was left to the host at %d bits\n", i, sb); exit(1); }
        ++g_whole;
    }
    (void)both(file.data(), len, coef, "whole", i, len);
    for (uint32_t n = 0; n < len; ++n) {
        uint8_t* copy = (uint8_t*)malloc(n ? n : 1);          // exactly n bytes: one byte too far is a heap overflow
        memcpy(copy, file.data(), n);
        (void)both(copy, n, coef, "prefix", i, n);
        free(copy);
        ++g_prefixes;
    }
    uint32_t seed = 12345u + i;
    uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
    for (int k = 0; k < 2000 && len; ++k) {
        memcpy(copy, file.data(), len);
        seed = seed * 1664525u + 1013904223u;
        const uint32_t pos = (seed >> 8) % len;
        seed = seed * 1664525u + 1013904223u;
        copy[pos] = (uint8_t)(seed >> 16);
        (void)both(copy, len, coef, "corruption", i, (unsigned)k);
        ++g_corruptions;
    }
    free(copy);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: jpeg_huff_check FILES.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t count = rd32(f);
    std::vector<std::vector<uint8_t>> files(count);
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t len = rd32(f);
        files[i].resize(len);
        if (len && fread(files[i].data(), 1, len, f) != len) { fprintf(stderr, "short input\n"); return 2; }
    }
    fclose(f);
    unsigned threads = std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : threads > 16 ? 16 : threads;   // the files are independent: one worker each, every check as in a serial run
    ynjpeg::parallel_for((int)count, (int)threads, [&](int i) { one_file((uint32_t)i, files[(size_t)i]); });
    printf("%u files (%ld sound ones decoded by the device route), %ld prefixes, %ld corruptions; device route %ld, host mark %ld, most rounds %ld: ok\n", count,
           g_whole.load(), g_prefixes.load(), g_corruptions.load(), g_device.load(), g_host.load(), g_rounds_max.load());
    return 0;
}
