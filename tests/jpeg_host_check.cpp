// jpeg_host_check.cpp — a stand-alone driver of the host half of the JPEG decode (csrc/yn_jpeg_host.h: marker parser + entropy decoder),
// meant to be built with -fsanitize=address,undefined and run as a child process (tests/test_jpeg_cpu.py).
//
//     jpeg_host_check FILES.bin
//
// FILES.bin: uint32 count, then per file uint32 length + the bytes (little endian).  For every file it decodes every proper prefix and
// 2000 seeded single-byte corruptions; the input copies are heap blocks of the exact length, so a read past the end is a sanitizer report.
// It checks that the whole file decodes, that no prefix that cuts the scan short is accepted with a different result than the full file
// has (a status is all that is asked of the rest), and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "yn_jpeg_host.h"

namespace {

int decode(const uint8_t* data, int64_t len, std::vector<int16_t>& coef, ynjpeg::Header& H)
{
    std::string reason;
    H = ynjpeg::Header();
    int st = ynjpeg::parse(data, len, H, reason);
    if (st != ynjpeg::JPEG_OK) {
        if (reason.empty()) { fprintf(stderr, "a refusal without a reason\n"); exit(2); }
        return st;
    }
    coef.assign((size_t)H.coef_total, 0);
    st = ynjpeg::entropy_decode(data, len, H, coef.data(), reason);
    if (st != ynjpeg::JPEG_OK && reason.empty()) { fprintf(stderr, "a refusal without a reason\n"); exit(2); }
    return st;
}

uint32_t rd32(FILE* f)
{
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short input\n"); exit(2); }
    return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: jpeg_host_check FILES.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t count = rd32(f);
    static ynjpeg::Header H, H2;
    long prefixes = 0, corruptions = 0, accepted = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t len = rd32(f);
        std::vector<uint8_t> file(len);
        if (len && fread(file.data(), 1, len, f) != len) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<int16_t> full, part;
        const int whole = decode(file.data(), len, full, H);
        for (uint32_t n = 0; n < len; ++n) {
            uint8_t* copy = (uint8_t*)malloc(n ? n : 1);          // exactly n bytes: one byte too far is a heap overflow
            memcpy(copy, file.data(), n);
            const int st = decode(copy, n, part, H2);
            free(copy);
            ++prefixes;
            if (st == ynjpeg::JPEG_OK) {                           // only the bytes behind the last MCU (the EOI marker) may be missing
                ++accepted;
                if (whole != ynjpeg::JPEG_OK || part != full) { fprintf(stderr, "file %u: the prefix of %u bytes decodes to something else\n", i, n); return 1; }
            }
        }
        uint32_t seed = 12345u + i;
        uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
        for (int k = 0; k < 2000 && len; ++k) {
            memcpy(copy, file.data(), len);
            seed = seed * 1664525u + 1013904223u;
            const uint32_t pos = (seed >> 8) % len;
            seed = seed * 1664525u + 1013904223u;
            copy[pos] = (uint8_t)(seed >> 16);
            (void)decode(copy, len, part, H2);
            ++corruptions;
        }
        free(copy);
    }
    fclose(f);
    printf("%u files, %ld prefixes (%ld accepted), %ld corruptions: ok\n", count, prefixes, accepted, corruptions);
    return 0;
}
