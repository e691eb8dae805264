// kernels_chip.hip — detections cut out of uint8 BGR device frames as fixed-size chips, straight from the record list: the state behind
// yn_chip.  DESIGN.md §32 is the specification; tests/chip_oracle.py restates it one record at a time.
//
//   chip_select_kernel    one workgroup per frame walks the frame's records in list order, 256 at a time (draw_prims_kernel's recipe):
//                         the filter (score > min_score, class, class_keep), un-letterbox (or take pixels), int() of every coordinate,
//                         margin and clip in integers, the fit into the cw x ch chip, and an order-preserving compaction (ballot +
//                         prefix popcount, a running base; no atomic decides a position) into the frame's descriptor list
//                         desc[start .. start + count)
//   chip_scan_kernel      one workgroup: the exclusive scan of the B frame counts = the dense slot base of every frame, clamped to
//                         max_chips -> chip_offsets, and the counters
//   chip_resample_kernel  the hot path, a fixed grid striding over the work items (slot, run of 256 four-pixel groups of the chip);
//                         the count is read on the device.  The column table of the chip (sx, a0, a1 per destination column) is
//                         computed once per item in LDS and a thread's row values once in registers, with prep_sample's operations in
//                         prep_sample's order (yn_prep.h): the output bits are prep_sample's.  A thread produces four adjacent columns
//                         of one row: one 16-byte store per plane (f32) or three dword stores (u8).
//
// The source rectangle is read in place, byte-granular, at whatever alignment the frame has; a pad pixel loads nothing.  Slots at or
// past the count are not written in any output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "yn_eval_shared.h"
#include "yn_internal.h"
#include "yn_prep.h"

namespace ynk {

namespace {

constexpr int CHIP_THREADS = 256;                // evs::ordered_rank's and evs::block_scan_incl's workgroup
constexpr int CHIP_FRAMES = 32;                 // frames per select launch (descriptors travel in the kernel arguments)
constexpr int CHIP_DESC = 12;                   // int32 words per descriptor: x, y, sw, sh, rw, rh, left, top | record, pitch, pointer lo, hi
constexpr int CHIP_MAX_W = 1024;                // widest chip: the column table's size
constexpr int CHIP_MAX_B = 1024;                // frames per batch: the scan's four frames per thread
constexpr int CHIP_GRID = 2048;                 // resample workgroups: 8 per CU of a 256-CU device, each striding over the items
constexpr int CHIP_LETTERBOX = 0, CHIP_U8 = 0;  // YN_CHIP_LETTERBOX, YN_CHIP_U8 (yn_api.hip asserts the values); spaces: 0 letterbox, 1 pixels

__device__ __forceinline__ long long lmin(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long lmax(long long a, long long b) { return a > b ? a : b; }

struct ChipFrames {
    const unsigned char* p[CHIP_FRAMES];
    int32_t g[CHIP_FRAMES][7];                  // w0, h0, rw, rh, left, top, side
};

struct ChipRule {
    int32_t cw, ch, fit, format, margin_px, margin_permille, min_side, C;
    float min_score, fill[3], mean[3], std[3];
};

// stat: [0] chips, [1] skipped, [2] overflow, [3] range mark.  book [2][bcap]: start and count of every frame's descriptor list.
__global__ __launch_bounds__(CHIP_THREADS) void chip_select_kernel(ChipFrames fr, int frame0, int B, int bcap, const float* __restrict__ rec,
                                                                   const int32_t* __restrict__ offsets, long long rec_capacity, int space,
                                                                   ChipRule rule, const unsigned char* __restrict__ class_keep,
                                                                   int32_t* __restrict__ desc, int32_t* __restrict__ book,
                                                                   unsigned long long* __restrict__ stat)
{
    __shared__ int wsum[CHIP_THREADS / 64];
    const int f = blockIdx.x, b = frame0 + f;
    if (offsets[B] < 0) {                       // the split-f16 range mark: the records are not valid, no chip is cut
        if (threadIdx.x == 0) { book[b] = 0; book[bcap + b] = 0; atomicOr(&stat[3], 1ull); }
        return;
    }
    long long lo = offsets[b], hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > rec_capacity ? rec_capacity : lo);      // never a read past the record buffer, whatever the offsets hold
    hi = hi < lo ? lo : (hi > rec_capacity ? rec_capacity : hi);
    int32_t g[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) g[i] = fr.g[f][i];
    const long long w0 = g[0], h0 = g[1];
    const uintptr_t img = (uintptr_t)fr.p[f];
    int running = 0, skipped = 0;
    for (long long base = lo; base < hi; base += CHIP_THREADS) {
        const long long i = base + threadIdx.x;
        bool use = false;
        int32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i < hi) {
            float r[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) r[c] = rec[i * 6 + c];
            if (r[4] > rule.min_score) {        // strict, so a NaN score is not selected (and not counted)
                const bool cls_ok = r[5] >= 0.0f && r[5] < (float)rule.C && r[5] == truncf(r[5]);
                if (!cls_ok) {
                    ++skipped;
                } else if (class_keep[(int)r[5]]) {
                    float m[4];
                    if (space == 0) evs::unletterbox(r, g, m);
                    else { m[0] = r[0]; m[1] = r[1]; m[2] = r[2]; m[3] = r[3]; }
                    bool ok = true;
#pragma unroll
                    for (int c = 0; c < 4; ++c) ok = ok && fabsf(m[c]) < 1073741824.0f;      // false for NaN and the infinities
                    if (ok) {
                        const long long X1 = (int32_t)m[0], Y1 = (int32_t)m[1], X2 = (int32_t)m[2], Y2 = (int32_t)m[3];      // int(): toward zero
                        ok = X2 >= X1 && Y2 >= Y1;
                        if (ok) {
                            const long long mx = rule.margin_px + ((X2 - X1 + 1) * rule.margin_permille + 500) / 1000;
                            const long long my = rule.margin_px + ((Y2 - Y1 + 1) * rule.margin_permille + 500) / 1000;
                            const long long xa = lmax(X1 - mx, 0), xb = lmin(X2 + mx, w0 - 1);
                            const long long ya = lmax(Y1 - my, 0), yb = lmin(Y2 + my, h0 - 1);
                            const long long sw = xb - xa + 1, sh = yb - ya + 1;
                            ok = sw >= 1 && sh >= 1 && sw >= rule.min_side && sh >= rule.min_side;
                            if (ok) {
                                int rw = rule.cw, rh = rule.ch, left = 0, top = 0;
                                if (rule.fit == CHIP_LETTERBOX) {
                                    const long long p = sh * rule.cw, q = sw * rule.ch;
                                    if (p > q) { rw = (int)((double)sw / (double)sh * (double)rule.ch); left = (rule.cw - rw) / 2; }
                                    else if (p < q) { rh = (int)((double)sh / (double)sw * (double)rule.cw); top = (rule.ch - rh) / 2; }
                                }
                                ok = rw > 0 && rh > 0;
                                d[0] = (int32_t)xa; d[1] = (int32_t)ya; d[2] = (int32_t)sw; d[3] = (int32_t)sh;
                                d[4] = rw; d[5] = rh; d[6] = left; d[7] = top;
                            }
                        }
                    }
                    if (ok) use = true; else ++skipped;
                }
            }
        }
        int n;
        const int rank = evs::ordered_rank(use, wsum, n);
        if (use) {
            int32_t* p = desc + (lo + running + rank) * CHIP_DESC;                       // running + rank <= i - lo: inside the frame's slots
            const uintptr_t src = img + ((size_t)d[1] * (size_t)w0 + (size_t)d[0]) * 3;
            *reinterpret_cast<int4*>(p) = make_int4(d[0], d[1], d[2], d[3]);
            *reinterpret_cast<int4*>(p + 4) = make_int4(d[4], d[5], d[6], d[7]);
            *reinterpret_cast<int4*>(p + 8) = make_int4((int32_t)i, (int32_t)w0, (int32_t)(uint32_t)(src & 0xFFFFFFFFull), (int32_t)(uint32_t)(src >> 32));
        }
        running += n;
    }
    for (int o = 32; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o);
    if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(&stat[1], (unsigned long long)skipped);
    if (threadIdx.x == 0) {
        book[b] = (int32_t)lo;
        book[bcap + b] = running;
    }
}

// One workgroup; thread t owns frames 4t .. 4t + 3.  chip_offsets[b] = min(usable records of the frames before b, max_chips).
__global__ __launch_bounds__(CHIP_THREADS) void chip_scan_kernel(int B, int bcap, const int32_t* __restrict__ offsets, int max_chips,
                                                                 const int32_t* __restrict__ book, int32_t* __restrict__ chip_offsets,
                                                                 unsigned long long* __restrict__ stat)
{
    __shared__ long long lds[CHIP_THREADS / 64];
    const int t = threadIdx.x;
    if (offsets[B] < 0) {                       // (uniform) the range mark: 0, .., 0, -1
        for (int b = t; b <= B; b += CHIP_THREADS) chip_offsets[b] = b == B ? -1 : 0;
        return;
    }
    long long c[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = 4 * t + k;
        c[k] = b < B ? book[bcap + b] : 0;
        sum += c[k];
    }
    const long long incl = evs::block_scan_incl(sum, [](long long a, long long b) { return a + b; }, lds);
    long long at = incl - sum;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = 4 * t + k;
        if (b < B) chip_offsets[b] = (int32_t)lmin(at, max_chips);
        at += c[k];
    }
    if (t == CHIP_THREADS - 1) {                // incl is the total here
        const long long n = lmin(incl, max_chips);
        chip_offsets[B] = (int32_t)n;
        stat[0] = (unsigned long long)n;
        stat[2] = (unsigned long long)(incl - n);
    }
}

struct ChipOut { void* chips; int32_t* index; int32_t* rect; };

__global__ __launch_bounds__(CHIP_THREADS) void chip_resample_kernel(int B, int bcap, ChipRule rule, const int32_t* __restrict__ desc,
                                                                     const int32_t* __restrict__ book, const int32_t* __restrict__ chip_offsets,
                                                                     ChipOut out)
{
    __shared__ int2 col[CHIP_MAX_W];            // per destination column of the resized extent: sx, a0 | a1 << 16
    const int count = chip_offsets[B];          // <= max_chips; negative: the range mark
    const int qpr = rule.cw >> 2;               // four-pixel groups per row
    const int quads = qpr * rule.ch;
    const int tiles = (quads + CHIP_THREADS - 1) / CHIP_THREADS;
    const long long items = (long long)(count > 0 ? count : 0) * tiles;
    const size_t plane = (size_t)rule.cw * rule.ch;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {      // (uniform over the workgroup: the barriers below are met by all)
        const int slot = (int)(item / tiles), tile = (int)(item - (long long)slot * tiles);
        const int b = evs::image_of(chip_offsets, B, slot);                  // the last frame whose base is <= slot: the one that holds it
        const int32_t* dp = desc + ((size_t)book[b] + (size_t)(slot - chip_offsets[b])) * CHIP_DESC;
        const int4 d0 = *reinterpret_cast<const int4*>(dp), d1 = *reinterpret_cast<const int4*>(dp + 4), d2 = *reinterpret_cast<const int4*>(dp + 8);
        PrepArgs a;
        a.img = reinterpret_cast<const unsigned char*>((uintptr_t)(uint32_t)d2.z | (uintptr_t)(uint32_t)d2.w << 32);
        a.w0 = d0.z; a.h0 = d0.w; a.pitch = d2.y; a.rw = d1.x; a.rh = d1.y; a.left = d1.z; a.top = d1.w; a.side = 0; a.out = nullptr;
        a.mode = prep_mode(a.h0, a.w0, a.rw, a.rh);
#pragma unroll
        for (int c = 0; c < 3; ++c) { a.mean[c] = rule.mean[c]; a.std[c] = rule.std[c]; }
        if (tile == 0 && threadIdx.x < 9) {     // the slot's bookkeeping, once
            const int32_t v[9] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w, d2.x};
            if (threadIdx.x < 8) out.rect[(size_t)slot * 8 + threadIdx.x] = v[threadIdx.x];
            else out.index[slot] = v[8];
        }
        if (a.mode == 2) {
            const double scx = 1.0 / ((double)a.rw / (double)a.w0);
            for (int rx = threadIdx.x; rx < a.rw; rx += CHIP_THREADS) {      // prep_sample's column set-up, operation for operation
                float fx = (float)(((double)rx + 0.5) * scx - 0.5);
                int sx = (int)floorf(fx);
                fx -= (float)sx;
                if (sx < 0) { fx = 0.0f; sx = 0; }
                if (sx >= a.w0 - 1) { fx = 0.0f; sx = a.w0 - 1; }
                const int a0 = __float2int_rn((1.0f - fx) * 2048.0f), a1 = __float2int_rn(fx * 2048.0f);
                col[rx] = make_int2(sx, a0 | a1 << 16);
            }
            __syncthreads();
        }
        const int q = tile * CHIP_THREADS + threadIdx.x;
        if (q < quads) {
            const int y = q / qpr, x4 = (q - y * qpr) * 4;
            const int ry = y - a.top;
            const bool row_in = ry >= 0 && ry < a.rh;
            int b0 = 0, b1 = 0;
            const unsigned char* p0 = a.img;
            const unsigned char* p1 = a.img;
            if (row_in && a.mode == 2) {        // prep_sample's row set-up
                const double scy = 1.0 / ((double)a.rh / (double)a.h0);
                float fy = (float)(((double)ry + 0.5) * scy - 0.5);
                const int sy = (int)floorf(fy);
                fy -= (float)sy;
                b0 = __float2int_rn((1.0f - fy) * 2048.0f); b1 = __float2int_rn(fy * 2048.0f);
                const int r0 = min(max(sy, 0), a.h0 - 1), r1 = min(max(sy + 1, 0), a.h0 - 1);
                p0 = a.img + (size_t)r0 * a.pitch * 3;
                p1 = a.img + (size_t)r1 * a.pitch * 3;
            }
            float v[4][3];                      // BGR; f32: before Normalize
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int rx = x4 + k - a.left;
                in[k] = row_in && rx >= 0 && rx < a.rw;
                if (!in[k]) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[k][c] = rule.fill[c];
                } else if (a.mode != 2) {
                    prep_sample(a, ry, rx, v[k]);                            // copy or the 2:1 box: no set-up to share
                } else {
                    const int2 t = col[rx];
                    const int sx = t.x, a0 = t.y & 0xFFFF, a1 = t.y >> 16;
                    const int sx1 = min(sx + 1, a.w0 - 1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int s0 = p0[sx * 3 + c] * a0 + p0[sx1 * 3 + c] * a1;          // HResizeLinear (scale 2048)
                        const int s1 = p1[sx * 3 + c] * a0 + p1[sx1 * 3 + c] * a1;
                        const int r = (((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2;   // VResizeLinear 8u
                        v[k][c] = (float)min(max(r, 0), 255);
                    }
                }
            }
            if (rule.format == CHIP_U8) {
                uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int byte = 3 * k + c;
                        w[byte >> 2] |= (uint32_t)(int)v[k][c] << ((byte & 3) * 8);          // integer-valued in 0..255, the fill included
                    }
                uint32_t* o = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(out.chips) + ((size_t)slot * plane + (size_t)y * rule.cw + x4) * 3);
                o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
            } else {
                float* o = static_cast<float*>(out.chips) + (size_t)slot * 3 * plane + (size_t)y * rule.cw + x4;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    *reinterpret_cast<float4*>(o + (size_t)(2 - c) * plane) =
                        make_float4(prep_normalise(a, c, v[0][c]), prep_normalise(a, c, v[1][c]), prep_normalise(a, c, v[2][c]), prep_normalise(a, c, v[3][c]));
            }
        }
        if (a.mode == 2) __syncthreads();       // the table is rewritten by the next item
    }
}

}  // namespace

struct ChipState {
    int device = 0, max_chips = 0;
    ChipRule rule{};
    DevBuf<unsigned char> keep;                                 // [C]
    DevBuf<int32_t> desc;                                       // [records][CHIP_DESC]: frame b's list starts at its first record's slot
    DevBuf<int32_t> book;                                       // [2][frames()]: start, count per frame
    size_t frames() const { return book.cap() / 2; }
    DevBuf<unsigned long long> stat;                            // chips, skipped, overflow, range mark of the last batch
    int last_B = -1;
};

int chip_device(const ChipState* c) { return c->device; }

void chip_destroy(ChipState* c)
{
    if (!c) return;
    DeviceScope on(c->device);
    delete c;
}

int chip_create(int device, int C, const uint8_t* class_keep, int max_chips, const int32_t* ip, const float* fp, ChipState** out, std::string& err)
{
    static const char* const inames[7] = {"cw", "ch", "fit", "format", "margin_px", "margin_permille", "min_side"};
    static const int ilo[7] = {8, 8, 0, 0, 0, 0, 1}, ihi[7] = {1024, 1024, 1, 1, 4096, 4000, 16384};
    static const char* const fnames[10] = {"min_score", "fill[0]", "fill[1]", "fill[2]", "mean[0]", "mean[1]", "mean[2]", "std[0]", "std[1]", "std[2]"};
    if (C < 1 || C > 2000) { err = "yn_chip_create: num_classes " + std::to_string(C) + " outside 1..2000"; return 1; }
    if (max_chips < 1 || max_chips > 65536) { err = "yn_chip_create: max_chips " + std::to_string(max_chips) + " outside 1..65536"; return 1; }
    for (int i = 0; i < 7; ++i)
        if (ip[i] < ilo[i] || ip[i] > ihi[i]) {
            err = std::string("yn_chip_create: ") + inames[i] + " " + std::to_string(ip[i]) + " outside " + std::to_string(ilo[i]) + ".." + std::to_string(ihi[i]);
            return 1;
        }
    if (ip[0] % 4) { err = "yn_chip_create: cw " + std::to_string(ip[0]) + " is no multiple of 4"; return 1; }
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(fp[i])) { err = std::string("yn_chip_create: ") + fnames[i] + " is not finite"; return 1; }
    for (int i = 7; i < 10; ++i)
        if (!(fp[i] > 0.0f)) { err = std::string("yn_chip_create: ") + fnames[i] + " is not positive"; return 1; }
    if (ip[3] == CHIP_U8)
        for (int i = 1; i < 4; ++i)
            if (fp[i] < 0.0f || fp[i] > 255.0f || fp[i] != truncf(fp[i])) { err = std::string("yn_chip_create: ") + fnames[i] + " is no integer in 0..255 (u8 chips)"; return 1; }
    auto* c = new ChipState;
    c->device = device; c->max_chips = max_chips;
    ChipRule& r = c->rule;
    r.cw = ip[0]; r.ch = ip[1]; r.fit = ip[2]; r.format = ip[3]; r.margin_px = ip[4]; r.margin_permille = ip[5]; r.min_side = ip[6]; r.C = C;
    r.min_score = fp[0];
    for (int i = 0; i < 3; ++i) { r.fill[i] = fp[1 + i]; r.mean[i] = fp[4 + i]; r.std[i] = fp[7 + i]; }
    std::vector<unsigned char> keep(C, 1);
    if (class_keep)
        for (int i = 0; i < C; ++i) keep[i] = class_keep[i] ? 1 : 0;
    int rc = c->keep.reserve((size_t)C);
    if (!rc) rc = c->stat.reserve(4);
    if (!rc) rc = hipMemcpy(c->keep, keep.data(), (size_t)C, hipMemcpyHostToDevice);
    if (!rc) rc = hipMemset(c->stat, 0, 4 * sizeof(unsigned long long));
    if (rc) { err = std::string("yn_chip_create: ") + hipGetErrorString((hipError_t)rc); chip_destroy(c); return 1; }
    *out = c;
    return 0;
}

int chip_batch(ChipState* c, int handle_device, hipStream_t s, int B, const uint8_t* const* frames, const int32_t* geom, int space, const float* rec_dev,
               const int32_t* offsets_dev, int64_t rec_capacity, void* chips_dev, int32_t* index_dev, int32_t* rect_dev, int32_t* chip_offsets_dev,
               std::string& err)
{
    if (B < 0 || B > CHIP_MAX_B) { err = "yn_chip_batch: B " + std::to_string(B) + " outside 0..1024"; return 1; }
    if (rec_capacity < 0 || rec_capacity > ((int64_t)1 << 31) - 1) { err = "yn_chip_batch: rec_capacity outside 0..2^31 - 1"; return 1; }
    if ((uintptr_t)chips_dev & 15) { err = "yn_chip_batch: chips_dev is not 16-byte aligned"; return 1; }
    if (!chip_offsets_dev) { err = "yn_chip_batch: null pointer chip_offsets_dev"; return 1; }
    if (B > 0) {
        if (!frames) { err = "yn_chip_batch: null pointer frames_host"; return 1; }
        if (!geom) { err = "yn_chip_batch: null pointer geom_host"; return 1; }
        if (!rec_dev && rec_capacity > 0) { err = "yn_chip_batch: null pointer rec_dev"; return 1; }
        if (!offsets_dev) { err = "yn_chip_batch: null pointer offsets_dev"; return 1; }
        if (!chips_dev) { err = "yn_chip_batch: null pointer chips_dev"; return 1; }
        if (!index_dev) { err = "yn_chip_batch: null pointer index_dev"; return 1; }
        if (!rect_dev) { err = "yn_chip_batch: null pointer rect_dev"; return 1; }
        for (int b = 0; b < B; ++b)
            if (!frames[b]) { err = "yn_chip_batch: null frame pointer for frame " + std::to_string(b); return 1; }
        for (int b = 0; b < B; ++b) {
            const int32_t* g = geom + (size_t)b * 7;
            if (g[0] < 1 || g[1] < 1 || g[0] > 16384 || g[1] > 16384) {
                err = "yn_chip_batch: frame " + std::to_string(b) + " is " + std::to_string(g[0]) + "x" + std::to_string(g[1]) + ", sides must be 1..16384";
                return 1;
            }
            if (space == 0 && (g[2] < 1 || g[3] < 1 || g[4] < 0 || g[5] < 0 || g[6] < 1 || g[4] + g[2] > g[6] || g[5] + g[3] > g[6])) {
                err = "yn_chip_batch: bad letterbox geometry for frame " + std::to_string(b);
                return 1;
            }
        }
    }
    if (space != 0 && space != 1) {
        err = "yn_chip_batch: space " + std::to_string(space) + " is neither YN_DRAW_LETTERBOX nor YN_DRAW_PIXELS";
        return 1;
    }
    if (c->device != handle_device) {
        err = "yn_chip_batch: the object was made for device " + std::to_string(c->device) + ", the handle is on device " + std::to_string(handle_device);
        return 1;
    }
    c->last_B = -1;
    EVCHK(hipMemsetAsync(c->stat, 0, 4 * sizeof(unsigned long long), s));
    if (B == 0) {                                               // an empty batch is not an error: chip_offsets[0] = 0 and nothing else
        EVCHK(hipMemsetAsync(chip_offsets_dev, 0, sizeof(int32_t), s));
        c->last_B = 0;
        return 0;
    }
    EVCHK(c->desc.reserve((size_t)std::max<int64_t>(rec_capacity, 1) * CHIP_DESC, 1));
    if ((size_t)B > c->frames()) {                              // [2][frames]: both halves move, so start over from one element
        c->book.reset();
        EVCHK(c->book.reserve(2 * (size_t)std::max(B, CHIP_FRAMES), 1));
    }
    const int bcap = (int)c->frames();
    for (int b0 = 0; b0 < B; b0 += CHIP_FRAMES) {
        ChipFrames fr{};
        const int m = std::min(CHIP_FRAMES, B - b0);
        for (int i = 0; i < m; ++i) {
            fr.p[i] = frames[b0 + i];
            for (int k = 0; k < 7; ++k) fr.g[i][k] = geom[(size_t)(b0 + i) * 7 + k];
        }
        hipLaunchKernelGGL(chip_select_kernel, dim3(m), dim3(CHIP_THREADS), 0, s, fr, b0, B, bcap, rec_dev, offsets_dev, (long long)rec_capacity, space,
                           c->rule, c->keep, c->desc, c->book, c->stat);
    }
    hipLaunchKernelGGL(chip_scan_kernel, dim3(1), dim3(CHIP_THREADS), 0, s, B, bcap, offsets_dev, c->max_chips, c->book, chip_offsets_dev, c->stat);
    const int tiles = ((c->rule.cw >> 2) * c->rule.ch + CHIP_THREADS - 1) / CHIP_THREADS;
    const long long cap_items = (long long)c->max_chips * tiles;
    hipLaunchKernelGGL(chip_resample_kernel, dim3((unsigned)std::min<long long>(cap_items, CHIP_GRID)), dim3(CHIP_THREADS), 0, s, B, bcap, c->rule, c->desc,
                       c->book, chip_offsets_dev, ChipOut{chips_dev, index_dev, rect_dev});
    EVCHK(hipGetLastError());
    c->last_B = B;
    return 0;
}

int chip_status(ChipState* c, hipStream_t s, int64_t* counters, std::string& err)
{
    if (c->last_B < 0) { err = "yn_chip_status: no yn_chip_batch has run"; return 1; }
    unsigned long long st[4] = {0, 0, 0, 0};
    EVCHK(hipMemcpyAsync(st, c->stat, sizeof(st), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    for (int i = 0; i < 3; ++i) counters[i] = (int64_t)st[i];
    counters[3] = st[3] ? 1 : 0;
    return 0;
}

}  // namespace ynk
