// kernels_draw.hip — detections painted onto uint8 BGR frames in list order (test.py:50-92 visualize / plot_bbox_labels, demo.py:48-71):
// the state behind yn_draw.  DESIGN.md §23 is the specification; tests/draw_oracle.py restates it one pixel at a time.
//
//   draw_prims_kernel   one workgroup per frame walks the frame's records in list order, 256 at a time: un-letterbox (or take pixels),
//                       int() of every coordinate, the filter (score > vis_thresh, class, finite |v| < 2^30, '%.2f' digits k in 0..100)
//                       and an order-preserving compaction (ballot + prefix popcount, a running base; no atomics decide a position)
//                       into the frame's primitive list prims[start .. start + count)
//   draw_tile_kernel    one workgroup per 64 x 16 tile of one frame: 256 primitives at a time it keeps, in order, those whose PAINTED
//                       area (the four edge strips of the outline and the title bar, not the bounding box) meets the tile, then every
//                       thread applies that short list in sequence to its four pixels (one column, four rows) held in registers
//
// No pixel is ever read: a later primitive overwrites an earlier one, and the only blend (the glyph coverage) is over the title bar
// the same primitive has just painted, so the destination colour is known.  A pixel no primitive touches is not written either.
// Stores are byte-granular, three per touched pixel: a row is w0 * 3 bytes at any alignment, so a dword that straddles a tile edge
// belongs to two workgroups and a read-modify-write of it would race.  Integer arithmetic only past unletterbox().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "yn_eval_shared.h"
#include "yn_internal.h"

namespace ynk {

namespace {

constexpr int DRAW_THREADS = 256;                // evs::ordered_rank's workgroup
constexpr int DRAW_TW = 64, DRAW_TH = 16;       // tile: one lane per column, each wave four rows
constexpr int DRAW_ROWS = DRAW_TH / (DRAW_THREADS / 64);
constexpr int DRAW_FRAMES = 32;                 // frames per launch (descriptors travel in the kernel arguments)
constexpr int DRAW_LABEL = 32;                  // longest label
constexpr int DRAW_PRIM = 8;                    // int32 words per primitive: x1, y1, x2, y2, class, k, frame, pad

struct DrawFrames {
    unsigned char* p[DRAW_FRAMES];
    int32_t g[DRAW_FRAMES][7];                  // w0, h0, rw, rh, left, top, side
    int32_t tile0[DRAW_FRAMES + 1];             // first tile of frame i among the launch's workgroups
    int32_t m;                                  // frames in this launch
};

struct DrawStyle {
    const uint32_t* colors;                     // [C] b | g << 8 | r << 16
    const unsigned char* labels;                // [C][DRAW_LABEL], null: outlines only
    const int32_t* lens;                        // [C] strlen(label)
    const unsigned char* atlas;                 // [95][gh][gw]
    int32_t gw, gh, thickness, C;
};

// stat: [0] drawn, [1] skipped, [2] range mark.  book [2][bcap]: start and count of every frame's primitive list.
__global__ __launch_bounds__(DRAW_THREADS) void draw_prims_kernel(DrawFrames fr, int frame0, int B, int bcap, const float* __restrict__ rec,
                                                                  const int32_t* __restrict__ offsets, long long rec_capacity, float vis_thresh,
                                                                  int space, int C, int32_t* __restrict__ prims, int32_t* __restrict__ book,
                                                                  unsigned long long* __restrict__ stat)
{
    __shared__ int wsum[DRAW_THREADS / 64];
    const int f = blockIdx.x, b = frame0 + f;
    const int total_all = offsets[B];
    if (total_all < 0) {                        // the split-f16 range mark: the records are not valid, nothing is drawn
        if (threadIdx.x == 0) { book[b] = 0; book[bcap + b] = 0; atomicOr(&stat[2], 1ull); }
        return;
    }
    long long lo = offsets[b], hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > rec_capacity ? rec_capacity : lo);      // never a read past the record buffer, whatever the offsets hold
    hi = hi < lo ? lo : (hi > rec_capacity ? rec_capacity : hi);
    int32_t g[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) g[i] = fr.g[f][i];
    int running = 0, skipped = 0;
    for (long long base = lo; base < hi; base += DRAW_THREADS) {
        const long long i = base + threadIdx.x;
        bool draw = false;
        int32_t v[4] = {0, 0, 0, 0};
        int cls = 0, k = 0;
        if (i < hi) {
            float r[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) r[c] = rec[i * 6 + c];
            if (r[4] > vis_thresh) {            // strict, so a NaN score is not drawn (and not counted)
                float m[4];
                if (space == 0) evs::unletterbox(r, g, m);
                else { m[0] = r[0]; m[1] = r[1]; m[2] = r[2]; m[3] = r[3]; }
                bool ok = r[5] >= 0.0f && r[5] < (float)C && r[5] == truncf(r[5]);
#pragma unroll
                for (int c = 0; c < 4; ++c) ok = ok && fabsf(m[c]) < 1073741824.0f;      // false for NaN and the infinities
                const double kd = rint((double)r[4] * 100.0);                           // the product is exact: '%.2f' of the score
                ok = ok && kd >= 0.0 && kd <= 100.0;
                if (ok) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = (int32_t)m[c];                   // int(): toward zero
                    cls = (int)r[5];
                    k = (int)kd;
                    draw = true;
                } else {
                    ++skipped;
                }
            }
        }
        int n;
        const int rank = evs::ordered_rank(draw, wsum, n);
        if (draw) {
            int32_t* p = prims + (lo + running + rank) * DRAW_PRIM;                      // running + rank <= i - lo: inside the frame's slots
            *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<int4*>(p + 4) = make_int4(cls, k, b, 0);
        }
        running += n;
    }
    for (int o = 32; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o);
    if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(&stat[1], (unsigned long long)skipped);
    if (threadIdx.x == 0) {
        book[b] = (int32_t)lo;
        book[bcap + b] = running;
        if (running) atomicAdd(&stat[0], (unsigned long long)running);
    }
}

__device__ __forceinline__ bool rects_meet(int ax0, int ay0, int ax1, int ay1, int bx0, int by0, int bx1, int by1)
{
    return ax0 <= bx1 && bx0 <= ax1 && ay0 <= by1 && by0 <= ay1;      // an empty rectangle a (x0 > x1, an inverted box) can pass: conservative only,
                                                                      // the per-pixel test then paints nothing
}

struct Shape {                                  // what one primitive paints, from its six numbers
    int ox0, oy0, ox1, oy1;                     // outline: outer rectangle
    int hx0, hy0, hx1, hy1;                     // its hole (hole == false: none, the rectangle is filled)
    int bx0, by0, bx1, by1;                     // title bar (bar == false: none)
    bool hole, bar;
};

__device__ __forceinline__ Shape shape_of(const int4 q, int len, const DrawStyle& st)
{
    const int a = st.thickness >> 1, c = (st.thickness - 1) >> 1;
    Shape s;
    s.ox0 = q.x - a; s.oy0 = q.y - a; s.ox1 = q.z + a; s.oy1 = q.w + a;
    s.hx0 = q.x + c + 1; s.hy0 = q.y + c + 1; s.hx1 = q.z - c - 1; s.hy1 = q.w - c - 1;
    s.hole = s.hx0 <= s.hx1 && s.hy0 <= s.hy1;
    s.bar = st.labels != nullptr;
    s.bx0 = q.x; s.bx1 = q.x + (len + 6) * st.gw + 1; s.by0 = q.y - st.gh - 1; s.by1 = q.y;
    return s;
}

__global__ __launch_bounds__(DRAW_THREADS) void draw_tile_kernel(DrawFrames fr, int frame0, int bcap, const int32_t* __restrict__ prims,
                                                                 const int32_t* __restrict__ book, DrawStyle st)
{
    __shared__ int wsum[DRAW_THREADS / 64];
    __shared__ int4 list[DRAW_THREADS][2];
    int f = 0;
    while (f + 1 < fr.m && (int)blockIdx.x >= fr.tile0[f + 1]) ++f;                      // uniform: at most 31 steps
    const int w0 = fr.g[f][0], h0 = fr.g[f][1];
    const int tiles_x = (w0 + DRAW_TW - 1) / DRAW_TW;
    const int t = (int)blockIdx.x - fr.tile0[f];
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int tx0 = tx * DRAW_TW, ty0 = ty * DRAW_TH;
    const int tx1 = min(tx0 + DRAW_TW, w0) - 1, ty1 = min(ty0 + DRAW_TH, h0) - 1;
    const int start = book[frame0 + f], count = book[bcap + frame0 + f];
    const int x = tx0 + (threadIdx.x & 63);
    const int yb = ty0 + (threadIdx.x >> 6) * DRAW_ROWS;
    uint32_t col[DRAW_ROWS];
    unsigned touched = 0;
    for (int c0 = 0; c0 < count; c0 += DRAW_THREADS) {          // a list longer than the LDS holds: chunk after chunk, still in order
        const int idx = c0 + threadIdx.x;
        int4 q = make_int4(0, 0, 0, 0), e = make_int4(0, 0, 0, 0);
        bool meets = false;
        if (idx < count) {
            const int32_t* p = prims + ((size_t)start + idx) * DRAW_PRIM;
            q = *reinterpret_cast<const int4*>(p);
            e = *reinterpret_cast<const int4*>(p + 4);
            const Shape s = shape_of(q, st.labels ? st.lens[e.x] : 0, st);
            if (!s.hole) {
                meets = rects_meet(s.ox0, s.oy0, s.ox1, s.oy1, tx0, ty0, tx1, ty1);
            } else {                                            // top, bottom, left, right strip
                meets = rects_meet(s.ox0, s.oy0, s.ox1, s.hy0 - 1, tx0, ty0, tx1, ty1) || rects_meet(s.ox0, s.hy1 + 1, s.ox1, s.oy1, tx0, ty0, tx1, ty1) ||
                        rects_meet(s.ox0, s.oy0, s.hx0 - 1, s.oy1, tx0, ty0, tx1, ty1) || rects_meet(s.hx1 + 1, s.oy0, s.ox1, s.oy1, tx0, ty0, tx1, ty1);
            }
            if (s.bar) meets = meets || rects_meet(s.bx0, s.by0, s.bx1, s.by1, tx0, ty0, tx1, ty1);
        }
        int n;
        const int rank = evs::ordered_rank(meets, wsum, n);
        if (meets) { list[rank][0] = q; list[rank][1] = e; }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const int4 pq = list[j][0], pe = list[j][1];
            const int cls = pe.x, k = pe.y;
            const int len = st.labels ? st.lens[cls] : 0;
            const Shape s = shape_of(pq, len, st);
            const uint32_t color = st.colors[cls];
            const bool in_ox = x >= s.ox0 && x <= s.ox1;
            const bool in_hx = s.hole && x >= s.hx0 && x <= s.hx1;
            const bool in_bx = s.bar && x >= s.bx0 && x <= s.bx1;
            if (!in_ox && !in_bx) continue;
            // the glyph column of this pixel column (the text lies inside the bar: columns x1 + 1 .. x1 + L * gw, rows y1 - gh .. y1 - 1)
            int ch = -1, gcol = 0;
            if (in_bx) {
                const int u = x - pq.x - 1;
                if (u >= 0 && u < (len + 6) * st.gw) {
                    const int gj = u / st.gw;
                    gcol = u - gj * st.gw;
                    if (gj < len) ch = st.labels[cls * DRAW_LABEL + gj];
                    else {
                        const int d = gj - len;                 // ": D.DD"
                        ch = d == 0 ? ':' : d == 1 ? ' ' : d == 2 ? '0' + k / 100 : d == 3 ? '.' : d == 4 ? '0' + (k / 10) % 10 : '0' + k % 10;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < DRAW_ROWS; ++i) {
                const int y = yb + i;
                if (in_ox && y >= s.oy0 && y <= s.oy1 && !(in_hx && y >= s.hy0 && y <= s.hy1)) { col[i] = color; touched |= 1u << i; }
                if (in_bx && y >= s.by0 && y <= s.by1) {
                    uint32_t cc = color;
                    const int r = y - (pq.y - st.gh);
                    if (ch >= 0 && r >= 0 && r < st.gh) {
                        const uint32_t a8 = st.atlas[((size_t)(ch - 32) * st.gh + r) * st.gw + gcol];
                        const uint32_t ia = 255u - a8;          // text colour (0, 0, 0): out = (dst * (255 - a8) + 0 * a8 + 127) / 255
                        cc = ((cc & 255u) * ia + 127u) / 255u | (((cc >> 8) & 255u) * ia + 127u) / 255u << 8 | (((cc >> 16) & 255u) * ia + 127u) / 255u << 16;
                    }
                    col[i] = cc;
                    touched |= 1u << i;
                }
            }
        }
        __syncthreads();                                        // the list is rewritten by the next chunk
    }
    if (!touched || x > tx1) return;
    unsigned char* img = fr.p[f];
#pragma unroll
    for (int i = 0; i < DRAW_ROWS; ++i) {
        const int y = yb + i;
        if ((touched >> i & 1u) && y <= ty1) {
            unsigned char* o = img + ((size_t)y * w0 + x) * 3;
            o[0] = (unsigned char)(col[i] & 255u); o[1] = (unsigned char)(col[i] >> 8 & 255u); o[2] = (unsigned char)(col[i] >> 16 & 255u);
        }
    }
}

}  // namespace

struct DrawState {
    int device = 0, C = 0, thickness = 2, gw = 0, gh = 0;
    bool labelled = false;
    DevBuf<uint32_t> colors;
    DevBuf<unsigned char> labels, atlas;
    DevBuf<int32_t> lens;
    DevBuf<int32_t> prims;                                      // [records][DRAW_PRIM]: frame b's list starts at its first record's slot
    DevBuf<int32_t> book;                                       // [2][frames()]: start, count per frame
    size_t frames() const { return book.cap() / 2; }
    DevBuf<unsigned long long> stat;                            // drawn, skipped, range mark of the last batch
    int last_B = -1;
};

int draw_device(const DrawState* d) { return d->device; }

void draw_destroy(DrawState* d)
{
    if (!d) return;
    DeviceScope on(d->device);
    delete d;
}

int draw_create(int device, int C, const uint8_t* colors, const char* const* labels, const uint8_t* atlas, int gw, int gh, int thickness,
                DrawState** out, std::string& err)
{
    if (!colors) { err = "yn_draw_create: null colours"; return 1; }
    if (C < 1 || C > 2000) { err = "yn_draw_create: num_classes " + std::to_string(C) + " outside 1..2000"; return 1; }
    if (thickness < 1 || thickness > 8) { err = "yn_draw_create: thickness " + std::to_string(thickness) + " outside 1..8"; return 1; }
    if ((labels != nullptr) != (atlas != nullptr)) { err = "yn_draw_create: labels and a font atlas come together (both or neither)"; return 1; }
    std::vector<unsigned char> lab;
    std::vector<int32_t> lens;
    if (labels) {
        if (gw < 4 || gw > 32 || gh < 4 || gh > 32) { err = "yn_draw_create: glyph cell " + std::to_string(gw) + "x" + std::to_string(gh) + " outside 4..32"; return 1; }
        lab.assign((size_t)C * DRAW_LABEL, 0);
        lens.assign(C, 0);
        for (int c = 0; c < C; ++c) {
            if (!labels[c]) { err = "yn_draw_create: null label for class " + std::to_string(c); return 1; }
            const size_t n = strnlen(labels[c], DRAW_LABEL + 1);
            if (n > (size_t)DRAW_LABEL) { err = "yn_draw_create: the label of class " + std::to_string(c) + " is longer than 32 characters"; return 1; }
            for (size_t i = 0; i < n; ++i) {
                const unsigned char ch = (unsigned char)labels[c][i];
                if (ch < 32 || ch > 126) { err = "yn_draw_create: the label of class " + std::to_string(c) + " has a byte outside 32..126 at position " + std::to_string(i); return 1; }
                lab[(size_t)c * DRAW_LABEL + i] = ch;
            }
            lens[c] = (int32_t)n;
        }
    }
    std::vector<uint32_t> packed(C);
    for (int c = 0; c < C; ++c) packed[c] = (uint32_t)colors[3 * c] | (uint32_t)colors[3 * c + 1] << 8 | (uint32_t)colors[3 * c + 2] << 16;
    auto* d = new DrawState;
    d->device = device; d->C = C; d->thickness = thickness; d->labelled = labels != nullptr;
    d->gw = labels ? gw : 0; d->gh = labels ? gh : 0;
    const size_t an = (size_t)95 * gh * gw;
    int r = d->colors.reserve((size_t)C);
    if (!r) r = d->stat.reserve(3);
    if (!r && labels) r = d->labels.reserve(lab.size());
    if (!r && labels) r = d->lens.reserve((size_t)C);
    if (!r && labels) r = d->atlas.reserve(an);
    if (!r) r = hipMemcpy(d->colors, packed.data(), (size_t)C * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (!r) r = hipMemset(d->stat, 0, 3 * sizeof(unsigned long long));
    if (labels) {
        if (!r) r = hipMemcpy(d->labels, lab.data(), lab.size(), hipMemcpyHostToDevice);
        if (!r) r = hipMemcpy(d->lens, lens.data(), (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice);
        if (!r) r = hipMemcpy(d->atlas, atlas, an, hipMemcpyHostToDevice);
    }
    if (r) { err = std::string("yn_draw_create: ") + hipGetErrorString((hipError_t)r); draw_destroy(d); return 1; }
    *out = d;
    return 0;
}

int draw_batch(DrawState* d, hipStream_t s, int B, uint8_t* const* frames, const int32_t* geom, int space, const float* rec_dev,
               const int32_t* offsets_dev, int64_t rec_capacity, float vis_thresh, std::string& err)
{
    if (B < 0) { err = "yn_draw_batch: negative batch"; return 1; }
    if (space != 0 && space != 1) { err = "yn_draw_batch: space " + std::to_string(space) + " is neither YN_DRAW_LETTERBOX nor YN_DRAW_PIXELS"; return 1; }
    if (rec_capacity < 0 || rec_capacity > ((int64_t)1 << 31) - 1) { err = "yn_draw_batch: rec_capacity outside 0..2^31 - 1"; return 1; }
    d->last_B = -1;
    if (B == 0) {                                               // an empty batch is not an error: its status is all zeros
        EVCHK(hipMemsetAsync(d->stat, 0, 3 * sizeof(unsigned long long), s));
        d->last_B = 0;
        return 0;
    }
    if (!frames || !geom || !rec_dev || !offsets_dev) { err = "yn_draw_batch: null pointer"; return 1; }
    std::vector<std::pair<uintptr_t, int>> spans(B);
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + (size_t)b * 7;
        if (!frames[b]) { err = "yn_draw_batch: null frame pointer for frame " + std::to_string(b); return 1; }
        if (g[0] < 1 || g[1] < 1 || g[0] > 16384 || g[1] > 16384) {
            err = "yn_draw_batch: frame " + std::to_string(b) + " is " + std::to_string(g[0]) + "x" + std::to_string(g[1]) + ", sides must be 1..16384";
            return 1;
        }
        if (space == 0 && (g[2] < 1 || g[3] < 1 || g[4] < 0 || g[5] < 0 || g[6] < 1 || g[4] + g[2] > g[6] || g[5] + g[3] > g[6])) {
            err = "yn_draw_batch: bad letterbox geometry for frame " + std::to_string(b);
            return 1;
        }
        spans[b] = {(uintptr_t)frames[b], b};
    }
    std::sort(spans.begin(), spans.end());
    for (int i = 1; i < B; ++i) {
        const int p = spans[i - 1].second, q = spans[i].second;
        const int32_t* g = geom + (size_t)p * 7;
        if (spans[i].first == spans[i - 1].first) {
            err = "yn_draw_batch: frames " + std::to_string(std::min(p, q)) + " and " + std::to_string(std::max(p, q)) + " are the same buffer";
            return 1;
        }
        if (spans[i].first < spans[i - 1].first + (uintptr_t)g[0] * g[1] * 3) {
            err = "yn_draw_batch: frames " + std::to_string(std::min(p, q)) + " and " + std::to_string(std::max(p, q)) + " overlap";
            return 1;
        }
    }
    EVCHK(d->prims.reserve((size_t)std::max<int64_t>(rec_capacity, 1) * DRAW_PRIM, 1));
    if ((size_t)B > d->frames()) {                              // [2][frames]: both halves move, so start over from one element
        d->book.reset();
        EVCHK(d->book.reserve(2 * (size_t)std::max(B, DRAW_FRAMES), 1));
    }
    EVCHK(hipMemsetAsync(d->stat, 0, 3 * sizeof(unsigned long long), s));
    DrawStyle st{d->colors, d->labels, d->lens, d->atlas, d->gw, d->gh, d->thickness, d->C};
    for (int b0 = 0; b0 < B; b0 += DRAW_FRAMES) {
        DrawFrames fr{};
        fr.m = std::min(DRAW_FRAMES, B - b0);
        int tiles = 0;
        for (int i = 0; i < fr.m; ++i) {
            const int32_t* g = geom + (size_t)(b0 + i) * 7;
            fr.p[i] = frames[b0 + i];
            for (int k = 0; k < 7; ++k) fr.g[i][k] = g[k];
            fr.tile0[i] = tiles;
            tiles += ((g[0] + DRAW_TW - 1) / DRAW_TW) * ((g[1] + DRAW_TH - 1) / DRAW_TH);      // at most 32 * 256 * 1024 = 2^23
        }
        for (int i = fr.m; i <= DRAW_FRAMES; ++i) fr.tile0[i] = tiles;
        hipLaunchKernelGGL(draw_prims_kernel, dim3(fr.m), dim3(DRAW_THREADS), 0, s, fr, b0, B, (int)d->frames(), rec_dev, offsets_dev,
                           (long long)rec_capacity, vis_thresh, space, d->C, d->prims, d->book, d->stat);
        hipLaunchKernelGGL(draw_tile_kernel, dim3(tiles), dim3(DRAW_THREADS), 0, s, fr, b0, (int)d->frames(), d->prims, d->book, st);
    }
    EVCHK(hipGetLastError());
    d->last_B = B;
    return 0;
}

int draw_status(DrawState* d, hipStream_t s, int64_t* drawn, int64_t* skipped, int* range_mark, std::string& err)
{
    if (d->last_B < 0) { err = "yn_draw_status: no yn_draw_batch has run"; return 1; }
    unsigned long long st[3] = {0, 0, 0};
    EVCHK(hipMemcpyAsync(st, d->stat, sizeof(st), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    if (drawn) *drawn = (int64_t)st[0];
    if (skipped) *skipped = (int64_t)st[1];
    if (range_mark) *range_mark = st[2] ? 1 : 0;
    return 0;
}

int draw_prims(DrawState* d, hipStream_t s, int32_t* host, int64_t cap, std::string& err)
{
    if (d->last_B < 0) { err = "yn_draw_prims: no yn_draw_batch has run"; return 1; }
    const int B = d->last_B;
    if (B == 0) return 0;
    std::vector<int32_t> book(2 * d->frames());
    EVCHK(hipMemcpyAsync(book.data(), d->book, book.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    int64_t n = 0;
    for (int b = 0; b < B; ++b) n += book[d->frames() + b];
    if (n > cap) { err = "yn_draw_prims: " + std::to_string(n) + " primitives, room for " + std::to_string(cap); return 1; }
    std::vector<int32_t> tmp;
    int64_t at = 0;
    for (int b = 0; b < B; ++b) {
        const int cnt = book[d->frames() + b];
        if (!cnt) continue;
        tmp.resize((size_t)cnt * DRAW_PRIM);
        EVCHK(hipMemcpyAsync(tmp.data(), d->prims + (size_t)book[b] * DRAW_PRIM, tmp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        EVCHK(hipStreamSynchronize(s));
        for (int i = 0; i < cnt; ++i, ++at) {
            const int32_t* p = tmp.data() + (size_t)i * DRAW_PRIM;
            int32_t* o = host + at * 7;
            o[0] = p[6]; o[1] = p[4]; o[2] = p[0]; o[3] = p[1]; o[4] = p[2]; o[5] = p[3]; o[6] = p[5];
        }
    }
    return 0;
}

}  // namespace ynk
