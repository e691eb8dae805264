// kernels_jpeg.hip — the device half of the baseline JPEG decode and the state behind yn_jpeg.
//
// The host (yn_jpeg_host.h) parses the markers and undoes the Huffman coding; what it uploads is int16 coefficients, 64 per block in natural
// order.  Two kernels finish a whole batch of images of different sizes and samplings, driven by one descriptor per image:
//   jpeg_idct_kernel    dequantise + libjpeg's jidctint 8x8 (integer, column pass then row pass) -> uint8 component planes padded to whole blocks
//   jpeg_color_kernel   libjpeg's "fancy" (triangle) chroma upsampling for 2x1 / 2x2 + YCbCr -> BGR, written as uint8 [h][w][3] frames
// Every step is the integer arithmetic of libjpeg's default decode (JDCT_ISLOW, do_fancy_upsampling), so the frames equal cv2.imread's and
// PIL's byte for byte (tests/jpeg_oracle.py restates the rules).  Nothing is addressed by data: garbage coefficients give garbage pixels, no fault.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "yn_internal.h"
#include "yn_jpeg_host.h"

namespace ynk {

namespace {

struct alignas(16) JpegDesc {
    uint16_t qt[3][64];            // natural order, per component
    uint8_t* frame;                // uint8 [h][w][3] BGR
    int64_t coef_off[3];           // int16 elements into the coefficient buffer
    int64_t plane_off[3];          // bytes into the plane buffer (multiples of 64)
    int32_t w, h, nc, hs, vs;      // hs x vs: luma sampling = how far the chroma planes are subsampled
    int32_t bw[3], bh[3];          // block grid per component (MCU-padded): a plane is [bh * 8][bw * 8]
    int32_t dw[3], dh[3];          // the samples of a plane that belong to the image: ceil(w * h_i / h_max), ceil(h * v_i / v_max)
    int32_t group0[3];             // first 8-block group of the component in the chunk's numbering
    int32_t wide;                  // frame rows start on 4-byte boundaries: 12-byte stores
};

__device__ __forceinline__ int find_image(const int32_t* start, int n, int v)      // the largest i < n with start[i] <= v
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// jidctint's 1-D pass (constants round(x * 2^13)), in unsigned arithmetic: wrap-around instead of undefined behaviour on garbage
template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int32_t (&x)[8], int32_t (&o)[8])
{
    typedef uint32_t u;
    const u x0 = (u)x[0], x1 = (u)x[1], x2 = (u)x[2], x3 = (u)x[3], x4 = (u)x[4], x5 = (u)x[5], x6 = (u)x[6], x7 = (u)x[7];
    u z1 = (x2 + x6) * 4433u;
    const u t2 = z1 - x6 * 15137u, t3 = z1 + x2 * 6270u;
    const u t0 = (x0 + x4) << 13, t1 = (x0 - x4) << 13;
    const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u a0 = x7, a1 = x5, a2 = x3, a3 = x1;
    z1 = a0 + a3;
    u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u z5 = (z3 + z4) * 9633u;
    a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
    z1 *= (u)-7373; z2 *= (u)-20995;
    z3 = z3 * (u)-16069 + z5; z4 = z4 * (u)-3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const u r = 1u << (SHIFT - 1);
    o[0] = (int32_t)(t10 + a3 + r) >> SHIFT; o[7] = (int32_t)(t10 - a3 + r) >> SHIFT;
    o[1] = (int32_t)(t11 + a2 + r) >> SHIFT; o[6] = (int32_t)(t11 - a2 + r) >> SHIFT;
    o[2] = (int32_t)(t12 + a1 + r) >> SHIFT; o[5] = (int32_t)(t12 - a1 + r) >> SHIFT;
    o[3] = (int32_t)(t13 + a0 + r) >> SHIFT; o[4] = (int32_t)(t13 - a0 + r) >> SHIFT;
}

constexpr int IDCT_LD = 9;          // LDS row stride of a block in words: 8 + 1 against bank conflicts of the transposed accesses

// A wavefront takes 8 blocks: lane = (block, j).  The lane loads row j (16 bytes) and dequantises it, owns COLUMN j in the first pass and
// ROW j in the second (the transposes go through LDS), and stores row j of the block into its component plane (8 bytes).
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegDesc* __restrict__ desc, const int32_t* __restrict__ group_start, int n,
                                                        const int16_t* __restrict__ coef, uint8_t* __restrict__ planes)
{
    __shared__ int32_t ws[4][8][8 * IDCT_LD];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = lane >> 3, j = lane & 7;
    const int g = blockIdx.x * 4 + wave;
    bool live = g < group_start[n];
    int img = 0, c = 0, blk = 0;
    if (live) {
        img = find_image(group_start, n, g);
        if (desc[img].nc == 3) c = g >= desc[img].group0[2] ? 2 : g >= desc[img].group0[1] ? 1 : 0;
        blk = (g - desc[img].group0[c]) * 8 + b;
        live = blk < desc[img].bw[c] * desc[img].bh[c];
    }
    const JpegDesc& D = desc[img];
    int32_t* w = ws[wave][b];
    if (live) {
        const int4 raw = *reinterpret_cast<const int4*>(coef + D.coef_off[c] + (int64_t)blk * 64 + j * 8);
        const int4 q = *reinterpret_cast<const int4*>(&D.qt[c][j * 8]);
        const int rv[4] = {raw.x, raw.y, raw.z, raw.w}, qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[j * IDCT_LD + 2 * k] = (int32_t)((uint32_t)(int32_t)(int16_t)(rv[k] & 0xffff) * ((uint32_t)qv[k] & 0xffffu));
            w[j * IDCT_LD + 2 * k + 1] = (int32_t)((uint32_t)(rv[k] >> 16) * ((uint32_t)qv[k] >> 16));
        }
    }
    __syncthreads();
    int32_t x[8], o[8];
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = w[r * IDCT_LD + j];
        idct_1d<11>(x, o);                                   // columns: CONST_BITS - PASS1_BITS
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r * IDCT_LD + j] = o[r];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = w[j * IDCT_LD + k];
        idct_1d<18>(x, o);                                   // rows: CONST_BITS + PASS1_BITS + 3
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)min(max(o[k] + 128, 0), 255) << (8 * k);
            hi |= (uint32_t)min(max(o[k + 4] + 128, 0), 255) << (8 * k);
        }
        const int bw = D.bw[c], by = blk / bw, bx = blk - by * bw;
        *reinterpret_cast<uint2*>(planes + D.plane_off[c] + ((int64_t)by * 8 + j) * ((int64_t)bw * 8) + bx * 8) = make_uint2(lo, hi);
    }
}

// four samples x0 .. x0 + 3 (x0 a multiple of 4) of output row y of one chroma plane, upsampled as libjpeg does; only samples of the
// plane's real extent dw x dh are read
__device__ __forceinline__ void chroma4(const JpegDesc& D, const uint8_t* __restrict__ planes, int k, int y, int x0, int (&v)[4])
{
    const int pw = D.bw[k] * 8, dw = D.dw[k], dh = D.dh[k];
    const uint8_t* pl = planes + D.plane_off[k];
    if (D.hs == 1) {                                         // 4:4:4
        const uint32_t four = *reinterpret_cast<const uint32_t*>(pl + (int64_t)y * pw + x0);
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = (four >> (8 * t)) & 255;
        return;
    }
    const int r = D.vs == 2 ? y >> 1 : y;
    const uint8_t* row = pl + (int64_t)r * pw;
    const int c0 = x0 >> 1;
    if (dw <= 2) {                                           // libjpeg drops to replication for such narrow planes
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = row[min(c0 + (t >> 1), dw - 1)];
        return;
    }
    const int col[4] = {max(c0 - 1, 0), c0, min(c0 + 1, dw - 1), min(c0 + 2, dw - 1)};
    int s[4];
    if (D.vs == 2) {
        const int nr = (y & 1) ? min(r + 1, dh - 1) : max(r - 1, 0);
        const uint8_t* near = pl + (int64_t)nr * pw;
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = 3 * row[col[t]] + near[col[t]];
        v[0] = (3 * s[1] + s[0] + 8) >> 4; v[1] = (3 * s[1] + s[2] + 7) >> 4;
        v[2] = (3 * s[2] + s[1] + 8) >> 4; v[3] = (3 * s[2] + s[3] + 7) >> 4;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = row[col[t]];
        v[0] = (3 * s[1] + s[0] + 1) >> 2; v[1] = (3 * s[1] + s[2] + 2) >> 2;
        v[2] = (3 * s[2] + s[1] + 1) >> 2; v[3] = (3 * s[2] + s[3] + 2) >> 2;
    }
}

// a thread writes four neighbouring pixels of one frame row
__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegDesc* __restrict__ desc, const int32_t* __restrict__ tile_start, int n,
                                                         const uint8_t* __restrict__ planes)
{
    const int tile = blockIdx.x;
    const int img = find_image(tile_start, n, tile);
    const JpegDesc& D = desc[img];
    const int W = D.w, H = D.h, quads = (W + 3) >> 2;
    const int item = (tile - tile_start[img]) * 256 + threadIdx.x;
    if (item >= H * quads) return;
    const int y = item / quads, x0 = (item - y * quads) * 4, npx = min(4, W - x0);
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(planes + D.plane_off[0] + (int64_t)y * (D.bw[0] * 8) + x0);
    uint8_t px[12];
    if (D.nc == 1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) px[3 * t] = px[3 * t + 1] = px[3 * t + 2] = (uint8_t)((y4 >> (8 * t)) & 255);
    } else {
        int cb[4], cr[4];
        chroma4(D, planes, 1, y, x0, cb);
        chroma4(D, planes, 2, y, x0, cr);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int Y = (y4 >> (8 * t)) & 255, u = cb[t] - 128, v = cr[t] - 128;
            px[3 * t] = (uint8_t)min(max(Y + ((116130 * u + 32768) >> 16), 0), 255);
            px[3 * t + 1] = (uint8_t)min(max(Y + ((-22554 * u - 46802 * v + 32768) >> 16), 0), 255);
            px[3 * t + 2] = (uint8_t)min(max(Y + ((91881 * v + 32768) >> 16), 0), 255);
        }
    }
    uint8_t* out = D.frame + ((int64_t)y * W + x0) * 3;
    if (D.wide) {                                            // W is a multiple of 4 here: npx == 4
        uint32_t wd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) wd[k] = (uint32_t)px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
        uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
        o32[0] = wd[0]; o32[1] = wd[1]; o32[2] = wd[2];
    } else {
#pragma unroll
        for (int t = 0; t < 12; ++t)
            if (t < npx * 3) out[t] = px[t];
    }
}

struct JpegSlot {
    PinnedBuf<int16_t> coef;       // staging_bytes of coefficients
    PinnedBuf<char> table;         // [max_batch] JpegDesc, then int32 [max_batch + 1] group starts, int32 [max_batch + 1] tile starts
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;       // before the upload, after it (the slot may be rewritten), after the kernels
    bool used = false;
};

}  // namespace

struct JpegState {
    int device = 0, max_batch = 0, threads = 1;
    int64_t staging_bytes = 0;
    JpegSlot slot[2];
    int next = 0, last_slot = -1;
    DevBuf<int16_t> coef_dev;
    DevBuf<uint8_t> planes;
    DevBuf<char> table_dev;
    std::vector<ynjpeg::Header> hdr;
    std::vector<std::string> reasons;
    double host_ms = 0.0;
    bool launched = false;
    size_t table_bytes() const { return (size_t)max_batch * sizeof(JpegDesc) + 2 * ((size_t)max_batch + 1) * sizeof(int32_t); }
};

int jpeg_device(const JpegState* j) { return j->device; }

void jpeg_destroy(JpegState* j)
{
    if (!j) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    (void)hipSetDevice(j->device);
    if (j->launched) (void)hipDeviceSynchronize();           // the kernels read the buffers below, the copies read the pinned slots
    for (JpegSlot& s : j->slot)
        for (hipEvent_t e : {s.e0, s.e1, s.e2})
            if (e) (void)hipEventDestroy(e);
    delete j;
    if (prev >= 0) (void)hipSetDevice(prev);
}

int jpeg_create(int device, int max_batch, int64_t staging_bytes, int threads, JpegState** out, std::string& err)
{
    if (max_batch < 1 || max_batch > 1024) { err = "yn_jpeg_create: max_batch " + std::to_string(max_batch) + " outside 1..1024"; return 1; }
    if (staging_bytes < 128 || staging_bytes > ((int64_t)1 << 32)) { err = "yn_jpeg_create: staging_bytes " + std::to_string(staging_bytes) + " outside 128..2^32"; return 1; }
    if (threads < 1) { err = "yn_jpeg_create: threads " + std::to_string(threads) + " below 1"; return 1; }
    auto* j = new JpegState;
    j->device = device; j->max_batch = max_batch; j->threads = threads > 16 ? 16 : threads;
    j->staging_bytes = (staging_bytes + 127) / 128 * 128;                     // whole blocks
    const size_t elems = (size_t)j->staging_bytes / sizeof(int16_t);
    int r = j->coef_dev.reserve(elems);
    if (!r) r = j->planes.reserve(elems);
    if (!r) r = j->table_dev.reserve(j->table_bytes());
    for (JpegSlot& s : j->slot) {
        if (!r) r = s.coef.reserve(elems);
        if (!r) r = s.table.reserve(j->table_bytes());
        if (!r) r = (int)hipEventCreate(&s.e0);
        if (!r) r = (int)hipEventCreate(&s.e1);
        if (!r) r = (int)hipEventCreate(&s.e2);
    }
    if (r) {
        (void)hipGetLastError();
        err = std::string("yn_jpeg_create: ") + hipGetErrorString((hipError_t)r) + " (" + std::to_string(j->staging_bytes) + " staging bytes: twice that pinned, 1.5 times on the device)";
        jpeg_destroy(j);
        return 1;
    }
    *out = j;
    return 0;
}

const char* jpeg_reason(const JpegState* j, int i)
{
    if (!j || i < 0 || (size_t)i >= j->reasons.size()) return "";
    return j->reasons[(size_t)i].c_str();
}

int jpeg_decode_batch(JpegState* j, hipStream_t st, int n, const uint8_t* const* data, const int64_t* len, uint8_t* const* frames, int32_t* status,
                      int32_t* failed, std::string& err)
{
    if (n < 0) { err = "yn_jpeg_decode_batch: negative batch"; return 1; }
    if (failed) *failed = 0;
    j->reasons.assign((size_t)n, std::string());
    j->host_ms = 0.0;
    j->last_slot = -1;
    if (n == 0) return 0;
    if (!data || !len || !frames || !status) { err = "yn_jpeg_decode_batch: null argument"; return 1; }
    // headers of the whole batch first: a batch that does not fit fails before anything is written or launched
    j->hdr.assign((size_t)n, ynjpeg::Header());
    const auto t0 = std::chrono::steady_clock::now();
    ynjpeg::parallel_for(n, j->threads, [&](int i) {
        status[i] = (!data[i] || len[i] < 0) ? ynjpeg::refuse_null(j->reasons[(size_t)i]) : ynjpeg::parse(data[i], len[i], j->hdr[(size_t)i], j->reasons[(size_t)i]);
    });
    int64_t need = 0;
    for (int c0 = 0; c0 < n; c0 += j->max_batch) {
        int64_t bytes = 0;
        for (int i = c0; i < n && i < c0 + j->max_batch; ++i) {
            if (status[i] != ynjpeg::JPEG_OK) continue;
            if (!frames[i]) { err = "yn_jpeg_decode_batch: image " + std::to_string(i) + " has no frame"; return 1; }
            bytes += j->hdr[(size_t)i].coef_total * (int64_t)sizeof(int16_t);
        }
        if (bytes > need) need = bytes;
    }
    if (need > j->staging_bytes) {
        err = "yn_jpeg_decode_batch: the coefficients of " + std::to_string(n < j->max_batch ? n : j->max_batch) + " images need " + std::to_string(need) +
              " staging bytes, the decoder has " + std::to_string(j->staging_bytes);
        return 1;
    }
    j->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::vector<int64_t> off((size_t)j->max_batch);
    for (int c0 = 0; c0 < n; c0 += j->max_batch) {
        const int m = n - c0 < j->max_batch ? n - c0 : j->max_batch;
        JpegSlot& s = j->slot[j->next];
        if (s.used) {                                        // its previous upload must have left the pinned memory
            const hipError_t e = hipEventSynchronize(s.e1);
            if (e != hipSuccess) { err = std::string("yn_jpeg_decode_batch: ") + hipGetErrorString(e); return 1; }
        }
        int64_t total = 0;
        for (int i = 0; i < m; ++i) {
            off[(size_t)i] = total;
            if (status[c0 + i] == ynjpeg::JPEG_OK) total += j->hdr[(size_t)(c0 + i)].coef_total;
        }
        const auto t1 = std::chrono::steady_clock::now();
        ynjpeg::parallel_for(m, j->threads, [&](int i) {
            const int g = c0 + i;
            if (status[g] == ynjpeg::JPEG_OK) status[g] = ynjpeg::entropy_decode(data[g], len[g], j->hdr[(size_t)g], s.coef.get() + off[(size_t)i], j->reasons[(size_t)g]);
        });
        j->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        JpegDesc* desc = reinterpret_cast<JpegDesc*>(s.table.get());
        int32_t* group_start = reinterpret_cast<int32_t*>(s.table.get() + (size_t)j->max_batch * sizeof(JpegDesc));
        int32_t* tile_start = group_start + j->max_batch + 1;
        int k = 0;
        int64_t groups = 0, tiles = 0;
        for (int i = 0; i < m; ++i) {
            if (status[c0 + i] != ynjpeg::JPEG_OK) continue;
            const ynjpeg::Header& H = j->hdr[(size_t)(c0 + i)];
            JpegDesc& D = desc[k];
            memset(&D, 0, sizeof D);
            D.frame = frames[c0 + i];
            D.w = H.w; D.h = H.h; D.nc = H.nc; D.hs = H.hmax; D.vs = H.vmax;
            D.wide = (H.w % 4 == 0) && (reinterpret_cast<uintptr_t>(D.frame) % 4 == 0);
            group_start[k] = (int32_t)groups;
            tile_start[k] = (int32_t)tiles;
            for (int c = 0; c < H.nc; ++c) {
                memcpy(D.qt[c], H.qt[H.tq[c]], sizeof D.qt[c]);
                D.bw[c] = H.bw[c]; D.bh[c] = H.bh[c];
                D.dw[c] = (H.w * H.hs[c] + H.hmax - 1) / H.hmax;
                D.dh[c] = (H.h * H.vs[c] + H.vmax - 1) / H.vmax;
                D.coef_off[c] = off[(size_t)i] + H.coef_off[c];
                D.plane_off[c] = D.coef_off[c];              // one byte per coefficient, the same order
                D.group0[c] = (int32_t)groups;
                groups += ((int64_t)H.bw[c] * H.bh[c] + 7) / 8;
            }
            tiles += ((int64_t)H.h * ((H.w + 3) / 4) + 255) / 256;
            ++k;
        }
        group_start[k] = (int32_t)groups;
        tile_start[k] = (int32_t)tiles;
        if (k == 0) continue;                                // nothing of this chunk can be decoded: the slot stays free
        hipError_t e = hipEventRecord(s.e0, st);
        if (e == hipSuccess) e = hipMemcpyAsync(j->coef_dev.get(), s.coef.get(), (size_t)total * sizeof(int16_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(j->table_dev.get(), s.table.get(), j->table_bytes(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(s.e1, st);
        if (e != hipSuccess) { err = std::string("yn_jpeg_decode_batch: ") + hipGetErrorString(e); return 1; }
        s.used = true;
        j->launched = true;
        const JpegDesc* ddesc = reinterpret_cast<const JpegDesc*>(j->table_dev.get());
        const int32_t* dgroup = reinterpret_cast<const int32_t*>(j->table_dev.get() + (size_t)j->max_batch * sizeof(JpegDesc));
        const int32_t* dtile = dgroup + j->max_batch + 1;
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, st, ddesc, dgroup, k, j->coef_dev.get(), j->planes.get());
        hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)tiles), dim3(256), 0, st, ddesc, dtile, k, j->planes.get());
        e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(s.e2, st);
        if (e != hipSuccess) { err = std::string("yn_jpeg_decode_batch: ") + hipGetErrorString(e); return 1; }
        j->last_slot = j->next;
        j->next ^= 1;
    }
    int bad = 0;
    for (int i = 0; i < n; ++i) bad += status[i] != ynjpeg::JPEG_OK;
    if (failed) *failed = bad;
    return 0;
}

int jpeg_timing(JpegState* j, float* ms3, std::string& err)
{
    ms3[0] = (float)j->host_ms; ms3[1] = ms3[2] = 0.0f;
    if (j->last_slot < 0) return 0;
    JpegSlot& s = j->slot[j->last_slot];
    hipError_t e = hipEventSynchronize(s.e2);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms3[1], s.e0, s.e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms3[2], s.e1, s.e2);
    if (e != hipSuccess) { err = std::string("yn_jpeg_timing: ") + hipGetErrorString(e); return 1; }
    return 0;
}

// ---- host only: no device, no handle ------------------------------------------------------------------------------------------------
int jpeg_info(const uint8_t* data, int64_t len, int32_t* info8, std::string& reason)
{
    static thread_local ynjpeg::Header H;
    H = ynjpeg::Header();
    const int st = (!data || len < 0) ? ynjpeg::refuse_null(reason) : ynjpeg::parse(data, len, H, reason);
    info8[0] = H.w; info8[1] = H.h; info8[2] = H.nc; info8[3] = H.hmax; info8[4] = H.vmax; info8[5] = H.restart; info8[6] = H.sof; info8[7] = st;
    return st;
}

int jpeg_coefficients(const uint8_t* data, int64_t len, int16_t* coef, int64_t cap, uint16_t* qt, int32_t* grid, int64_t* needed, std::string& reason)
{
    static thread_local ynjpeg::Header H;
    H = ynjpeg::Header();
    *needed = 0;
    int st = (!data || len < 0) ? ynjpeg::refuse_null(reason) : ynjpeg::parse(data, len, H, reason);
    if (st != ynjpeg::JPEG_OK) return st;
    *needed = H.coef_total;
    for (int c = 0; c < 3; ++c) {
        if (grid) { grid[2 * c] = c < H.nc ? H.bh[c] : 0; grid[2 * c + 1] = c < H.nc ? H.bw[c] : 0; }
        if (qt) for (int k = 0; k < 64; ++k) qt[64 * c + k] = c < H.nc ? H.qt[H.tq[c]][k] : 0;
    }
    if (H.coef_total > cap || !coef) {
        reason = "the coefficients need " + std::to_string(H.coef_total) + " int16 elements, the buffer has " + std::to_string(cap);
        return ynjpeg::JPEG_TOO_LARGE;
    }
    return ynjpeg::entropy_decode(data, len, H, coef, reason);
}

}  // namespace ynk
