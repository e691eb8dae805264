// kernels_jpeg.hip — the device half of the baseline JPEG decode and the state behind yn_jpeg.
//
// The host (yn_jpeg_host.h) parses the markers and undoes the Huffman coding; what it uploads is int16 coefficients, 64 per block in natural
// order.  Two kernels finish a whole batch of images of different sizes and samplings, driven by one descriptor per image:
//   jpeg_idct_kernel    dequantise + libjpeg's jidctint 8x8 (integer, column pass then row pass) -> uint8 component planes padded to whole blocks
//   jpeg_color_kernel   libjpeg's "fancy" (triangle) chroma upsampling for 2x1 / 2x2 + YCbCr -> BGR, written as uint8 [h][w][3] frames
// Every step is the integer arithmetic of libjpeg's default decode (JDCT_ISLOW, do_fancy_upsampling), so the frames equal cv2.imread's and
// PIL's byte for byte (tests/jpeg_oracle.py restates the rules).  Nothing is addressed by data: garbage coefficients give garbage pixels, no fault.
// Opt-in (yn_jpeg_entropy): the Huffman stage runs on the device too (kernels_jpeg_huff.hip) and leaves the same coefficient
// buffer to the same two kernels; jpeg_entropy_device() below stages the scans, reads one result word per file back and lets the host decode
// whatever the device could not vouch for.
#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
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

// ---- the device entropy mode: what exists only after yn_jpeg_entropy(j, 1, ..) -------------------------------------------------
struct JpegHuffSlot {
    PinnedBuf<uint8_t> scan;       // the chunk's unstuffed scans, each file on a 16-byte boundary and zeroed up to the next one
    PinnedBuf<char> meta;          // FileDesc [max_batch], int32 [max_batch + 1] workgroup starts, Segment [seg_cap], Table [6 * max_batch]
    PinnedBuf<ynhuff::FileResult> result;
};

struct JpegHuffLast {              // a file of the last chunk, for the test entries
    int64_t off = 0, total = 0;
    int dev = -1;                  // its FileDesc, -1: the device never saw it
    int flag = 0;
};

struct JpegHuff {
    int sb = 0, max_rounds = 0, max_batch = 0;
    int64_t scan_cap = 0, seg_cap = 0;
    JpegHuffSlot slot[2];
    DevBuf<uint8_t> scan;
    DevBuf<char> meta;
    DevBuf<uint64_t> start, end;
    DevBuf<int32_t> nblk, base;
    DevBuf<ynhuff::FileResult> result;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};       // around: upload, clear, first round, sync, write, dc
    bool timed = false;
    int64_t device_files = 0, host_files = 0, decodes_last = 0;
    int32_t rounds_last = 0, subseqs_last = 0;
    std::vector<JpegHuffLast> last;
    std::vector<ynhuff::FileDesc> last_desc;
    std::vector<ynjpeg::ScanSegment> segs;
    std::vector<ynjpeg::ScanInfo> info;
    std::vector<int64_t> scan_off, seg_off;
    size_t files_bytes() const { return ((size_t)max_batch * sizeof(ynhuff::FileDesc) + ((size_t)max_batch + 1) * sizeof(int32_t) + 15) / 16 * 16; }
    size_t segs_at() const { return files_bytes(); }
    size_t tables_at() const { return segs_at() + (size_t)seg_cap * sizeof(ynhuff::Segment); }
    size_t meta_bytes() const { return tables_at() + 6 * (size_t)max_batch * sizeof(ynhuff::Table); }
    ~JpegHuff()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

struct JpegState {
    std::unique_ptr<JpegHuff> huff;                          // null: the host decodes the Huffman stage
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
    DeviceScope on(j->device);
    if (j->launched) (void)hipDeviceSynchronize();           // the kernels read the buffers below, the copies read the pinned slots
    for (JpegSlot& s : j->slot)
        for (hipEvent_t e : {s.e0, s.e1, s.e2})
            if (e) (void)hipEventDestroy(e);
    delete j;
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

static int64_t scan_reserve(int64_t stuffed) { return stuffed > 0 ? (stuffed + 15) / 16 * 16 : 16; }      // what a file's unstuffed scan may take of the slot

#define YN_JPEG_HIP(call)                                                                              \
    do {                                                                                               \
        const hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) { err = std::string("yn_jpeg_decode_batch: ") + hipGetErrorString(e_); return 1; } \
    } while (0)

// The Huffman stage of one chunk on the device.  On return the coefficients of every file that is still JPEG_OK are in (or on
// their way to) coef_dev at off[i]; a file the device could not vouch for went through entropy_decode on the worker pool, which decided its
// status and reason and whose coefficients were uploaded over the device's.  Synchronous: it waits for the chunk's result words.
static int jpeg_entropy_device(JpegState* j, JpegSlot& s, hipStream_t st, int c0, int m, const uint8_t* const* data, const int64_t* len, int32_t* status,
                               const std::vector<int64_t>& off, int64_t total, std::string& err)
{
    using namespace ynhuff;
    JpegHuff& F = *j->huff;
    JpegHuffSlot& hs = F.slot[j->next];
    const auto t0 = std::chrono::steady_clock::now();
    F.scan_off.assign((size_t)m, 0); F.seg_off.assign((size_t)m, 0);
    F.info.assign((size_t)m, ynjpeg::ScanInfo());
    F.last.assign((size_t)m, JpegHuffLast());
    F.last_desc.clear();
    F.rounds_last = 0; F.subseqs_last = 0; F.decodes_last = 0; F.timed = false;
    int64_t sbytes = 0, nsegs = 0;
    for (int i = 0; i < m; ++i) {
        if (status[c0 + i] != ynjpeg::JPEG_OK) continue;
        const ynjpeg::Header& H = j->hdr[(size_t)(c0 + i)];
        F.scan_off[(size_t)i] = sbytes; sbytes += scan_reserve(len[c0 + i] - H.scan_pos);
        F.seg_off[(size_t)i] = nsegs; nsegs += ynjpeg::scan_segments(H);
        F.last[(size_t)i].off = off[(size_t)i]; F.last[(size_t)i].total = H.coef_total;
    }
    if (sbytes > F.scan_cap || nsegs > F.seg_cap) { err = "yn_jpeg_decode_batch: the scans of a chunk outgrew their staging slot"; return 1; }
    F.segs.resize((size_t)nsegs);
    const int copiers = (int)(1 + (sbytes >> 21)) < j->threads ? (int)(1 + (sbytes >> 21)) : j->threads;      // a worker per 2 MiB: starting one costs what copying 1 MiB does
    ynjpeg::parallel_for(m, copiers, [&](int i) {
        const int g = c0 + i;
        if (status[g] != ynjpeg::JPEG_OK) return;
        const ynjpeg::Header& H = j->hdr[(size_t)g];
        uint8_t* out = hs.scan.get() + F.scan_off[(size_t)i];
        ynjpeg::ScanInfo& I = F.info[(size_t)i];
        ynjpeg::scan_prepare(data[g], len[g], H, out, len[g] - H.scan_pos, F.segs.data() + F.seg_off[(size_t)i], ynjpeg::scan_segments(H), I);
        memset(out + I.bytes, 0, (size_t)((I.bytes + 15) / 16 * 16 - I.bytes));
    });
    FileDesc* fd = reinterpret_cast<FileDesc*>(hs.meta.get());
    int32_t* wg_start = reinterpret_cast<int32_t*>(hs.meta.get() + (size_t)F.max_batch * sizeof(FileDesc));
    Segment* dseg = reinterpret_cast<Segment*>(hs.meta.get() + F.segs_at());
    Table* dtab = reinterpret_cast<Table*>(hs.meta.get() + F.tables_at());
    const int per_wg = jpeg_huff_write_threads();
    int nf = 0, ntab = 0;
    int64_t nsub = 0, wgs = 0, ndseg = 0;
    Table fresh;
    for (int i = 0; i < m; ++i) {
        if (status[c0 + i] != ynjpeg::JPEG_OK || F.info[(size_t)i].host) continue;
        const ynjpeg::Header& H = j->hdr[(size_t)(c0 + i)];
        const ynjpeg::ScanInfo& I = F.info[(size_t)i];
        FileDesc& D = fd[nf];
        memset(&D, 0, sizeof D);
        ynjpeg::huff_geometry(H, off[(size_t)i], D.G);
        D.scan_off = F.scan_off[(size_t)i]; D.scan_bytes = I.bytes;
        D.seg0 = (int32_t)ndseg; D.nseg = I.segments; D.sub0 = (int32_t)nsub; D.nc = H.nc;
        int64_t fsub = 0;
        for (int k = 0; k < I.segments; ++k) {
            const ynjpeg::ScanSegment& a = F.segs[(size_t)(F.seg_off[(size_t)i] + k)];
            const int64_t end = k + 1 < I.segments ? F.segs[(size_t)(F.seg_off[(size_t)i] + k + 1)].start : I.bytes;
            const int64_t bits = (end - a.start) * 8;
            Segment& g = dseg[ndseg++];
            g.start = a.start; g.first_mcu = a.first_mcu; g.sub0 = (int32_t)fsub; g.pad = 0;
            fsub += bits > F.sb ? (bits + F.sb - 1) / F.sb : 1;
        }
        D.nsub = (int32_t)fsub;
        for (int c = 0; c < H.nc; ++c)
            for (int ac = 0; ac < 2; ++ac) {                 // identical tables of a chunk are stored once
                ynjpeg::huff_table(ac ? H.ac[H.ta[c]] : H.dc[H.td[c]], fresh);
                int at = 0;
                while (at < ntab && memcmp(&dtab[at], &fresh, sizeof fresh) != 0) ++at;
                if (at == ntab) dtab[ntab++] = fresh;
                D.tab[2 * c + ac] = at;
            }
        wg_start[nf] = (int32_t)wgs;
        wgs += (fsub + per_wg - 1) / per_wg;
        nsub += fsub;
        F.last[(size_t)i].dev = nf;
        F.last_desc.push_back(D);
        ++nf;
    }
    wg_start[nf] = (int32_t)wgs;
    j->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    YN_JPEG_HIP(hipEventRecord(s.e0, st));
    if (nf) {
        if (nsub > 0x7fffffff || wgs > 0x7fffffff) { err = "yn_jpeg_decode_batch: more than 2^31 subsequences in a chunk; raise subseq_bits"; return 1; }
        int r = F.start.reserve((size_t)nsub, 4096);
        if (!r) r = F.end.reserve((size_t)nsub, 4096);
        if (!r) r = F.nblk.reserve((size_t)nsub, 4096);
        if (!r) r = F.base.reserve((size_t)nsub, 4096);
        if (r) { (void)hipGetLastError(); err = std::string("yn_jpeg_decode_batch: ") + hipGetErrorString((hipError_t)r) + " (" + std::to_string(nsub) + " subsequences)"; return 1; }
        YN_JPEG_HIP(hipEventRecord(F.ev[0], st));
        YN_JPEG_HIP(hipMemcpyAsync(F.scan.get(), hs.scan.get(), (size_t)sbytes, hipMemcpyHostToDevice, st));
        YN_JPEG_HIP(hipMemcpyAsync(F.meta.get(), hs.meta.get(), F.files_bytes(), hipMemcpyHostToDevice, st));
        YN_JPEG_HIP(hipMemcpyAsync(F.meta.get() + F.segs_at(), dseg, (size_t)ndseg * sizeof(Segment), hipMemcpyHostToDevice, st));
        YN_JPEG_HIP(hipMemcpyAsync(F.meta.get() + F.tables_at(), dtab, (size_t)ntab * sizeof(Table), hipMemcpyHostToDevice, st));
        YN_JPEG_HIP(hipEventRecord(F.ev[1], st));
        YN_JPEG_HIP(hipMemsetAsync(j->coef_dev.get(), 0, (size_t)total * sizeof(int16_t), st));
        YN_JPEG_HIP(hipEventRecord(F.ev[2], st));
        j->launched = true;
        s.used = true;
        JpegHuffArgs a;
        a.files = F.meta.get();
        a.wg_start = reinterpret_cast<const int32_t*>(F.meta.get() + (size_t)F.max_batch * sizeof(FileDesc));
        a.segs = F.meta.get() + F.segs_at();
        a.tables = F.meta.get() + F.tables_at();
        a.scan = F.scan.get();
        a.start = F.start.get(); a.end = F.end.get(); a.nblk = F.nblk.get(); a.base = F.base.get();
        a.result = F.result.get();
        a.coef = j->coef_dev.get();
        a.nfiles = nf; a.write_wgs = (int)wgs; a.sb = F.sb; a.max_rounds = F.max_rounds;
        jpeg_huff_launch(a, st, F.ev[3], F.ev[4], F.ev[5]);
        YN_JPEG_HIP(hipGetLastError());
        YN_JPEG_HIP(hipEventRecord(F.ev[6], st));
        YN_JPEG_HIP(hipMemcpyAsync(hs.result.get(), F.result.get(), (size_t)nf * sizeof(FileResult), hipMemcpyDeviceToHost, st));
        YN_JPEG_HIP(hipEventRecord(s.e1, st));               // the slot's pinned memory is free again once this has passed
        YN_JPEG_HIP(hipStreamSynchronize(st));               // the one synchronisation of the mode: the per-file result words
        F.timed = true;
    }
    // what the device could not vouch for takes the host decoder, which knows the status and the reason
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<int> redo;
    for (int i = 0; i < m; ++i) {
        if (status[c0 + i] != ynjpeg::JPEG_OK) continue;
        JpegHuffLast& L = F.last[(size_t)i];
        if (L.dev >= 0) {
            const FileResult& R = hs.result.get()[L.dev];
            L.flag = R.flag;
            F.subseqs_last += R.nsub; F.decodes_last += R.decodes;
            if (R.rounds > F.rounds_last) F.rounds_last = R.rounds;
        }
        if (L.dev < 0 || L.flag) redo.push_back(i); else F.device_files += 1;
    }
    F.host_files += (int64_t)redo.size();
    ynjpeg::parallel_for((int)redo.size(), j->threads, [&](int r) {
        const int i = redo[(size_t)r], g = c0 + i;
        status[g] = ynjpeg::entropy_decode(data[g], len[g], j->hdr[(size_t)g], s.coef.get() + off[(size_t)i], j->reasons[(size_t)g]);
    });
    j->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    for (int i : redo) {
        if (status[c0 + i] != ynjpeg::JPEG_OK) continue;
        YN_JPEG_HIP(hipMemcpyAsync(j->coef_dev.get() + off[(size_t)i], s.coef.get() + off[(size_t)i], (size_t)j->hdr[(size_t)(c0 + i)].coef_total * sizeof(int16_t),
                                   hipMemcpyHostToDevice, st));
        j->launched = true;
        s.used = true;
    }
    return 0;
}
#undef YN_JPEG_HIP

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
    const int parsers = !j->huff ? j->threads : 1 + n / 64 < j->threads ? 1 + n / 64 : j->threads;      // device entropy mode: the host's work is small, a worker per 64 headers
    ynjpeg::parallel_for(n, parsers, [&](int i) {
        status[i] = (!data[i] || len[i] < 0) ? ynjpeg::refuse_null(j->reasons[(size_t)i]) : ynjpeg::parse(data[i], len[i], j->hdr[(size_t)i], j->reasons[(size_t)i]);
    });
    int64_t need = 0, need_scan = 0;
    for (int c0 = 0; c0 < n; c0 += j->max_batch) {
        int64_t bytes = 0, scan = 0;
        for (int i = c0; i < n && i < c0 + j->max_batch; ++i) {
            if (status[i] != ynjpeg::JPEG_OK) continue;
            if (!frames[i]) { err = "yn_jpeg_decode_batch: image " + std::to_string(i) + " has no frame"; return 1; }
            bytes += j->hdr[(size_t)i].coef_total * (int64_t)sizeof(int16_t);
            scan += scan_reserve(len[i] - j->hdr[(size_t)i].scan_pos);
        }
        if (bytes > need) need = bytes;
        if (scan > need_scan) need_scan = scan;
    }
    // device entropy mode: the unstuffed scans of a chunk are staged too, in a slot of their own of the same size.  The segment table holds
    // a segment per 128 coefficient bytes and the table store six tables per image: whatever fits above fits those.
    if (j->huff && need_scan > j->huff->scan_cap) {
        err = "yn_jpeg_decode_batch: the scans of " + std::to_string(n < j->max_batch ? n : j->max_batch) + " images need " + std::to_string(need_scan) +
              " staging bytes, the decoder has " + std::to_string(j->huff->scan_cap);
        return 1;
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
        if (j->huff) {
            if (jpeg_entropy_device(j, s, st, c0, m, data, len, status, off, total, err)) return 1;
        } else {
            const auto t1 = std::chrono::steady_clock::now();
            ynjpeg::parallel_for(m, j->threads, [&](int i) {
                const int g = c0 + i;
                if (status[g] == ynjpeg::JPEG_OK) status[g] = ynjpeg::entropy_decode(data[g], len[g], j->hdr[(size_t)g], s.coef.get() + off[(size_t)i], j->reasons[(size_t)g]);
            });
            j->host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
        }
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
        hipError_t e = j->huff ? hipSuccess : hipEventRecord(s.e0, st);      // device entropy mode: e0 went in front of its uploads
        if (e == hipSuccess && !j->huff) e = hipMemcpyAsync(j->coef_dev.get(), s.coef.get(), (size_t)total * sizeof(int16_t), hipMemcpyHostToDevice, st);
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

int jpeg_scan_prepare(const uint8_t* data, int64_t len, uint8_t* unstuffed, int64_t cap, int32_t* segments, int64_t seg_cap, int32_t* info4, std::string& reason)
{
    static thread_local ynjpeg::Header H;
    H = ynjpeg::Header();
    info4[0] = info4[1] = info4[2] = info4[3] = 0;
    const int st = (!data || len < 0) ? ynjpeg::refuse_null(reason) : ynjpeg::parse(data, len, H, reason);
    if (st != ynjpeg::JPEG_OK) return st;
    const int64_t want = ynjpeg::scan_segments(H);
    info4[3] = (int32_t)want;
    if (!unstuffed || cap < len - H.scan_pos || !segments || seg_cap < want) {
        reason = "the scan needs " + std::to_string(len - H.scan_pos) + " bytes and " + std::to_string(want) + " segments";
        return ynjpeg::JPEG_TOO_LARGE;
    }
    std::vector<ynjpeg::ScanSegment> segs((size_t)want);
    ynjpeg::ScanInfo I;
    ynjpeg::scan_prepare(data, len, H, unstuffed, cap, segs.data(), want, I);
    for (int k = 0; k < I.segments; ++k) { segments[2 * k] = (int32_t)segs[(size_t)k].start; segments[2 * k + 1] = segs[(size_t)k].first_mcu; }
    info4[0] = (int32_t)I.bytes; info4[1] = I.segments; info4[2] = I.host ? 1 : 0;
    return ynjpeg::JPEG_OK;
}

// ---- the entropy mode --------------------------------------------------------------------------------------------------------------------
enum { HUFF_DEFAULT_BITS = 1024, HUFF_DEFAULT_ROUNDS = 64 };

int jpeg_entropy(JpegState* j, int mode, int subseq_bits, int max_rounds, std::string& err)
{
    if (mode != 0 && mode != 1) { err = "yn_jpeg_entropy: mode " + std::to_string(mode) + " is neither 0 (host) nor 1 (device)"; return 1; }
    if (subseq_bits < 0 || subseq_bits % 32 || subseq_bits > (1 << 20)) { err = "yn_jpeg_entropy: subseq_bits " + std::to_string(subseq_bits) + " is no multiple of 32 in 32..2^20 (0: the default)"; return 1; }
    if (max_rounds < 0 || max_rounds > (1 << 24)) { err = "yn_jpeg_entropy: max_rounds " + std::to_string(max_rounds) + " outside 1..2^24 (0: the default)"; return 1; }
    DeviceScope on(j->device);
    if (j->launched) (void)hipDeviceSynchronize();           // nothing in flight reads what is released or replaced below
    j->huff.reset();
    int r = 0;
    if (mode == 1) {
        std::unique_ptr<JpegHuff> F(new JpegHuff);
        F->sb = subseq_bits ? subseq_bits : HUFF_DEFAULT_BITS;
        F->max_rounds = max_rounds ? max_rounds : HUFF_DEFAULT_ROUNDS;
        F->max_batch = j->max_batch;
        F->scan_cap = j->staging_bytes + 16 * (int64_t)j->max_batch;
        F->seg_cap = j->staging_bytes / 128 + j->max_batch;
        r = F->scan.reserve((size_t)F->scan_cap);
        if (!r) r = F->meta.reserve(F->meta_bytes());
        if (!r) r = F->result.reserve((size_t)j->max_batch);
        for (JpegHuffSlot& s : F->slot) {
            if (!r) r = s.scan.reserve((size_t)F->scan_cap);
            if (!r) r = s.meta.reserve(F->meta_bytes());
            if (!r) r = s.result.reserve((size_t)j->max_batch);
        }
        for (hipEvent_t& e : F->ev)
            if (!r) r = (int)hipEventCreate(&e);
        if (r) {
            (void)hipGetLastError();
            err = std::string("yn_jpeg_entropy: ") + hipGetErrorString((hipError_t)r) + " (the device mode stages the scans: " + std::to_string(F->scan_cap) + " bytes twice pinned, once on the device)";
        } else {
            j->huff = std::move(F);
        }
    }
    return r ? 1 : 0;
}

void jpeg_entropy_stats(const JpegState* j, int64_t* device_files, int64_t* host_files, int32_t* rounds_last, int32_t* subseqs_last)
{
    const JpegHuff* F = j->huff.get();
    if (device_files) *device_files = F ? F->device_files : 0;
    if (host_files) *host_files = F ? F->host_files : 0;
    if (rounds_last) *rounds_last = F ? F->rounds_last : 0;
    if (subseqs_last) *subseqs_last = F ? F->subseqs_last : 0;
}

static const JpegHuffLast* huff_last(JpegState* j, int i, const char* who, std::string& err)
{
    if (!j->huff) { err = std::string(who) + ": the decoder is in host entropy mode"; return nullptr; }
    if (i < 0 || (size_t)i >= j->huff->last.size()) { err = std::string(who) + ": file " + std::to_string(i) + " outside the last chunk of " + std::to_string(j->huff->last.size()); return nullptr; }
    const JpegHuffLast& L = j->huff->last[(size_t)i];
    if (L.dev < 0 || L.flag) { err = std::string(who) + ": file " + std::to_string(i) + " of the last chunk took the host decoder (flag " + std::to_string(L.dev < 0 ? -1 : L.flag) + ")"; return nullptr; }
    return &L;
}

int jpeg_device_coefficients(JpegState* j, hipStream_t s, int i, int16_t* host, int64_t cap, std::string& err)
{
    const JpegHuffLast* L = huff_last(j, i, "yn_jpeg_device_coefficients", err);
    if (!L) return 1;
    if (!host || cap < L->total) { err = "yn_jpeg_device_coefficients: the file has " + std::to_string(L->total) + " coefficients, the buffer " + std::to_string(cap); return 1; }
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(host, j->coef_dev.get() + L->off, (size_t)L->total * sizeof(int16_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = std::string("yn_jpeg_device_coefficients: ") + hipGetErrorString(e); return 1; }
    return 0;
}

int jpeg_entropy_states(JpegState* j, hipStream_t s, int i, int32_t* host, int64_t cap, std::string& err)
{
    const JpegHuffLast* L = huff_last(j, i, "yn_jpeg_entropy_states", err);
    if (!L) return 1;
    const ynhuff::FileDesc& D = j->huff->last_desc[(size_t)L->dev];
    if (!host || cap < 4 * (int64_t)D.nsub) { err = "yn_jpeg_entropy_states: the file has " + std::to_string(D.nsub) + " subsequences of 4 numbers, the buffer holds " + std::to_string(cap); return 1; }
    std::vector<uint64_t> st((size_t)D.nsub);
    std::vector<int32_t> before((size_t)D.nsub);
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(st.data(), j->huff->start.get() + D.sub0, st.size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(before.data(), j->huff->base.get() + D.sub0, before.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = std::string("yn_jpeg_entropy_states: ") + hipGetErrorString(e); return 1; }
    for (int32_t k = 0; k < D.nsub; ++k) {
        host[4 * k] = (int32_t)ynhuff::state_bit(st[(size_t)k]); host[4 * k + 1] = ynhuff::state_u(st[(size_t)k]);
        host[4 * k + 2] = ynhuff::state_k(st[(size_t)k]); host[4 * k + 3] = before[(size_t)k];
    }
    return 0;
}

int jpeg_entropy_timing(JpegState* j, float* ms7, std::string& err)
{
    for (int k = 0; k < 7; ++k) ms7[k] = 0.0f;
    JpegHuff* F = j->huff.get();
    if (!F || !F->timed) return 0;
    hipError_t e = hipEventSynchronize(F->ev[6]);
    for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipEventElapsedTime(&ms7[k], F->ev[k], F->ev[k + 1]);
    if (e != hipSuccess) { err = std::string("yn_jpeg_entropy_timing: ") + hipGetErrorString(e); return 1; }
    ms7[6] = F->subseqs_last ? (float)((double)F->decodes_last / F->subseqs_last) : 0.0f;
    return 0;
}

}  // namespace ynk
