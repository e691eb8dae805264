// kernels_jpeg_enc.hip — baseline JPEG files written on the device and the state behind yn_jpeg_enc.
//
// uint8 [h][w][3] BGR frames in, complete files out, byte for byte what libjpeg writes with its defaults (JDCT_ISLOW, the Annex K tables, no
// optimisation): cv2.imwrite's and PIL's files.  One launch chain serves a batch of frames of any sizes, driven by one descriptor per image:
//   jpeg_fdct_kernel     rgb_ycc_convert, edge replication, chroma downsampling, jfdctint 8x8, quantisation -> int16 zigzag blocks in scan order
//   jpeg_bits_kernel     a wavefront per block, a lane per zigzag position: the bits of the block's Huffman codes
//   enc_scan_*           exclusive 64-bit scan of those lengths over the whole batch; an image's offsets are differences of it
//   jpeg_emit_kernel     the same codes again, gathered per block in LDS and written into the zeroed unstuffed stream at their offsets
//   jpeg_ffcount_kernel  0xFF bytes per 256-byte chunk; scanned the same way
//   jpeg_file_kernel     header, the bytes with a 0x00 after every 0xFF, FF D9
// The size of a file is known on the device only.  enc_layout_stream / enc_layout_files compare it with the buffers BEFORE anything is
// written at a data-dependent address: an image that does not fit is flagged and skipped, and yn_jpeg_encode_fetch reports it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "yn_internal.h"

namespace ynk {

namespace {

constexpr int ENC_HEADER = 623;            // SOI .. SOS
constexpr int ENC_GUARD = 64;              // bytes behind the output buffer that nothing may touch (yn_jpeg_enc_guard)
constexpr int SCAN_TILE = 2048;            // elements a workgroup scans
constexpr int CHUNK = 256;                 // unstuffed bytes a wavefront stuffs: 4 per lane
constexpr int HUFF_STRIDE = 12 + 256;      // per table pair: 12 DC entries, 256 AC entries; an entry is code | length << 16
constexpr int64_t ENC_MAX_BLOCKS = (int64_t)1 << 24;      // per call: 2 GiB of coefficients, a 3.3 GiB worst-case stream
constexpr int ENC_EVENTS = 11;

#define YN_ZIGZAG                                                                                                                        \
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, \
        43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
const uint8_t kZigzag[64] = {YN_ZIGZAG};                  // zigzag position -> natural index
__device__ const uint8_t d_zigzag[64] = {YN_ZIGZAG};

// Annex K.1 in the zigzag order of a DQT segment; Annex K.3 code counts and symbols
const uint8_t kBaseQ[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const uint8_t kDcCounts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kAcCounts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kAcSyms[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

struct alignas(16) EncDesc {
    const uint8_t* frame;          // uint8 [h][w][3] BGR
    int32_t w, h, hs, vs;          // hs x vs: the luma sampling factors = how far the chroma planes are downsampled
    int32_t mw, bpm;               // MCUs per row, blocks per MCU (hs * vs + 2)
    int32_t wib, hib;              // luma blocks that hold image samples; the MCU grid may be larger (dummy blocks)
    int32_t block0, pad;           // first block of the image in the call's numbering
    uint16_t q8[2][64];            // the divisors 8 q, natural order: luma, chroma
    uint8_t header[ENC_HEADER + 1];
};
static_assert(sizeof(EncDesc) % 16 == 0, "descriptor table stride");

struct EncImage {                  // what the device learns about an image while it encodes
    int64_t bit_base;              // the scan of the bit lengths at its first block
    int64_t ubytes;                // unstuffed bytes, the fill bits included
    int64_t ff_base;               // the scan of the 0xFF counts at its first chunk
    int64_t file_off, file_bytes;
    int32_t chunk0;                // its first chunk of the unstuffed stream
    int32_t fits;                  // bit 0: the unstuffed stream holds it, bit 1: the output buffer holds its file.  Only 3 is ever written.
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

// jfdctint's 1-D pass (constants round(x * 2^13)).  FIRST: the row pass (outputs 0 and 4 scaled up by 4, the others descaled by 11);
// else the column pass (descaled by 2 and 15).
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int32_t (&d)[8], int32_t (&o)[8])
{
    const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
    if (FIRST) { o[0] = (t10 + t11) * 4; o[4] = (t10 - t11) * 4; }
    else { o[0] = (t10 + t11 + 2) >> 2; o[4] = (t10 - t11 + 2) >> 2; }
    int32_t z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + R) >> N;
    o[6] = (z1 - t12 * 15137 + R) >> N;
    z1 = t4 + t7;
    int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int32_t z5 = (z3 + z4) * 9633;
    const int32_t a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    o[7] = (a4 + z1 + z3 + R) >> N; o[5] = (a5 + z2 + z4 + R) >> N;
    o[3] = (a6 + z2 + z3 + R) >> N; o[1] = (a7 + z1 + z4 + R) >> N;
}

// one sample of component c at (row, col) of the full-resolution frame, libjpeg's rgb_ycc_convert
__device__ __forceinline__ int ycc(const EncDesc& D, int c, int row, int col)
{
    const uint8_t* p = D.frame + ((int64_t)row * D.w + col) * 3;
    const int B = p[0], G = p[1], R = p[2];
    if (c == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (c == 1) return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

// where block `lb` of an image lies: MCU, index inside the MCU, component
struct BlockPos { int mcu, k, comp, bx, by; };
__device__ __forceinline__ BlockPos block_pos(const EncDesc& D, int lb)
{
    BlockPos P;
    P.mcu = lb / D.bpm;
    P.k = lb - P.mcu * D.bpm;
    const int nl = D.hs * D.vs, my = P.mcu / D.mw, mx = P.mcu - my * D.mw;
    P.comp = P.k < nl ? 0 : P.k - nl + 1;
    P.bx = P.comp ? mx : mx * D.hs + P.k % D.hs;
    P.by = P.comp ? my : my * D.vs + P.k / D.hs;
    return P;
}

constexpr int FDCT_LD = 9;          // LDS row stride of a block in words: 8 + 1 against bank conflicts of the transposed accesses

// A wavefront takes 8 blocks: lane = (block, j).  The lane gathers row j of the block's samples (colour conversion, edges and downsampling
// included), runs the row pass on it, owns COLUMN j in the second pass (the transpose goes through LDS), quantises, and stores 8 zigzag
// positions (16 bytes).  A dummy block (rule 3) computes the block it copies its DC from and drops the AC terms: no block waits for another.
__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const EncDesc* __restrict__ desc, const int32_t* __restrict__ block_start, int n,
                                                        int16_t* __restrict__ coef)
{
    __shared__ int32_t ws[4][8][8 * FDCT_LD];
    __shared__ int16_t qs[4][8][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = lane >> 3, j = lane & 7;
    const int blk = (blockIdx.x * 4 + wave) * 8 + b;
    const bool live = blk < block_start[n];
    const int img = live ? find_image(block_start, n, blk) : 0;
    const EncDesc& D = desc[img];
    int32_t* w = ws[wave][b];
    int16_t* q = qs[wave][b];
    bool dummy = false;
    int comp = 0;
    if (live) {
        BlockPos P = block_pos(D, blk - D.block0);
        comp = P.comp;
        if (comp == 0) {                                     // the block this one copies: the nearest real one before it in the MCU
            int k = P.k;
            while (k > 0 && (P.bx >= D.wib || P.by >= D.hib)) {
                --k;
                P.bx += (k % D.hs) - ((k + 1) % D.hs);
                P.by += (k / D.hs) - ((k + 1) / D.hs);
            }
            dummy = k != P.k;
        }
        const int fh = comp ? D.hs : 1, fv = comp ? D.vs : 1;
        const int rows = (D.h + fv - 1) / fv;                // downsampled rows that exist: the last one is replicated below (rule 2)
        const int cy = min(P.by * 8 + j, rows - 1);
        int32_t s[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cx = P.bx * 8 + i;
            int sum = 0;
            for (int dy = 0; dy < fv; ++dy)
                for (int dx = 0; dx < fh; ++dx) sum += ycc(D, comp, min(cy * fv + dy, D.h - 1), min(cx * fh + dx, D.w - 1));
            if (fh == 2) sum = fv == 2 ? (sum + 1 + (cx & 1)) >> 2 : (sum + (cx & 1)) >> 1;
            s[i] = sum - 128;
        }
        fdct_1d<true>(s, o);
#pragma unroll
        for (int i = 0; i < 8; ++i) w[j * FDCT_LD + i] = o[i];
    }
    __syncthreads();
    if (live) {
        int32_t x[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = w[r * FDCT_LD + j];
        fdct_1d<false>(x, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int qv = D.q8[comp ? 1 : 0][r * 8 + j];
            const int a = (abs(o[r]) + (qv >> 1)) / qv;
            q[r * 8 + j] = (int16_t)((dummy && (r | j)) ? 0 : (o[r] < 0 ? -a : a));
        }
    }
    __syncthreads();
    if (live) {
        uint32_t pk[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            pk[t] = (uint32_t)(uint16_t)q[d_zigzag[j * 8 + 2 * t]] | (uint32_t)(uint16_t)q[d_zigzag[j * 8 + 2 * t + 1]] << 16;
        *reinterpret_cast<uint4*>(coef + (int64_t)blk * 64 + j * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    }
}

// The code bits of one zigzag position of one block (lane = position), at most 59: up to three ZRL codes, the (run, size) code and the
// value's bits; position 0 carries the DC difference, position 63 the end-of-block code when it is zero.  Returns the lane's offset inside
// the block (an inclusive wave scan minus its own length) and the block's total.
struct LaneCode { uint64_t bits; int len, off, total; };
__device__ __forceinline__ LaneCode lane_code(const EncDesc& D, const int16_t* __restrict__ coef, const uint32_t* __restrict__ huff, int blk, int lane)
{
    const BlockPos P = block_pos(D, blk - D.block0);
    const int nl = D.hs * D.vs;
    int v = coef[(int64_t)blk * 64 + lane];
    if (lane == 0) {                                         // the previous block of the same component in scan order
        int prev = -1;
        if (P.comp == 0) prev = P.k > 0 ? blk - 1 : (P.mcu > 0 ? blk - D.bpm + nl - 1 : -1);
        else if (P.mcu > 0) prev = blk - D.bpm;
        if (prev >= 0) v -= coef[(int64_t)prev * 64];
    }
    const uint32_t* T = huff + (P.comp ? HUFF_STRIDE : 0);
    const uint64_t mask = __ballot(v != 0) | 1ull;
    const int a = abs(v), size = 32 - __clz(a);
    const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    LaneCode C;
    C.bits = 0; C.len = 0;
    if (lane == 0) {
        const uint32_t e = T[min(size, 11)];
        C.bits = ((uint64_t)(e & 0xffffu) << size) | extra;
        C.len = (int)(e >> 16) + size;
    } else if (v != 0) {
        const int prev = 63 - __clzll((long long)(mask & ((1ull << lane) - 1ull)));
        const int run = lane - prev - 1;
        const uint32_t z = T[12 + 0xF0], e = T[12 + (((run & 15) << 4) | min(size, 10))];
        for (int i = 0; i < (run >> 4); ++i) {
            C.bits = (C.bits << (z >> 16)) | (z & 0xffffu);
            C.len += (int)(z >> 16);
        }
        C.bits = (((C.bits << (e >> 16)) | (e & 0xffffu)) << size) | extra;
        C.len += (int)(e >> 16) + size;
    } else if (lane == 63) {
        const uint32_t e = T[12];
        C.bits = e & 0xffffu;
        C.len = (int)(e >> 16);
    }
    int incl = C.len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    C.off = incl - C.len;
    C.total = __shfl(incl, 63);
    return C;
}

__global__ __launch_bounds__(256) void jpeg_bits_kernel(const EncDesc* __restrict__ desc, const int32_t* __restrict__ block_start, int n,
                                                        const int16_t* __restrict__ coef, const uint32_t* __restrict__ huff, uint32_t* __restrict__ block_bits)
{
    const int lane = threadIdx.x & 63, blk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= block_start[n]) return;                       // uniform over the wavefront
    const LaneCode C = lane_code(desc[find_image(block_start, n, blk)], coef, huff, blk, lane);
    if (lane == 0) block_bits[blk] = (uint32_t)C.total;
}

// ---- exclusive scan of uint32 values into 64 bits: scan(i) = tile_base[i / SCAN_TILE] + local[i], scan(count) = tile_base[tiles] ---------
__global__ __launch_bounds__(256) void enc_scan_tiles_kernel(const uint32_t* __restrict__ val, int64_t count, uint32_t* __restrict__ local,
                                                             int64_t* __restrict__ tile_sum)
{
    __shared__ uint32_t part[256];
    const int64_t i0 = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 8;
    uint32_t v[8], sum = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) { v[t] = i0 + t < count ? val[i0 + t] : 0u; sum += v[t]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (i0 + t < count) local[i0 + t] = run;
        run += v[t];
    }
    if (threadIdx.x == 255) tile_sum[blockIdx.x] = (int64_t)part[255];
}

__global__ __launch_bounds__(256) void enc_scan_sums_kernel(int64_t* __restrict__ tile, int tiles)      // in place; tile[tiles] = the total
{
    __shared__ int64_t part[256];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < tiles; t0 += 256) {
        const int i = t0 + threadIdx.x;
        const int64_t v = i < tiles ? tile[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < tiles) tile[i] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile[tiles] = carry;
}

__device__ __forceinline__ int64_t scan_at(const uint32_t* __restrict__ local, const int64_t* __restrict__ tile_base, int64_t i, int64_t count)
{
    return i >= count ? tile_base[(count + SCAN_TILE - 1) / SCAN_TILE] : tile_base[i / SCAN_TILE] + (int64_t)local[i];
}

// One thread: where every image's bits go in the unstuffed stream (whole chunks each), and whether the stream holds them.
// result = {bytes the files need, first image that does not fit or -1, bytes the unstuffed stream needs, offsets[n + 1]}
__global__ void enc_layout_stream_kernel(const int32_t* __restrict__ block_start, int n, const uint32_t* __restrict__ local,
                                         const int64_t* __restrict__ tile_base, int64_t stream_chunks, EncImage* __restrict__ im,
                                         int32_t* __restrict__ chunk_start, int64_t* __restrict__ result)
{
    if (threadIdx.x | blockIdx.x) return;
    const int64_t count = block_start[n];
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t base = scan_at(local, tile_base, block_start[i], count);
        const int64_t bits = scan_at(local, tile_base, block_start[i + 1], count) - base;
        const int64_t ub = (bits + 7) >> 3, ch = (ub + CHUNK - 1) / CHUNK;
        im[i].bit_base = base; im[i].ubytes = ub; im[i].chunk0 = (int32_t)chunks;
        im[i].fits = chunks + ch <= stream_chunks ? 1 : 0;
        im[i].ff_base = 0; im[i].file_off = 0; im[i].file_bytes = 0;
        chunk_start[i] = (int32_t)chunks;
        chunks += ch;
    }
    chunk_start[n] = (int32_t)chunks;
    result[2] = chunks * CHUNK;
}

// `len` bits at bit `at` of a block's words in LDS, most significant bit first; lanes of the wavefront share words
__device__ __forceinline__ void put_bits(uint32_t* words, int at, uint64_t bits, int len)
{
    int idx = at >> 5, o = at & 31;
    while (len > 0) {
        const int take = min(len, 32 - o);
        const uint32_t piece = (uint32_t)((bits >> (len - take)) & ((1ull << take) - 1ull));
        if (piece) atomicOr(words + idx, piece << (32 - o - take));
        len -= take; o = 0; ++idx;
    }
}

constexpr int EMIT_WORDS = 56;      // 31 bits of the first word's other owner + 1665 + 7 fill bits: 54 words

// A wavefront per block.  The lanes OR their codes into the block's words in LDS; then a lane per word writes them out, byte-swapped (the
// stream is big-endian).  A word of the stream can belong to many blocks (a flat block is 4 to 6 bits), but only a block's first and last
// word can: those two are atomic ORs into the stream, which the call zeroed; the words in between have a single owner and are stored.
__global__ __launch_bounds__(256) void jpeg_emit_kernel(const EncDesc* __restrict__ desc, const int32_t* __restrict__ block_start, int n,
                                                        const int16_t* __restrict__ coef, const uint32_t* __restrict__ huff,
                                                        const uint32_t* __restrict__ local, const int64_t* __restrict__ tile_base,
                                                        const EncImage* __restrict__ im, uint32_t* __restrict__ stream, int64_t stream_words)
{
    __shared__ uint32_t acc[4][EMIT_WORDS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, blk = blockIdx.x * 4 + wave;
    uint32_t* w = acc[wave];
    if (lane < EMIT_WORDS) w[lane] = 0;
    bool live = blk < block_start[n];                        // every condition on `live` is uniform over the wavefront
    int img = 0;
    if (live) {
        img = find_image(block_start, n, blk);
        live = (im[img].fits & 1) != 0;                      // its bits have no place: nothing of it is written
    }
    __syncthreads();
    int64_t at0 = 0;
    int total = 0;
    if (live) {
        const LaneCode C = lane_code(desc[img], coef, huff, blk, lane);
        const int64_t in_image = tile_base[blk / SCAN_TILE] + (int64_t)local[blk] - im[img].bit_base;
        total = C.total;
        if (blk + 1 == block_start[img + 1]) total += (int)((-(in_image + C.total)) & 7);      // the last byte of an image is filled with 1-bits
        live = in_image >= 0 && in_image + total <= im[img].ubytes * 8 && total <= (EMIT_WORDS - 1) * 32;
        if (live) {
            at0 = (int64_t)im[img].chunk0 * CHUNK * 8 + in_image;
            const int o0 = (int)(at0 & 31);
            put_bits(w, o0 + C.off, C.bits, C.len);
            if (lane == 63) put_bits(w, o0 + C.total, (1u << (total - C.total)) - 1u, total - C.total);
        }
    }
    __syncthreads();
    if (live) {
        const int nwords = ((int)(at0 & 31) + total + 31) >> 5;
        const int64_t at = (at0 >> 5) + lane;
        if (lane < nwords && at < stream_words && w[lane]) {
            const uint32_t v = __builtin_bswap32(w[lane]);
            if (lane == 0 || lane == nwords - 1) atomicOr(stream + at, v); else stream[at] = v;
        }
    }
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the bytes of a lane's word that belong to the image and are 0xFF, as a 4-bit mask
__device__ __forceinline__ int ff_mask(uint32_t word, int64_t idx, int64_t ubytes)
{
    int m = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (idx + t < ubytes && ((word >> (8 * t)) & 255u) == 255u) m |= 1 << t;
    return m;
}

__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(const int32_t* __restrict__ chunk_start, int n, const EncImage* __restrict__ im,
                                                           const uint32_t* __restrict__ stream, int64_t stream_chunks, uint32_t* __restrict__ ff)
{
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= stream_chunks) return;
    int count = 0;
    if (c < chunk_start[n]) {
        const int img = find_image(chunk_start, n, (int)c);
        if (im[img].fits & 1)
            count = wave_sum(__popc(ff_mask(stream[c * (CHUNK / 4) + lane], (c - im[img].chunk0) * CHUNK + lane * 4, im[img].ubytes)));
    }
    if (lane == 0) ff[c] = (uint32_t)count;
}

// One thread: the size and place of every file, and whether the output buffer holds it.
__global__ void enc_layout_files_kernel(const int32_t* __restrict__ chunk_start, int n, const uint32_t* __restrict__ local,
                                        const int64_t* __restrict__ tile_base, int64_t stream_chunks, int64_t out_bytes,
                                        EncImage* __restrict__ im, int64_t* __restrict__ result)
{
    if (threadIdx.x | blockIdx.x) return;
    int64_t off = 0, bad = -1;
    for (int i = 0; i < n; ++i) {
        int64_t ffs = 0;
        if (im[i].fits & 1) {
            im[i].ff_base = scan_at(local, tile_base, chunk_start[i], stream_chunks);
            ffs = scan_at(local, tile_base, chunk_start[i + 1], stream_chunks) - im[i].ff_base;
        }
        im[i].file_bytes = ENC_HEADER + im[i].ubytes + ffs + 2;      // a lower bound for an image whose bits had no place
        im[i].file_off = off;
        if ((im[i].fits & 1) && off + im[i].file_bytes <= out_bytes) im[i].fits = 3;
        else if (bad < 0) bad = i;
        result[3 + i] = off;
        off += im[i].file_bytes;
    }
    result[3 + n] = off;
    result[0] = off;
    result[1] = bad;
}

__global__ __launch_bounds__(256) void jpeg_file_kernel(const EncDesc* __restrict__ desc, const int32_t* __restrict__ chunk_start, int n,
                                                        const EncImage* __restrict__ im, const uint32_t* __restrict__ stream, int64_t stream_chunks,
                                                        const uint32_t* __restrict__ local, const int64_t* __restrict__ tile_base,
                                                        uint8_t* __restrict__ out, int64_t out_bytes)
{
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= stream_chunks || c >= chunk_start[n]) return;
    const int img = find_image(chunk_start, n, (int)c);
    const EncImage I = im[img];
    if (I.fits != 3 || I.file_off + I.file_bytes > out_bytes) return;
    uint8_t* file = out + I.file_off;
    if (c == I.chunk0) {
        for (int t = lane; t < ENC_HEADER; t += 64) file[t] = desc[img].header[t];
        if (lane == 0) { file[I.file_bytes - 2] = 0xFF; file[I.file_bytes - 1] = 0xD9; }
    }
    const int64_t idx = (c - I.chunk0) * CHUNK + lane * 4;
    const uint32_t word = stream[c * (CHUNK / 4) + lane];
    const int m = ff_mask(word, idx, I.ubytes);
    int incl = __popc(m);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    int64_t at = ENC_HEADER + idx + (tile_base[c / SCAN_TILE] + (int64_t)local[c] - I.ff_base) + (incl - __popc(m));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (idx + t >= I.ubytes || at >= I.file_bytes - 2) break;
        file[at++] = (uint8_t)(word >> (8 * t));
        if (m & (1 << t)) {
            if (at >= I.file_bytes - 2) break;
            file[at++] = 0;
        }
    }
}

// ---- host: tables and header ------------------------------------------------------------------------------------------------------------
int sampling_factors(int sampling, int& hs, int& vs)       // 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (PIL's numbering)
{
    if (sampling == 0) { hs = 1; vs = 1; } else if (sampling == 1) { hs = 2; vs = 1; } else if (sampling == 2) { hs = 2; vs = 2; } else return 1;
    return 0;
}

// Annex C: canonical codes from the counts; entry[symbol] = code | length << 16
void huff_entries(const uint8_t* counts, const uint8_t* syms, uint32_t* entry)
{
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < counts[len - 1]; ++i) entry[syms[k++]] = code++ | (uint32_t)len << 16;
        code <<= 1;
    }
}

}  // namespace

void jpeg_quant_tables(int quality, uint16_t* qt2x64)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            int v = (kBaseQ[t][k] * scale + 50) / 100;
            v = v < 1 ? 1 : v > 255 ? 255 : v;
            qt2x64[64 * t + kZigzag[k]] = (uint16_t)v;
        }
}

void jpeg_header(int w, int h, int quality, int hs, int vs, uint8_t* out)
{
    static const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    static const uint8_t dc_syms[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    uint16_t qt[128];
    jpeg_quant_tables(quality, qt);
    uint8_t* p = out;
    memcpy(p, app0, sizeof app0); p += sizeof app0;
    for (int t = 0; t < 2; ++t) {
        *p++ = 0xFF; *p++ = 0xDB; *p++ = 0; *p++ = 67; *p++ = (uint8_t)t;
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)qt[64 * t + kZigzag[k]];
    }
    const uint8_t sof[] = {0xFF, 0xC0, 0, 17, 8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3,
                           1, (uint8_t)(hs << 4 | vs), 0, 2, 0x11, 1, 3, 0x11, 1};
    memcpy(p, sof, sizeof sof); p += sizeof sof;
    for (int t = 0; t < 2; ++t) {
        *p++ = 0xFF; *p++ = 0xC4; *p++ = 0; *p++ = 31; *p++ = (uint8_t)t;
        memcpy(p, kDcCounts[t], 16); p += 16;
        memcpy(p, dc_syms, 12); p += 12;
        *p++ = 0xFF; *p++ = 0xC4; *p++ = 0; *p++ = 181; *p++ = (uint8_t)(0x10 | t);
        memcpy(p, kAcCounts[t], 16); p += 16;
        memcpy(p, kAcSyms[t], 162); p += 162;
    }
    memcpy(p, sos, sizeof sos); p += sizeof sos;
    static_assert(sizeof app0 + 2 * 69 + 19 + 2 * (33 + 183) + sizeof sos == ENC_HEADER, "header length");
}

// ---- the object -----------------------------------------------------------------------------------------------------------------------------
struct JpegEncState {
    int device = 0, max_batch = 0;
    int64_t out_bytes = 0, stream_chunks = 0;                // the output buffer; the unstuffed stream in chunks (out_bytes rounded up)
    DevBuf<uint8_t> out;                                     // out_bytes + ENC_GUARD
    DevBuf<uint32_t> stream, ff, ff_local;
    DevBuf<int64_t> ff_tile;
    DevBuf<int16_t> coef;                                    // these four grow with the blocks of a call
    DevBuf<uint32_t> bits, bits_local;
    DevBuf<int64_t> bits_tile;
    DevBuf<uint32_t> huff;
    DevBuf<char> table_dev;                                  // [max_batch] EncDesc, then int32 [max_batch + 1] block starts
    DevBuf<EncImage> im;
    DevBuf<int32_t> chunk_start;
    DevBuf<int64_t> result;                                  // 3 + max_batch + 1
    PinnedBuf<char> table;
    PinnedBuf<int64_t> result_host;
    hipEvent_t uploaded = nullptr, ev[ENC_EVENTS] = {};
    bool used = false, launched = false;
    int n_last = 0;
    std::vector<EncDesc> last;                               // the geometry of the last call (yn_jpeg_enc_coefficients)
    size_t table_bytes() const { return (size_t)max_batch * sizeof(EncDesc) + ((size_t)max_batch + 1) * sizeof(int32_t); }
};

int jpeg_enc_device(const JpegEncState* j) { return j->device; }

void jpeg_enc_destroy(JpegEncState* j)
{
    if (!j) return;
    DeviceScope on(j->device);
    if (j->launched) (void)hipDeviceSynchronize();
    if (j->uploaded) (void)hipEventDestroy(j->uploaded);
    for (hipEvent_t e : j->ev)
        if (e) (void)hipEventDestroy(e);
    delete j;
}

int jpeg_enc_create(int device, int max_batch, int64_t stream_bytes, JpegEncState** out, std::string& err)
{
    if (max_batch < 1 || max_batch > 1024) { err = "yn_jpeg_enc_create: max_batch " + std::to_string(max_batch) + " outside 1..1024"; return 1; }
    if (stream_bytes < 1024 || stream_bytes > ((int64_t)1 << 32)) { err = "yn_jpeg_enc_create: stream_bytes " + std::to_string(stream_bytes) + " outside 1024..2^32"; return 1; }
    auto* j = new JpegEncState;
    j->device = device; j->max_batch = max_batch;
    j->out_bytes = stream_bytes;
    j->stream_chunks = (stream_bytes + CHUNK - 1) / CHUNK;
    const size_t tiles = (size_t)((j->stream_chunks + SCAN_TILE - 1) / SCAN_TILE);
    std::vector<uint32_t> huff(2 * HUFF_STRIDE, 0u);
    static const uint8_t dc_syms[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (int t = 0; t < 2; ++t) {
        huff_entries(kDcCounts[t], dc_syms, huff.data() + t * HUFF_STRIDE);
        huff_entries(kAcCounts[t], kAcSyms[t], huff.data() + t * HUFF_STRIDE + 12);
    }
    int r = j->out.reserve((size_t)stream_bytes + ENC_GUARD);
    if (!r) r = j->stream.reserve((size_t)j->stream_chunks * (CHUNK / 4));
    if (!r) r = j->ff.reserve((size_t)j->stream_chunks);
    if (!r) r = j->ff_local.reserve((size_t)j->stream_chunks);
    if (!r) r = j->ff_tile.reserve(tiles + 1);
    if (!r) r = j->huff.reserve(huff.size());
    if (!r) r = j->table_dev.reserve(j->table_bytes());
    if (!r) r = j->im.reserve((size_t)max_batch);
    if (!r) r = j->chunk_start.reserve((size_t)max_batch + 1);
    if (!r) r = j->result.reserve((size_t)max_batch + 4);
    if (!r) r = j->table.reserve(j->table_bytes());
    if (!r) r = j->result_host.reserve((size_t)max_batch + 4);
    if (!r) r = (int)hipEventCreate(&j->uploaded);
    for (hipEvent_t& e : j->ev)
        if (!r) r = (int)hipEventCreate(&e);
    if (!r) r = (int)hipMemcpy(j->huff.get(), huff.data(), huff.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (!r) r = (int)hipMemset(j->out.get() + stream_bytes, 0xA5, ENC_GUARD);
    if (r) {
        (void)hipGetLastError();
        err = std::string("yn_jpeg_enc_create: ") + hipGetErrorString((hipError_t)r) + " (" + std::to_string(stream_bytes) + " stream bytes: twice that on the device)";
        jpeg_enc_destroy(j);
        return 1;
    }
    *out = j;
    return 0;
}

int jpeg_encode_batch(JpegEncState* j, hipStream_t st, int n, const uint8_t* const* frames, const int32_t* geom, int quality, int sampling, std::string& err)
{
    const std::string me = "yn_jpeg_encode_batch: ";
    if (n < 0) { err = me + "negative batch"; return 1; }
    if (n == 0) { j->n_last = 0; j->last.clear(); return 0; }       // a refused call below leaves the previous batch fetchable
    if (!frames || !geom) { err = me + "null argument"; return 1; }
    if (n > j->max_batch) { err = me + std::to_string(n) + " images, the encoder was made for " + std::to_string(j->max_batch); return 1; }
    if (quality < 1 || quality > 100) { err = me + "quality " + std::to_string(quality) + " outside 1..100"; return 1; }
    int hs = 0, vs = 0;
    if (sampling_factors(sampling, hs, vs)) { err = me + "unknown sampling " + std::to_string(sampling) + " (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)"; return 1; }
    uint16_t qt[128];
    jpeg_quant_tables(quality, qt);
    std::vector<EncDesc> desc((size_t)n);
    std::vector<int32_t> start((size_t)n + 1);
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const int w = geom[2 * i], h = geom[2 * i + 1];
        if (!frames[i]) { err = me + "image " + std::to_string(i) + " has no frame"; return 1; }
        if (w < 1 || w > 16384 || h < 1 || h > 16384) {
            err = me + "image " + std::to_string(i) + " is " + std::to_string(w) + " x " + std::to_string(h) + ": a side outside 1..16384";
            return 1;
        }
        EncDesc& D = desc[(size_t)i];
        memset(&D, 0, sizeof D);
        D.frame = frames[i];
        D.w = w; D.h = h; D.hs = hs; D.vs = vs;
        D.mw = (w + 8 * hs - 1) / (8 * hs);
        D.bpm = hs * vs + 2;
        D.wib = (w + 7) / 8; D.hib = (h + 7) / 8;
        for (int k = 0; k < 128; ++k) D.q8[k / 64][k % 64] = (uint16_t)(8 * qt[k]);
        jpeg_header(w, h, quality, hs, vs, D.header);
        const int64_t mh = (h + 8 * vs - 1) / (8 * vs);
        if (blocks + D.mw * mh * D.bpm > ENC_MAX_BLOCKS) {
            err = me + "image " + std::to_string(i) + " brings the batch to " + std::to_string(blocks + D.mw * mh * D.bpm) + " blocks: the worst case of its unstuffed stream (209 bytes a block) cannot be staged, the limit is " +
                  std::to_string(ENC_MAX_BLOCKS) + " blocks";
            return 1;
        }
        D.block0 = (int32_t)blocks;
        start[(size_t)i] = (int32_t)blocks;
        blocks += D.mw * mh * D.bpm;
    }
    start[(size_t)n] = (int32_t)blocks;
    const size_t tiles = (size_t)((blocks + SCAN_TILE - 1) / SCAN_TILE);
    hipError_t e = hipSuccess;
    j->n_last = 0;                                           // from here on the previous batch's results are overwritten
    j->last.clear();
    // The per-block buffers grow together, by doubling from 2^14 blocks; the tile sums follow the capacity (one per SCAN_TILE blocks and
    // one for the total), so a later call that fills the capacity finds room for every tile.
    size_t cap = j->bits.cap() ? j->bits.cap() : (size_t)1 << 14;
    while (cap < (size_t)blocks) cap *= 2;
    if (cap > j->bits.cap() || cap * 64 > j->coef.cap() || cap > j->bits_local.cap() || cap / SCAN_TILE + 1 > j->bits_tile.cap()) {
        e = hipStreamSynchronize(st);                        // earlier work on the stream may still read the old buffers
        int r = (int)e;
        if (!r) r = j->coef.reserve(cap * 64);
        if (!r) r = j->bits.reserve(cap);
        if (!r) r = j->bits_local.reserve(cap);
        if (!r) r = j->bits_tile.reserve(cap / SCAN_TILE + 1);
        if (r) {
            (void)hipGetLastError();
            j->coef.reset(); j->bits.reset(); j->bits_local.reset(); j->bits_tile.reset();
            err = me + hipGetErrorString((hipError_t)r) + " (the coefficients of " + std::to_string(blocks) + " blocks cannot be staged)";
            return 1;
        }
    }
    if (j->used) e = hipEventSynchronize(j->uploaded);       // the previous upload must have left the pinned table
    if (e != hipSuccess) { err = me + hipGetErrorString(e); return 1; }
    memcpy(j->table.get(), desc.data(), (size_t)n * sizeof(EncDesc));
    memcpy(j->table.get() + (size_t)j->max_batch * sizeof(EncDesc), start.data(), ((size_t)n + 1) * sizeof(int32_t));
    const EncDesc* ddesc = reinterpret_cast<const EncDesc*>(j->table_dev.get());
    const int32_t* dstart = reinterpret_cast<const int32_t*>(j->table_dev.get() + (size_t)j->max_batch * sizeof(EncDesc));
    // The chunks this call can touch: its worst case (209 bytes a block, whole chunks per image) or the whole stream, whichever is less.
    // Clearing, the 0xFF count, its scan and the file kernel run over these only, so a small call on a grown object stays small; whether an
    // image fits is still decided against the whole capacity.
    const int64_t worst = (blocks * 209 + CHUNK - 1) / CHUNK + n;
    const int64_t sc = worst < j->stream_chunks ? worst : j->stream_chunks, words = sc * (CHUNK / 4);
    const unsigned per_block = (unsigned)((blocks + 3) / 4), per_chunk = (unsigned)((sc + 3) / 4);
    const int ff_tiles = (int)((sc + SCAN_TILE - 1) / SCAN_TILE);
    int k = 0;
    auto mark = [&]() { if (e == hipSuccess) e = hipGetLastError(); if (e == hipSuccess) e = hipEventRecord(j->ev[k++], st); };
    mark();
    if (e == hipSuccess) e = hipMemcpyAsync(j->table_dev.get(), j->table.get(), j->table_bytes(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(j->uploaded, st);
    if (e == hipSuccess) e = hipMemsetAsync(j->stream.get(), 0, (size_t)words * sizeof(uint32_t), st);      // cleared on every call
    if (e != hipSuccess) { err = me + hipGetErrorString(e); return 1; }
    j->used = true;
    j->launched = true;
    mark();
    hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, st, ddesc, dstart, n, j->coef.get());
    mark();
    hipLaunchKernelGGL(jpeg_bits_kernel, dim3(per_block), dim3(256), 0, st, ddesc, dstart, n, j->coef.get(), j->huff.get(), j->bits.get());
    mark();
    hipLaunchKernelGGL(enc_scan_tiles_kernel, dim3((unsigned)tiles), dim3(256), 0, st, j->bits.get(), blocks, j->bits_local.get(), j->bits_tile.get());
    mark();
    hipLaunchKernelGGL(enc_scan_sums_kernel, dim3(1), dim3(256), 0, st, j->bits_tile.get(), (int)tiles);
    hipLaunchKernelGGL(enc_layout_stream_kernel, dim3(1), dim3(64), 0, st, dstart, n, j->bits_local.get(), j->bits_tile.get(), j->stream_chunks, j->im.get(),
                       j->chunk_start.get(), j->result.get());
    mark();
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3(per_block), dim3(256), 0, st, ddesc, dstart, n, j->coef.get(), j->huff.get(), j->bits_local.get(),
                       j->bits_tile.get(), j->im.get(), j->stream.get(), words);
    mark();
    hipLaunchKernelGGL(jpeg_ffcount_kernel, dim3(per_chunk), dim3(256), 0, st, j->chunk_start.get(), n, j->im.get(), j->stream.get(), sc, j->ff.get());
    mark();
    hipLaunchKernelGGL(enc_scan_tiles_kernel, dim3((unsigned)ff_tiles), dim3(256), 0, st, j->ff.get(), sc, j->ff_local.get(), j->ff_tile.get());
    mark();
    hipLaunchKernelGGL(enc_scan_sums_kernel, dim3(1), dim3(256), 0, st, j->ff_tile.get(), ff_tiles);
    hipLaunchKernelGGL(enc_layout_files_kernel, dim3(1), dim3(64), 0, st, j->chunk_start.get(), n, j->ff_local.get(), j->ff_tile.get(), sc, j->out_bytes,
                       j->im.get(), j->result.get());
    mark();
    hipLaunchKernelGGL(jpeg_file_kernel, dim3(per_chunk), dim3(256), 0, st, ddesc, j->chunk_start.get(), n, j->im.get(), j->stream.get(), sc,
                       j->ff_local.get(), j->ff_tile.get(), j->out.get(), j->out_bytes);
    mark();
    if (e != hipSuccess) { err = me + hipGetErrorString(e); return 1; }
    j->n_last = n;
    j->last = std::move(desc);
    return 0;
}

int jpeg_encode_fetch(JpegEncState* j, hipStream_t st, int64_t* offsets, uint8_t* files, int64_t cap, std::string& err)
{
    const std::string me = "yn_jpeg_encode_fetch: ";
    if (!offsets) { err = me + "null argument"; return 1; }
    const int n = j->n_last;
    offsets[0] = 0;
    if (n == 0) return 0;
    hipError_t e = hipMemcpyAsync(j->result_host.get(), j->result.get(), ((size_t)n + 4) * sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { err = me + hipGetErrorString(e); return 1; }
    const int64_t* r = j->result_host.get();
    memcpy(offsets, r + 3, ((size_t)n + 1) * sizeof(int64_t));
    if (r[1] >= 0) {
        err = me + "image " + std::to_string(r[1]) + " does not fit: the batch needs " + std::to_string(r[0]) + " output bytes and " + std::to_string(r[2]) +
              " stream bytes, the encoder has " + std::to_string(j->out_bytes);
        return 1;
    }
    if (!files || r[0] > cap) {
        int bad = 0;
        while (bad + 1 < n && offsets[bad + 1] <= cap) ++bad;
        err = me + "image " + std::to_string(bad) + " does not fit the caller's buffer: the batch needs " + std::to_string(r[0]) + " bytes, it has " + std::to_string(files ? cap : 0);
        return 1;
    }
    e = hipMemcpyAsync(files, j->out.get(), (size_t)r[0], hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { err = me + hipGetErrorString(e); return 1; }
    return 0;
}

// image i's quantised coefficients in yn_jpeg_coefficients' layout: natural order, per component, block-row-major over the MCU-padded grid
int jpeg_enc_coefficients(JpegEncState* j, hipStream_t st, int i, int16_t* host, int64_t cap, std::string& err)
{
    const std::string me = "yn_jpeg_enc_coefficients: ";
    if (!host) { err = me + "null argument"; return 1; }
    if (i < 0 || i >= j->n_last) { err = me + "image " + std::to_string(i) + " is not in the last batch of " + std::to_string(j->n_last); return 1; }
    const EncDesc& D = j->last[(size_t)i];
    const int nl = D.hs * D.vs, mw = D.mw, mh = (D.h + 8 * D.vs - 1) / (8 * D.vs);
    const int64_t blocks = (int64_t)mw * mh * D.bpm;
    if (blocks * 64 > cap) { err = me + "image " + std::to_string(i) + " needs " + std::to_string(blocks * 64) + " int16 elements, the buffer has " + std::to_string(cap); return 1; }
    std::vector<int16_t> zz((size_t)blocks * 64);
    hipError_t e = hipMemcpyAsync(zz.data(), j->coef.get() + (int64_t)D.block0 * 64, zz.size() * sizeof(int16_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { err = me + hipGetErrorString(e); return 1; }
    const int64_t comp_off[3] = {0, (int64_t)mw * mh * nl, (int64_t)mw * mh * (nl + 1)};
    for (int64_t b = 0; b < blocks; ++b) {
        const int64_t mcu = b / D.bpm;
        const int k = (int)(b % D.bpm), my = (int)(mcu / mw), mx = (int)(mcu % mw);
        int64_t dst;
        if (k < nl) dst = ((int64_t)(my * D.vs + k / D.hs) * (mw * D.hs) + mx * D.hs + k % D.hs);
        else dst = comp_off[k - nl + 1] + mcu;
        for (int p = 0; p < 64; ++p) host[dst * 64 + kZigzag[p]] = zz[(size_t)b * 64 + p];
    }
    return 0;
}

int jpeg_enc_guard(JpegEncState* j, hipStream_t st, uint8_t* host64, std::string& err)
{
    hipError_t e = hipMemcpyAsync(host64, j->out.get() + j->out_bytes, ENC_GUARD, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { err = std::string("yn_jpeg_enc_guard: ") + hipGetErrorString(e); return 1; }
    return 0;
}

int jpeg_enc_timing(JpegEncState* j, float* ms10, std::string& err)
{
    for (int k = 0; k < ENC_EVENTS - 1; ++k) ms10[k] = 0.0f;
    if (j->n_last == 0) return 0;
    hipError_t e = hipEventSynchronize(j->ev[ENC_EVENTS - 1]);
    for (int k = 0; k < ENC_EVENTS - 1 && e == hipSuccess; ++k) e = hipEventElapsedTime(&ms10[k], j->ev[k], j->ev[k + 1]);
    if (e != hipSuccess) { err = std::string("yn_jpeg_enc_timing: ") + hipGetErrorString(e); return 1; }
    return 0;
}

}  // namespace ynk
