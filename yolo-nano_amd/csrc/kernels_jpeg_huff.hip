// kernels_jpeg_huff.hip — the Huffman stage of the JPEG decode on the device (opt-in, yn_jpeg_entropy).  The state stays in
// JpegState (kernels_jpeg.hip), which fills the descriptors and launches the four kernels through jpeg_huff_launch():
//   jpeg_huff_first_kernel   a thread per subsequence of the chunk: round 1 of the subsequence fixed point (yn_jpeg_huff.h), in which every
//                            subsequence decodes from its own first bit with u = 0, k = 0.
//   jpeg_huff_sync_kernel    one workgroup per file: the further rounds, separated by workgroup barriers, never more than max_rounds in
//                            all; then the exclusive prefix sum of the blocks each subsequence finished and the
//                            checks that place every subsequence where entropy_decode would have it.  Writes the file's result word.
//   jpeg_huff_write_kernel   a thread per subsequence of the files whose result word is 0: decodes once more from the verified state and
//                            stores AC values at their natural index and DC differences at 0, into the cleared coefficient buffer.
//   jpeg_huff_dc_kernel      one workgroup per such file: DC differences -> DC values, a segmented inclusive sum per component in decode
//                            order that starts again at every restart segment, in 16-bit wrap-around arithmetic as pred[] on the host.
// The output is the int16 coefficient buffer jpeg_idct_kernel reads, in the layout entropy_decode writes.
//
// Nothing is addressed by data, so garbage in a file gives garbage coefficients or a result word that sends the file to the host, never a
// fault: scan words are read below the file's word count only (Stream::word), table lookups are masked to the table (decode_span), and a
// coefficient goes to block_offset(g) + zz[k & 63] only for 0 <= g < the file's block count (CoefSink), g being a COUNT of
// finished blocks.  Descriptors, segment and workgroup tables come from the host's parser, not from the scan.
#include <hip/hip_runtime.h>

#include "yn_internal.h"
#include "yn_jpeg_huff.h"

namespace ynk {

namespace {

using namespace ynhuff;

__device__ const uint8_t ZZ_dev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};      // copied to LDS by the write kernel

constexpr int SYNC_THREADS = 1024, WRITE_THREADS = 256, TABLE_WORDS = (int)(sizeof(Table) / 4);

__device__ __forceinline__ void load_tables(Table* sh, const Table* __restrict__ all, const FileDesc& F, int t, int nt)
{
    const int n = 2 * F.nc * TABLE_WORDS;
    for (int i = t; i < n; i += nt) {
        const int tb = i / TABLE_WORDS, w = i - tb * TABLE_WORDS;
        reinterpret_cast<uint32_t*>(&sh[tb])[w] = reinterpret_cast<const uint32_t*>(&all[F.tab[tb]])[w];
    }
}

__device__ __forceinline__ Job make_job(const FileDesc& F, const Table* tabs, const Segment* segs, const uint8_t* scan, uint64_t* start, uint64_t* end,
                                        int32_t* nblk, int sb)
{
    Job J;
    J.S.words = reinterpret_cast<const uint32_t*>(scan + F.scan_off);
    J.S.nwords = (F.scan_bytes + 3) >> 2;
    J.tabs = tabs;
    J.segs = segs + F.seg0;
    J.nseg = F.nseg; J.nsub = F.nsub; J.sb = sb;
    J.scan_bits = F.scan_bytes * 8;
    J.U = F.G.U; J.L = F.G.L; J.blocks = F.G.blocks;
    J.start = start + F.sub0; J.end = end + F.sub0; J.nblk = nblk + F.sub0;
    return J;
}

// inclusive sum over the workgroup's SYNC_THREADS values (Hillis-Steele through LDS, sh[2 * SYNC_THREADS])
__device__ __forceinline__ int32_t wg_inclusive(int32_t v, int32_t* sh, int t)
{
    int32_t* a = sh;
    int32_t* b = sh + SYNC_THREADS;
    a[t] = v;
    __syncthreads();
    for (int d = 1; d < SYNC_THREADS; d <<= 1) {
        int32_t x = a[t];
        if (t >= d) x += a[t - d];
        b[t] = x;
        __syncthreads();
        int32_t* s = a; a = b; b = s;
    }
    const int32_t r = a[t];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(SYNC_THREADS) void jpeg_huff_sync_kernel(const FileDesc* __restrict__ files, const Segment* __restrict__ segs,
                                                                      const Table* __restrict__ tables, const uint8_t* __restrict__ scan, uint64_t* start,
                                                                      uint64_t* end, int32_t* nblk, int32_t* __restrict__ base, FileResult* __restrict__ result,
                                                                      int sb, int max_rounds)
{
    __shared__ Table tabs[6];
    __shared__ int32_t sums[2 * SYNC_THREADS];
    const int t = threadIdx.x;
    const FileDesc& F = files[blockIdx.x];
    load_tables(tabs, tables, F, t, SYNC_THREADS);
    const Job J = make_job(F, tabs, segs, scan, start, end, nblk, sb);
    __syncthreads();
    // Jacobi rounds: every subsequence first takes its predecessor's end state of the round before, then the changed ones decode.  The
    // barriers order the two (a workgroup's global writes are visible to it after __syncthreads).  Round 1, in which every subsequence
    // decodes, is jpeg_huff_first_kernel's: it has the whole device, this kernel one compute unit per file.
    int rounds = 1, decodes = 0, flag = 0;
    for (;;) {
        int dirty = 0;
        for (int32_t i = t; i < J.nsub; i += SYNC_THREADS) dirty |= sync_pull(J, i) ? 1 : 0;
        if (!__syncthreads_or(dirty)) break;
        if (rounds == max_rounds) { flag = FLAG_ROUNDS; break; }
        ++rounds;
        for (int32_t i = t; i < J.nsub; i += SYNC_THREADS) decodes += sync_decode(J, i);
        __syncthreads();
    }
    // place: blocks before each subsequence, then the checks
    int32_t carry = 0;
    for (int32_t c0 = 0; c0 < J.nsub; c0 += SYNC_THREADS) {
        const int32_t i = c0 + t;
        const int32_t v = i < J.nsub ? J.nblk[i] : 0;
        const int32_t incl = wg_inclusive(v, sums, t);
        const int32_t before = (int32_t)((uint32_t)carry + (uint32_t)incl - (uint32_t)v);
        if (i < J.nsub) {
            base[F.sub0 + i] = before;
            flag |= verify(J, i, before);
        }
        sums[t] = incl;
        __syncthreads();
        carry = (int32_t)((uint32_t)carry + (uint32_t)sums[SYNC_THREADS - 1]);
        __syncthreads();
    }
    flag = __syncthreads_or(flag);
    sums[t] = decodes;
    __syncthreads();
    if (t == 0) {
        int32_t all = 0;
        for (int i = 0; i < SYNC_THREADS; ++i) all += sums[i];
        FileResult r;
        r.flag = flag; r.rounds = rounds; r.decodes = all + J.nsub; r.nsub = J.nsub;
        result[blockIdx.x] = r;
    }
}

__device__ __forceinline__ int find_file(const int32_t* start, int n, int v)       // the largest i < n with start[i] <= v
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// round 1 of the fixed point, a thread per subsequence of the chunk: every subsequence decodes from its own first bit
__global__ __launch_bounds__(WRITE_THREADS) void jpeg_huff_first_kernel(const FileDesc* __restrict__ files, const int32_t* __restrict__ wg_start, int n,
                                                                        const Segment* __restrict__ segs, const Table* __restrict__ tables,
                                                                        const uint8_t* __restrict__ scan, uint64_t* start, uint64_t* end, int32_t* nblk, int sb)
{
    __shared__ Table tabs[6];
    const int t = threadIdx.x;
    const int f = find_file(wg_start, n, (int)blockIdx.x);
    const FileDesc& F = files[f];
    load_tables(tabs, tables, F, t, WRITE_THREADS);
    __syncthreads();
    const Job J = make_job(F, tabs, segs, scan, start, end, nblk, sb);
    const int32_t i = ((int32_t)blockIdx.x - wg_start[f]) * WRITE_THREADS + t;
    if (i >= J.nsub) return;
    sync_init(J, i);
    (void)sync_decode(J, i);
}

__global__ __launch_bounds__(WRITE_THREADS) void jpeg_huff_write_kernel(const FileDesc* __restrict__ files, const int32_t* __restrict__ wg_start, int n,
                                                                        const Segment* __restrict__ segs, const Table* __restrict__ tables,
                                                                        const uint8_t* __restrict__ scan, uint64_t* start, uint64_t* end, int32_t* nblk,
                                                                        const int32_t* __restrict__ base, const FileResult* __restrict__ result, int sb,
                                                                        int16_t* __restrict__ coef)
{
    __shared__ Table tabs[6];
    __shared__ Geometry geo;
    __shared__ uint8_t zz[64];
    const int t = threadIdx.x;
    const int f = find_file(wg_start, n, (int)blockIdx.x);
    if (result[f].flag) return;                            // the host decodes this file: its coefficients stay cleared
    const FileDesc& F = files[f];
    load_tables(tabs, tables, F, t, WRITE_THREADS);
    if (t == 0) geo = F.G;
    if (t < 64) zz[t] = ZZ_dev[t];
    __syncthreads();
    const Job J = make_job(F, tabs, segs, scan, start, end, nblk, sb);
    const int32_t i = ((int32_t)blockIdx.x - wg_start[f]) * WRITE_THREADS + t;
    if (i >= J.nsub) return;
    CoefSink sink;
    sink.coef = coef; sink.G = &geo; sink.zz = zz; sink.before = base[F.sub0 + i]; sink.cur = -1; sink.blk = nullptr;
    write_span(J, i, sink);
}

// (flag, value) pairs under "a flagged element starts again": the segmented inclusive sum of 16-bit values
__global__ __launch_bounds__(SYNC_THREADS) void jpeg_huff_dc_kernel(const FileDesc* __restrict__ files, const FileResult* __restrict__ result,
                                                                    int16_t* __restrict__ coef)
{
    __shared__ uint32_t sh[2 * SYNC_THREADS];              // value | flag << 16
    const int t = threadIdx.x;
    if (result[blockIdx.x].flag) return;
    const FileDesc& F = files[blockIdx.x];
    const Geometry& G = F.G;
    const int32_t mcus = G.blocks / G.U;
    for (int c = 0; c < F.nc; ++c) {
        const int32_t per = c == 0 ? G.L : 1, count = mcus * per;
        uint32_t carry = 0;
        for (int32_t c0 = 0; c0 < count; c0 += SYNC_THREADS) {
            const int32_t j = c0 + t;
            int16_t* at = nullptr;
            uint32_t x = 0;
            if (j < count) {
                const int32_t mcu = j / per, sub = j - mcu * per;
                const int32_t g = mcu * G.U + (c == 0 ? sub : G.L + c - 1);
                at = coef + block_offset(G, g);
                const bool head = sub == 0 && (G.restart ? mcu % G.restart == 0 : mcu == 0);
                x = (uint32_t)(uint16_t)*at | (head ? 1u << 16 : 0u);
            }
            uint32_t* a = sh;
            uint32_t* b = sh + SYNC_THREADS;
            a[t] = x;
            __syncthreads();
            for (int d = 1; d < SYNC_THREADS; d <<= 1) {
                uint32_t y = a[t];
                if (t >= d && !(y >> 16)) {
                    const uint32_t z = a[t - d];
                    y = ((y + z) & 0xffffu) | (z & 0x10000u);
                }
                b[t] = y;
                __syncthreads();
                uint32_t* s = a; a = b; b = s;
            }
            uint32_t y = a[t];
            if (!(y >> 16)) y = (y + carry) & 0xffffu;     // no segment began in this tile before j: the sum continues
            const uint32_t last = a[SYNC_THREADS - 1];
            __syncthreads();
            carry = (last >> 16) ? (last & 0xffffu) : ((last + carry) & 0xffffu);
            if (at) *at = (int16_t)(uint16_t)(y & 0xffffu);
        }
    }
}

}  // namespace

void jpeg_huff_launch(const JpegHuffArgs& a, hipStream_t st, hipEvent_t after_first, hipEvent_t after_sync, hipEvent_t after_write)
{
    const FileDesc* files = static_cast<const FileDesc*>(a.files);
    const Segment* segs = static_cast<const Segment*>(a.segs);
    const Table* tables = static_cast<const Table*>(a.tables);
    FileResult* result = static_cast<FileResult*>(a.result);
    hipLaunchKernelGGL(jpeg_huff_first_kernel, dim3((unsigned)a.write_wgs), dim3(WRITE_THREADS), 0, st, files, a.wg_start, a.nfiles, segs, tables, a.scan,
                       a.start, a.end, a.nblk, a.sb);
    if (after_first) (void)hipEventRecord(after_first, st);
    hipLaunchKernelGGL(jpeg_huff_sync_kernel, dim3((unsigned)a.nfiles), dim3(SYNC_THREADS), 0, st, files, segs, tables, a.scan, a.start, a.end, a.nblk, a.base,
                       result, a.sb, a.max_rounds);
    if (after_sync) (void)hipEventRecord(after_sync, st);
    hipLaunchKernelGGL(jpeg_huff_write_kernel, dim3((unsigned)a.write_wgs), dim3(WRITE_THREADS), 0, st, files, a.wg_start, a.nfiles, segs, tables, a.scan,
                       a.start, a.end, a.nblk, a.base, result, a.sb, a.coef);
    if (after_write) (void)hipEventRecord(after_write, st);
    hipLaunchKernelGGL(jpeg_huff_dc_kernel, dim3((unsigned)a.nfiles), dim3(SYNC_THREADS), 0, st, files, result, a.coef);
}

int jpeg_huff_write_threads() { return WRITE_THREADS; }

}  // namespace ynk
