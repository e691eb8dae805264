// kernels_kmeans.hip — anchor-box k-means (kmeans_anchor.py: iou :35, init_centroids :58, do_kmeans :95, anchor_box_kmeans :126) with
// exact sums.  Built with -ffp-contract=off: every distance is the reference's float64 operation sequence, bit for bit.
//
// Boxes are (w, h) float64 pairs centred at the origin, 1 <= w, h < 65536.  On that domain
//   - w = m * 2^(e-52) with a 53-bit m and e = 0..15, so w * 2^52 is an integer below 2^68;
//   - a distance 1 - IoU lies in [0, 1] and is an integer multiple of 2^-53 (IoU >= 1/2: the subtraction is exact and IoU itself is such a
//     multiple; IoU < 1/2: the result lies in (1/2, 1], where doubles are 2^-53 apart), so d * 2^53 is an integer <= 2^53.
// Every sum is therefore an integer sum: associative, independent of box order, grid and arrival order.  One thread rounds the wide
// integer to the nearest-even double at the end, which is the correctly rounded exact sum (what math.fsum returns).
//
// Limb layout of the iteration pass.  A box's w * 2^52 is split into lo = bits 0..46 and hi = bits 47..67; a workgroup adds both, and
// the group's count, into 64-bit LDS accumulators.  A workgroup sees at most 2^16 boxes (grid-stride over KM_PASS_BLOCKS = 256
// workgroups of 1024 threads, N <= 2^24), so the lo accumulator stays below 2^47 * 2^16 = 2^63.  THIS is what bounds N: 256 * 2^16 =
// 2^24.  The distance's d * 2^53 goes into two 32-bit limbs per thread, reduced in the wave, then in LDS.  Each workgroup stores its
// 5 K + 2 accumulators into its own slab row (8-byte agent-scope atomic stores); the workgroup that draws the last ticket reads all
// rows (agent-scope atomic loads), folds them in 32-bit limbs into 64-bit LDS accumulators (at most 256 terms below 2^32 each), builds
// the 128-bit totals, rounds, divides and decides.  No accumulator outlives a launch, so none needs zeroing; the ticket is put back to
// 0, and its 16-byte block is also zeroed by a memset in front of every pass or batch of passes.  The fold is one workgroup's work and bound by the latency of its loads: hence few, large workgroups (256 rows, 1024 threads with
// 16 loads in flight each) rather than many small ones - measured, 512 x 256 threads cost 12 us more per pass at K = 9.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "yn_internal.h"
#include "yn_eval_shared.h"

namespace ynk {

namespace {

typedef unsigned long long u64;

constexpr int KM_MAX_K = 32;
constexpr int64_t KM_MAX_N = 1ll << 24;
constexpr int KM_THREADS = 256;
constexpr int KM_PASS_THREADS = 1024;
constexpr int KM_PASS_BLOCKS = 256;            // see the limb layout above
constexpr int KM_FOLD = 16;                    // slab words a thread of the last workgroup has in flight
constexpr int KM_COLS = 5;                     // per group: count, w lo, w hi, h lo, h hi
constexpr int KM_CHUNK = 1024;                 // boxes per workgroup of the seeding pass: 1024 * 2^53 = 2^63 fits a u64
constexpr int KM_BATCH = 32;                   // passes enqueued per host read of `done`
constexpr int KM_MODE_SINGLE = 0, KM_MODE_RUN = 1;

// the device-side record of one clustering.  The first 16 bytes are the ticket's block, zeroed by a memset in front of every batch of
// launches (an aborted launch must not poison the next); a run zeroes the first 32 (its counters too)
struct KmDev {
    uint32_t ticket, tpad[3];                  // put back to zero by the last workgroup of every launch as well
    int32_t it;                                // passes since the run began (the reference's `iterations`)
    int32_t done;                              // the run has stopped: later passes are no-ops
    int32_t rpad[2];
    int32_t slot;                              // cent[slot] / count[slot] / loss[slot] are current
    int32_t k, bad, pad0;
    double old_loss, sum_d;
    double loss[2];
    double cent[2][KM_MAX_K][2];
    int64_t count[2][KM_MAX_K];
    int32_t picked[KM_MAX_K];
};

struct u128 { u64 hi, lo; };

__device__ __forceinline__ void add128(u128& a, u64 hi, u64 lo)
{
    const u64 s = a.lo + lo;
    a.hi += hi + (s < lo ? 1ull : 0ull);
    a.lo = s;
}
__device__ __forceinline__ void add_shifted(u128& a, u64 v, int sh)         // a += v << sh, 0 <= sh < 64
{
    add128(a, sh ? v >> (64 - sh) : 0ull, v << sh);
}
__device__ __forceinline__ bool gt128(const u128& a, const u128& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }

// the double nearest to v * 2^e2, ties to even
__device__ double round128(u128 v, int e2)
{
    if (!v.hi && !v.lo) return 0.0;
    const int p = v.hi ? 127 - __clzll((long long)v.hi) : 63 - __clzll((long long)v.lo);   // the top set bit
    if (p <= 52) return ldexp((double)v.lo, e2);
    const int sh = p - 52;                                                                 // 1..75
    u64 q = sh >= 64 ? v.hi >> (sh - 64) : (v.lo >> sh) | (v.hi << (64 - sh));             // the 53 leading bits
    const int hb = sh - 1;                                                                 // the half bit
    const bool half = hb >= 64 ? (v.hi >> (hb - 64)) & 1ull : (v.lo >> hb) & 1ull;
    bool sticky;
    if (hb >= 64) sticky = v.lo != 0ull || (hb > 64 && (v.hi & ((1ull << (hb - 64)) - 1ull)) != 0ull);
    else sticky = hb > 0 && (v.lo & ((1ull << hb) - 1ull)) != 0ull;
    if (half && (sticky || (q & 1ull))) ++q;                                               // q == 2^53 is still exact
    return ldexp((double)q, sh + e2);
}

// 1 - IoU of a box (w, h; s1 = w * h) and a centroid (cw, ch; s2 = cw * ch), iou() :35-55.  With both centred, min(xmax) - max(xmin)
// is min(w, cw) / 2 + min(w, cw) / 2 = min(w, cw) exactly.
__device__ __forceinline__ double distance(double w, double h, double s1, double cw, double ch, double s2)
{
    const double iw = w < cw ? w : cw, ih = h < ch ? h : ch;
    const double I = iw * ih;
    return 1.0 - I / (s1 + s2 - I);
}

__device__ __forceinline__ u64 scaled53(double d) { return (u64)(d * 9007199254740992.0); }   // d * 2^53, exact on [0, 1]

__device__ __forceinline__ u64 wave_sum(u64 v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ bool in_domain(double v) { return v >= 1.0 && v < 65536.0; }     // false for NaN

// ---- boxes in: copy into the object's buffer and count what lies outside the domain ------------------------------------------------
__global__ __launch_bounds__(KM_THREADS) void km_set_boxes_kernel(const double2* __restrict__ src, double2* __restrict__ dst, int n, KmDev* st)
{
    int bad = 0;
    for (int i = blockIdx.x * KM_THREADS + threadIdx.x; i < n; i += gridDim.x * KM_THREADS) {
        const double2 b = src[i];
        dst[i] = b;
        bad += (in_domain(b.x) && in_domain(b.y)) ? 0 : 1;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&st->bad, bad);
}

// ---- one do_kmeans (:95-123) ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KM_PASS_THREADS) void km_pass_kernel(const double2* __restrict__ boxes, int n, KmDev* st, u64* slab, int mode,
                                                             double loss_convergence, int iters)
{
    __shared__ double cw[KM_MAX_K], ch[KM_MAX_K], cs[KM_MAX_K];
    __shared__ u64 acc[KM_MAX_K * KM_COLS + 2];
    __shared__ u64 fold[(KM_MAX_K * KM_COLS + 2) * 2];
    __shared__ int last;
    const int tid = threadIdx.x;
    // written by the previous launch's last workgroup, or by the host through the stream: a launch boundary lies in between
    if (mode == KM_MODE_RUN && st->done) return;
    const int K = st->k, cur = st->slot, ncol = K * KM_COLS + 2;
    if (tid < K) {
        const double a = st->cent[cur][tid][0], b = st->cent[cur][tid][1];
        cw[tid] = a; ch[tid] = b; cs[tid] = a * b;
    }
    if (tid < ncol) acc[tid] = 0ull;
    __syncthreads();

    u64 d_lo = 0ull, d_hi = 0ull;
    for (int i = blockIdx.x * KM_PASS_THREADS + tid; i < n; i += gridDim.x * KM_PASS_THREADS) {
        const double2 b = boxes[i];                                    // one 16-byte load
        const double s1 = b.x * b.y;
        double best = 1.0;
        int g = 0;
        for (int k = 0; k < K; ++k) {                                  // strict <, in centroid order: ties go to the lower index
            const double d = distance(b.x, b.y, s1, cw[k], ch[k], cs[k]);
            if (d < best) { best = d; g = k; }
        }
        const u64 dv = scaled53(best);
        d_lo += dv & 0xffffffffull; d_hi += dv >> 32;
        u64* a = acc + g * KM_COLS;
        atomicAdd(a, 1ull);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const u64 bits = (u64)__double_as_longlong(c ? b.y : b.x);
            const int e = (int)(bits >> 52) - 1023;                    // 0..15 on the domain
            const u64 m = (bits & 0xfffffffffffffull) | 0x10000000000000ull;
            atomicAdd(a + 1 + 2 * c, (m << e) & 0x7fffffffffffull);    // bits 0..46 of m << e
            atomicAdd(a + 2 + 2 * c, m >> (47 - e));                   // bits 47..67
        }
    }
    d_lo = wave_sum(d_lo); d_hi = wave_sum(d_hi);
    if ((tid & 63) == 0) { atomicAdd(acc + ncol - 2, d_lo); atomicAdd(acc + ncol - 1, d_hi); }
    __syncthreads();

    // The hand-off: 8-byte agent-scope atomic stores, retired by every storing wave before the barrier, a relaxed ticket, and
    // agent-scope atomic loads of the same words on the other side.  Nobody waits for anybody.
    if (tid < ncol) __hip_atomic_store(slab + (size_t)blockIdx.x * ncol + tid, acc[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1;
        if (last) __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int j = tid; j < ncol * 2; j += KM_PASS_THREADS) fold[j] = 0ull;
    __syncthreads();
    if (!last) return;

    // 16 loads in flight per thread: the fold is bound by the latency of these loads, not by their number
    const int total = (int)gridDim.x * ncol;
    for (int j0 = 0; j0 < total; j0 += KM_FOLD * KM_PASS_THREADS) {
        u64 v[KM_FOLD];
#pragma unroll
        for (int q = 0; q < KM_FOLD; ++q) {
            const int j = j0 + q * KM_PASS_THREADS + tid;
            v[q] = j < total ? __hip_atomic_load(slab + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
#pragma unroll
        for (int q = 0; q < KM_FOLD; ++q) {
            const int j = j0 + q * KM_PASS_THREADS + tid;
            if (j < total && v[q]) {
                const int c = j % ncol;
                atomicAdd(fold + 2 * c, v[q] & 0xffffffffull);
                atomicAdd(fold + 2 * c + 1, v[q] >> 32);
            }
        }
    }
    __syncthreads();
    const int nxt = cur ^ 1;
    if (tid < 2 * K) {                                                 // one thread per (group, axis) rounds its sum
        const int k = tid >> 1, c = tid & 1;
        const u64* f = fold + 2 * (k * KM_COLS);
        const u64 cnt = f[0] + (f[1] << 32);
        u128 t = {0ull, 0ull};
        add_shifted(t, f[2 + 4 * c], 0); add_shifted(t, f[3 + 4 * c], 32);            // the lo limbs
        add_shifted(t, f[4 + 4 * c] + (f[5 + 4 * c] << 32), 47);                      // the hi limbs: below 2^45 in all
        const double s = round128(t, -52);
        st->cent[nxt][k][c] = s / (double)(cnt > 1ull ? cnt : 1ull);
        if (c == 0) st->count[nxt][k] = (int64_t)cnt;
    }
    if (tid == 64) {                                                   // another wave than the centroids': the loss and the decision
        const u64* f = fold + 2 * (ncol - 2);                         // sum d * 2^53 = f0 + (f1 + f2) * 2^32 + f3 * 2^64
        u128 t = {0ull, 0ull};
        add_shifted(t, f[0], 0); add_shifted(t, f[1], 32); add_shifted(t, f[2], 32); add128(t, f[3], 0ull);
        const double loss = round128(t, -53);
        const int it = st->it + 1;
        st->loss[nxt] = loss;
        if (mode == KM_MODE_RUN) {                                     // anchor_box_kmeans :147-155
            if (it == 1) st->old_loss = loss;
            else if (fabs(st->old_loss - loss) < loss_convergence || it > iters) st->done = 1;
            else st->old_loss = loss;
        }
        st->it = it;
        st->slot = nxt;
    }
}

// ---- the group of every box for the current centroids ------------------------------------------------------------------------------
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(const double2* __restrict__ boxes, int n, const KmDev* st, int32_t* __restrict__ group)
{
    __shared__ double cw[KM_MAX_K], ch[KM_MAX_K], cs[KM_MAX_K];
    const int tid = threadIdx.x, K = st->k, cur = st->slot;
    if (tid < K) {
        const double a = st->cent[cur][tid][0], b = st->cent[cur][tid][1];
        cw[tid] = a; ch[tid] = b; cs[tid] = a * b;
    }
    __syncthreads();
    for (int i = blockIdx.x * KM_THREADS + tid; i < n; i += gridDim.x * KM_THREADS) {
        const double2 b = boxes[i];
        const double s1 = b.x * b.y;
        double best = 1.0;
        int g = 0;
        for (int k = 0; k < K; ++k) {
            const double d = distance(b.x, b.y, s1, cw[k], ch[k], cs[k]);
            if (d < best) { best = d; g = k; }
        }
        group[i] = g;
    }
}

// ---- k-means++ (init_centroids :58-92) ---------------------------------------------------------------------------------------------
__global__ void km_seed_first_kernel(const double2* __restrict__ boxes, KmDev* st, int first, int k)
{
    const double2 b = boxes[first];
    st->cent[0][0][0] = b.x; st->cent[0][0][1] = b.y;
    st->picked[0] = first;
    st->k = k; st->slot = 0; st->it = 0; st->done = 0;
}

// min_distance[i] = min(min_distance[i], distance to the newest centroid r - 1) (1 before the first), and the exact sum of each
// workgroup's KM_CHUNK consecutive boxes as an integer
__global__ __launch_bounds__(KM_THREADS) void km_seed_update_kernel(const double2* __restrict__ boxes, int n, const KmDev* st, int r,
                                                                    double* __restrict__ md, u64* __restrict__ block_sum)
{
    __shared__ u64 part[KM_THREADS / 64];
    const int tid = threadIdx.x;
    const double cw = st->cent[0][r - 1][0], ch = st->cent[0][r - 1][1], cs = cw * ch;
    u64 s = 0ull;
#pragma unroll
    for (int q = 0; q < KM_CHUNK / KM_THREADS; ++q) {
        const int i = blockIdx.x * KM_CHUNK + q * KM_THREADS + tid;
        if (i < n) {
            const double2 b = boxes[i];
            const double d = distance(b.x, b.y, b.x * b.y, cw, ch, cs);
            const double old = r == 1 ? 1.0 : md[i];
            const double m = d < old ? d : old;
            md[i] = m;
            s += scaled53(m);
        }
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) block_sum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__device__ __forceinline__ u128 block_sum128(u128 v, u128* lds)         // the sum over the workgroup's 256 threads, to every thread
{
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int o = KM_THREADS / 2; o >= 1; o >>= 1) {
        if (tid < o) { u128 a = lds[tid]; const u128 b = lds[tid + o]; add128(a, b.hi, b.lo); lds[tid] = a; }
        __syncthreads();
    }
    const u128 r = lds[0];
    __syncthreads();
    return r;
}

// sum_distance: the exact total, rounded once.  One workgroup.
__global__ __launch_bounds__(KM_THREADS) void km_seed_total_kernel(const u64* __restrict__ block_sum, int nb, KmDev* st)
{
    __shared__ u128 lds[KM_THREADS];
    u128 t = {0ull, 0ull};
    for (int b = threadIdx.x; b < nb; b += KM_THREADS) add128(t, 0ull, block_sum[b]);
    t = block_sum128(t, lds);
    if (threadIdx.x == 0) st->sum_d = round128(t, -53);
}

// The pick of round r: the first index whose exact prefix sum P_i (in units of 2^-53) is > T = floor(thresh * 2^53); -1 and a (0, 0)
// centroid when no index qualifies.  One workgroup: the chunk whose prefix crosses T, then the box inside it.
__global__ __launch_bounds__(KM_THREADS) void km_seed_select_kernel(const double2* __restrict__ boxes, int n, const double* __restrict__ md,
                                                                    const u64* __restrict__ block_sum, int nb, u64 t_hi, u64 t_lo, int r,
                                                                    KmDev* st)
{
    __shared__ u128 pre[KM_THREADS];
    __shared__ u64 scan_lds[4];
    __shared__ int sel_b, pick;
    __shared__ u64 sel_r;
    const int tid = threadIdx.x;
    const u128 T = {t_hi, t_lo};
    const int Q = (nb + KM_THREADS - 1) / KM_THREADS;
    const int b0 = min(tid * Q, nb), b1 = min(b0 + Q, nb);
    u128 run = {0ull, 0ull};
    for (int b = b0; b < b1; ++b) add128(run, 0ull, block_sum[b]);
    if (tid == 0) { sel_b = -1; pick = 0x7fffffff; sel_r = 0ull; }
    pre[tid] = run;
    __syncthreads();
    for (int o = 1; o < KM_THREADS; o <<= 1) {                          // inclusive scan of the runs
        u128 v = pre[tid];
        const bool take = tid >= o;
        const u128 u = take ? pre[tid - o] : u128{0ull, 0ull};
        __syncthreads();
        if (take) { add128(v, u.hi, u.lo); pre[tid] = v; }
        __syncthreads();
    }
    const u128 incl = pre[tid];
    const u128 excl = tid ? pre[tid - 1] : u128{0ull, 0ull};
    if (gt128(incl, T) && !gt128(excl, T)) {                            // prefixes never decrease: at most one thread
        u128 e = excl;
        for (int b = b0; b < b1; ++b) {
            u128 nx = e;
            add128(nx, 0ull, block_sum[b]);
            if (gt128(nx, T)) { sel_b = b; sel_r = T.lo - e.lo; break; }   // T - e < block_sum[b] <= 2^63: the low words suffice
            e = nx;
        }
    }
    __syncthreads();
    const int sb = sel_b;
    if (sb >= 0) {
        const u64 R = sel_r;
        u64 v[4], s = 0ull;
        const int base = sb * KM_CHUNK + 4 * tid;                       // 4 consecutive boxes per thread, in index order
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[q] = base + q < n ? scaled53(md[base + q]) : 0ull; s += v[q]; }
        u64 p = evs::block_scan_incl(s, [](u64 a, u64 b) { return a + b; }, scan_lds) - s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p += v[q];
            if (p > R && base + q < n) { atomicMin(&pick, base + q); break; }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int i = (sb >= 0 && pick < n) ? pick : -1;
        double2 b = {0.0, 0.0};
        if (i >= 0) b = boxes[i];
        st->cent[0][r][0] = b.x; st->cent[0][r][1] = b.y;
        st->picked[r] = i;
    }
}

// ---- launch functions: no allocation, no synchronisation -----------------------------------------------------------------------------
int pass_blocks(int n) { return std::min((n + KM_PASS_THREADS - 1) / KM_PASS_THREADS, KM_PASS_BLOCKS); }
int flat_blocks(int n) { return std::min((n + KM_THREADS - 1) / KM_THREADS, 1024); }
int seed_blocks(int n) { return (n + KM_CHUNK - 1) / KM_CHUNK; }

}  // namespace

struct KmeansState {
    int device = 0;
    int64_t capacity = 0;
    int max_k = 0, n = 0, k = 0;
    bool have_centroids = false;
    DevBuf<double2> boxes;
    DevBuf<double> md;
    DevBuf<u64> block_sum, slab;
    DevBuf<KmDev> st;
    PinnedBuf<KmDev> pinned;
    int64_t host_reads = 0, passes = 0;        // of the last yn_kmeans_run
};

namespace {

void launch_pass(KmeansState* e, hipStream_t s, int mode, double conv, int iters)
{
    hipLaunchKernelGGL(km_pass_kernel, dim3(pass_blocks(e->n)), dim3(KM_PASS_THREADS), 0, s, e->boxes, e->n, e->st, e->slab, mode, conv, iters);
}

int read_state(KmeansState* e, hipStream_t s, std::string& err)        // the one host read: the whole record, then wait
{
    EVCHK(hipMemcpyAsync(e->pinned, e->st, sizeof(KmDev), hipMemcpyDeviceToHost, s));
    EVCHK(hipStreamSynchronize(s));
    return 0;
}

void copy_result(const KmeansState* e, double* centroids, int64_t* counts, double* loss)
{
    const KmDev& p = e->pinned[0];
    if (centroids) memcpy(centroids, p.cent[p.slot], sizeof(double) * 2 * e->k);
    if (counts) memcpy(counts, p.count[p.slot], sizeof(int64_t) * e->k);
    if (loss) *loss = p.loss[p.slot];
}

// floor(x * 2^53) for a finite x >= 0, as 128 bits (x < 2^75)
void floor_scaled53(double x, u64* hi, u64* lo)
{
    *hi = *lo = 0ull;
    if (!(x > 0.0)) return;
    int ex;
    const double fr = frexp(x, &ex);                                   // x = fr * 2^ex, fr in [0.5, 1)
    const u64 m = (u64)ldexp(fr, 53);                                  // 53-bit integer, exact
    const int sh = ex;                                                 // x * 2^53 = m * 2^ex
    if (sh <= -64) return;
    if (sh < 0) { *lo = m >> -sh; return; }
    if (sh == 0) { *lo = m; return; }
    if (sh >= 64) { *hi = m << (sh - 64); return; }
    *lo = m << sh; *hi = m >> (64 - sh);
}

}  // namespace

int kmeans_create(int device, int64_t capacity, int max_k, KmeansState** out, std::string& err)
{
    if (capacity < 1 || capacity > KM_MAX_N) { err = "yn_kmeans_create: capacity must be 1..2^24 boxes"; return 1; }
    if (max_k < 1 || max_k > KM_MAX_K) { err = "yn_kmeans_create: max_k must be 1..32"; return 1; }
    auto* e = new KmeansState;
    e->device = device; e->capacity = capacity; e->max_k = max_k;
    int r = e->boxes.reserve((size_t)capacity);
    if (!r) r = e->md.reserve((size_t)capacity);
    if (!r) r = e->block_sum.reserve((size_t)seed_blocks((int)capacity));
    if (!r) r = e->slab.reserve((size_t)KM_PASS_BLOCKS * (KM_MAX_K * KM_COLS + 2));
    if (!r) r = e->st.reserve(1);
    if (!r) r = e->pinned.reserve(1);
    if (!r) r = hipMemset(e->st, 0, sizeof(KmDev));
    if (r) { err = std::string("yn_kmeans_create: ") + hipGetErrorString((hipError_t)r); kmeans_destroy(e); return 1; }
    *out = e;
    return 0;
}

void kmeans_destroy(KmeansState* e)
{
    if (!e) return;
    DeviceScope on(e->device);
    delete e;
}

int kmeans_set_boxes(KmeansState* e, hipStream_t s, const double* wh_dev, int64_t n, std::string& err)
{
    e->n = 0; e->have_centroids = false;
    if (!wh_dev) { err = "yn_kmeans_set_boxes: null boxes"; return 1; }
    if (n < 1 || n > e->capacity) { err = "yn_kmeans_set_boxes: n must be 1.." + std::to_string(e->capacity) + " (the capacity), got " + std::to_string(n); return 1; }
    EVCHK(hipMemsetAsync(e->st, 0, sizeof(KmDev), s));
    hipLaunchKernelGGL(km_set_boxes_kernel, dim3(flat_blocks((int)n)), dim3(KM_THREADS), 0, s, (const double2*)wh_dev, e->boxes, (int)n, e->st);
    EVCHK(hipGetLastError());
    if (read_state(e, s, err)) return 1;
    if (e->pinned[0].bad) {
        err = "yn_kmeans_set_boxes: " + std::to_string(e->pinned[0].bad) + " of " + std::to_string(n) +
              " boxes are outside the domain 1 <= w, h < 65536 or not finite";
        return 1;
    }
    e->n = (int)n;
    return 0;
}

int kmeans_seed(KmeansState* e, hipStream_t s, int k, int64_t first_index, const double* u_host, double* centroids_host,
                int32_t* picked_host, std::string& err)
{
    if (!e->n) { err = "yn_kmeans_seed: no boxes set"; return 1; }
    if (k < 1 || k > e->max_k) { err = "yn_kmeans_seed: k must be 1.." + std::to_string(e->max_k); return 1; }
    if (first_index < 0 || first_index >= e->n) { err = "yn_kmeans_seed: first_index outside 0..n-1"; return 1; }
    if (k > 1 && !u_host) { err = "yn_kmeans_seed: null draws"; return 1; }
    for (int r = 1; r < k; ++r)
        if (!(u_host[r - 1] >= 0.0 && u_host[r - 1] < 1.0)) { err = "yn_kmeans_seed: every draw must lie in [0, 1)"; return 1; }
    e->have_centroids = false;
    const int nb = seed_blocks(e->n);
    hipLaunchKernelGGL(km_seed_first_kernel, dim3(1), dim3(1), 0, s, e->boxes, e->st, (int)first_index, k);
    for (int r = 1; r < k; ++r) {
        hipLaunchKernelGGL(km_seed_update_kernel, dim3(nb), dim3(KM_THREADS), 0, s, e->boxes, e->n, e->st, r, e->md, e->block_sum);
        hipLaunchKernelGGL(km_seed_total_kernel, dim3(1), dim3(KM_THREADS), 0, s, e->block_sum, nb, e->st);
        EVCHK(hipGetLastError());
        if (read_state(e, s, err)) return 1;                           // sum_distance: the threshold needs it
        const double thresh = e->pinned[0].sum_d * u_host[r - 1];
        u64 t_hi, t_lo;
        floor_scaled53(thresh, &t_hi, &t_lo);
        hipLaunchKernelGGL(km_seed_select_kernel, dim3(1), dim3(KM_THREADS), 0, s, e->boxes, e->n, e->md, e->block_sum, nb, t_hi, t_lo, r, e->st);
    }
    EVCHK(hipGetLastError());
    if (read_state(e, s, err)) return 1;
    e->k = k; e->have_centroids = true;
    if (centroids_host) memcpy(centroids_host, e->pinned[0].cent[0], sizeof(double) * 2 * k);
    if (picked_host) memcpy(picked_host, e->pinned[0].picked, sizeof(int32_t) * k);
    return 0;
}

int kmeans_set_centroids(KmeansState* e, hipStream_t s, const double* wh_host, int k, std::string& err)
{
    if (k < 1 || k > e->max_k) { err = "yn_kmeans_set_centroids: k must be 1.." + std::to_string(e->max_k); return 1; }
    if (!wh_host) { err = "yn_kmeans_set_centroids: null centroids"; return 1; }
    for (int i = 0; i < 2 * k; ++i)
        if (!(wh_host[i] >= 0.0 && wh_host[i] < 65536.0)) { err = "yn_kmeans_set_centroids: a centroid side is outside 0 <= v < 65536 or not finite"; return 1; }
    EVCHK(hipStreamSynchronize(s));                                    // the pinned record may still be the target of an earlier copy
    KmDev& p = e->pinned[0];
    memset(&p, 0, sizeof(KmDev));
    p.k = k;
    memcpy(p.cent[0], wh_host, sizeof(double) * 2 * k);
    EVCHK(hipMemcpyAsync(e->st, e->pinned, sizeof(KmDev), hipMemcpyHostToDevice, s));
    EVCHK(hipStreamSynchronize(s));
    e->k = k; e->have_centroids = true;
    return 0;
}

int kmeans_pass(KmeansState* e, hipStream_t s, double* centroids_host, int64_t* counts_host, double* loss_host, std::string& err)
{
    if (!e->n || !e->have_centroids) { err = "yn_kmeans_pass: set the boxes and seed or set the centroids first"; return 1; }
    EVCHK(hipMemsetAsync(e->st, 0, 16, s));                            // the ticket's block
    launch_pass(e, s, KM_MODE_SINGLE, 0.0, 0);
    EVCHK(hipGetLastError());
    if (read_state(e, s, err)) return 1;
    copy_result(e, centroids_host, counts_host, loss_host);
    return 0;
}

int kmeans_run(KmeansState* e, hipStream_t s, double loss_convergence, int iters, double* centroids_host, int64_t* counts_host,
               double* loss_host, int32_t* iterations_host, std::string& err)
{
    if (!e->n || !e->have_centroids) { err = "yn_kmeans_run: set the boxes and seed or set the centroids first"; return 1; }
    if (!(loss_convergence >= 0.0)) { err = "yn_kmeans_run: loss_convergence must be >= 0"; return 1; }
    EVCHK(hipMemsetAsync(e->st, 0, 32, s));                            // the ticket's block, then it and done
    // the loop stops at iterations > iters at the latest, and never before the second pass
    const int64_t most = std::max<int64_t>((int64_t)iters + 1, 2);
    e->host_reads = 0; e->passes = 0;
    for (int64_t sent = 0; sent < most;) {
        const int batch = (int)std::min<int64_t>(KM_BATCH, most - sent);
        for (int i = 0; i < batch; ++i) launch_pass(e, s, KM_MODE_RUN, loss_convergence, iters);   // no-ops once `done` is set
        EVCHK(hipGetLastError());
        sent += batch;
        if (read_state(e, s, err)) return 1;                           // one host read per batch
        ++e->host_reads;
        if (e->pinned[0].done) break;
    }
    if (!e->pinned[0].done) { err = "yn_kmeans_run: the loop did not stop within its bound of passes"; return 1; }
    e->passes = e->pinned[0].it;
    copy_result(e, centroids_host, counts_host, loss_host);
    if (iterations_host) *iterations_host = e->pinned[0].it;
    return 0;
}

int kmeans_assign(KmeansState* e, hipStream_t s, int32_t* group_dev, std::string& err)
{
    if (!e->n || !e->have_centroids) { err = "yn_kmeans_assign: set the boxes and seed or set the centroids first"; return 1; }
    if (!group_dev) { err = "yn_kmeans_assign: null output"; return 1; }
    hipLaunchKernelGGL(km_assign_kernel, dim3(flat_blocks(e->n)), dim3(KM_THREADS), 0, s, e->boxes, e->n, e->st, group_dev);
    EVCHK(hipGetLastError());
    return 0;
}

void kmeans_stats(const KmeansState* e, int64_t* passes, int64_t* host_reads)
{
    if (passes) *passes = e->passes;
    if (host_reads) *host_reads = e->host_reads;
}

}  // namespace ynk
