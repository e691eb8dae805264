// kernels_soft.hip — Soft-NMS, the third suppression function of the per-class NMS (the rule is the package's own, restated in
// tests/soft_nms_oracle.py, and parity with any third-party Soft-NMS is UNPINNED).
//
//   soft_nms_kernel   one 256-lane workgroup per (list, class) segment.  The segment's rows come in the order the NMS chain's bucket + sort left
//                     (only the grouping is used: the pick is a dynamic arg-max, a decay can reorder the rows).  A pick is one pass: every lane
//                     decays its rows (row j belongs to lane j % 256) against the picked box and keeps a running (score, row) maximum for the
//                     NEXT pick; the wavefronts reduce it with shuffles and meet through LDS.  The kept row's score goes to a side array at its
//                     row and keep[row] is set: the chain's compact_kernel gathers them in ascending row order.
//   soft_exp_kernel   E over an array (testing aid: the exp is pinned on its own)
//
// Every value operation is one IEEE float32 operation written with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn (the file is built with
// -ffp-contract=off as well).  The overlap is kernels_post.hip's suppressed() with the picked box in the place of bi, never DIoU.
//
// Nothing is exchanged between workgroups: no ticket, no flag, no spin wait, no atomic on device memory.  Inside the workgroup the loop's trip
// count comes from a value every lane reads from LDS behind the barrier, so no wavefront waits at a barrier the others skip.  The cost is
// picks x ceil(rows / 256) lane steps with a serial dependence over the picks (DESIGN.md 31 has the arithmetic).
#include <hip/hip_runtime.h>

#include "yn_internal.h"

namespace ynk {

namespace {

typedef unsigned long long u64;

// the package's exp for x <= 0 (tests/soft_nms_oracle.py E): Cephes' expf polynomial, every step one rounded operation
__device__ __forceinline__ float soft_exp(float x)
{
    if (x != x) return x;
    if (x < -87.0f) return 0.0f;
    const float k = rintf(__fmul_rn(x, 1.44269504f));       // ties to even
    const float r = __fsub_rn(__fsub_rn(x, __fmul_rn(k, 0.693359375f)), __fmul_rn(k, -2.12194440e-4f));
    float p = 1.9875691500e-4f;
    p = __fadd_rn(__fmul_rn(p, r), 1.3981999507e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 8.3334519073e-3f);
    p = __fadd_rn(__fmul_rn(p, r), 4.1665795894e-2f);
    p = __fadd_rn(__fmul_rn(p, r), 1.6666665459e-1f);
    p = __fadd_rn(__fmul_rn(p, r), 5.0000001201e-1f);
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(p, __fmul_rn(r, r)), r), 1.0f);
    return ldexpf(y, (int)k);
}

// A row's new score after the pick of box P (area_p its area), or a negative number when a hard hit removes it.  For hard and linear the
// division is left out where the row cannot be hit, by suppressed()'s argument (kernels_post.hip): rounding is monotonic, so
// inter < thr * un in real arithmetic - tested with a 1e-5 guard band for the rounding of the product - implies fl(inter / un) <= thr.
// Gaussian needs the VALUE of ovr for every row and always divides.
template <int METHOD>
__device__ __forceinline__ float soft_decay(float s, const float4 P, float area_p, const float4 r, float thr, float sigma)
{
    const float xx1 = fmaxf(P.x, r.x), yy1 = fmaxf(P.y, r.y);
    const float xx2 = fminf(P.z, r.z), yy2 = fminf(P.w, r.w);
    const float w = fmaxf(1e-28f, __fsub_rn(xx2, xx1));
    const float h = fmaxf(1e-28f, __fsub_rn(yy2, yy1));
    const float inter = __fmul_rn(w, h);
    const float area_r = __fmul_rn(__fsub_rn(r.z, r.x), __fsub_rn(r.w, r.y));
    const float un = __fsub_rn(__fadd_rn(area_p, area_r), inter);
    if (METHOD == SOFT_GAUSSIAN) {
        const float o = __fdiv_rn(inter, un);
        return __fmul_rn(s, soft_exp(-__fdiv_rn(__fmul_rn(o, o), sigma)));
    }
    const float p = __fmul_rn(thr, un);
    if (un > 0.0f && p > 1e-30f && inter < __fmul_rn(p, 0.99999f)) return s;      // not hit: the weight is 1
    const float o = __fdiv_rn(inter, un);
    if (o <= thr) return s;                                  // (a NaN hits)
    if (METHOD == SOFT_HARD) return -1.0f;
    return __fmul_rn(s, __fsub_rn(1.0f, o));
}

// (score, row) of a live row as one unsigned key: a live score is above score_floor >= 0, so its bits order as the floats do, and among equal
// scores the higher row wins.  0 = no live row.
__device__ __forceinline__ u64 soft_key(float s, int id) { return ((u64)__float_as_uint(s) << 32) | (unsigned)id; }

// the workgroup's LDS: the state of the segment's first YN_SOFT_LDS_ROWS rows (24 bytes a row) and the wavefronts' maxima
struct SoftLds {
    float4 box[YN_SOFT_LDS_ROWS];
    float s[YN_SOFT_LDS_ROWS];
    int id[YN_SOFT_LDS_ROWS];
    u64 key[2][4];                                          // two sets: a pick reads one while the next is written
    int pos[2][4];
};
static_assert(YN_SOFT_LDS_ROWS % 256 == 0, "a step's 256 rows lie on one side of the LDS / spill boundary");

template <int METHOD>
__device__ __forceinline__ void soft_walk(SoftLds& lds, const float* __restrict__ scores, const int32_t* __restrict__ bucket, const float4* __restrict__ sbox,
                                          int N, int n, size_t row0, size_t seg0, float thr, float sigma, float floor_,
                                          int32_t* __restrict__ keep, float* __restrict__ wscore, float* spill)
{
    constexpr int L = YN_SOFT_LDS_ROWS;
    float4* const l_box = lds.box; float* const l_s = lds.s; int* const l_id = lds.id;
    u64 (&l_key)[2][4] = lds.key; int (&l_pos)[2][4] = lds.pos;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // rows below L live in LDS (box, score, row id); beyond, the boxes stay in sbox, the ids in bucket, and the scores go to the spill array
    // at the row's sorted slot - read and written by the row's own lane only
    u64 best = 0;
    int best_pos = 0;
    for (int j = tid; j < n; j += 256) {
        const int id = bucket[seg0 + j];
        const float s = scores[row0 + id];
        if (j < L) { l_box[j] = sbox[seg0 + j]; l_s[j] = s; l_id[j] = id; }
        else spill[seg0 + j] = s;
        if (s > floor_) {                                    // (strict: a NaN score is never live)
            const u64 k = soft_key(s, id);
            if (k > best) { best = k; best_pos = j; }
        }
    }
    int par = 0;
    for (int it = 0; it <= n; ++it) {                        // at most n picks: every pick takes a row out of the live set
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const u64 k2 = __shfl_xor(best, o);
            const int p2 = __shfl_xor(best_pos, o);
            if (k2 > best) { best = k2; best_pos = p2; }
        }
        if (lane == 0) { l_key[par][wave] = best; l_pos[par][wave] = best_pos; }
        __syncthreads();
        // every lane reads the same four maxima: the pick, and with it the loop's exit, is uniform over the workgroup
        u64 k = l_key[par][0];
        int pos = l_pos[par][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const u64 k2 = l_key[par][w];
            if (k2 > k) { k = k2; pos = l_pos[par][w]; }
        }
        par ^= 1;
        // (the same value in every lane: through scalar registers, so that the exit is a scalar branch)
        k = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(k >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)k);
        pos = __builtin_amdgcn_readfirstlane(pos);
        if (k == 0 || it == n) break;
        const float sp = __uint_as_float((unsigned)(k >> 32));
        const int idp = (int)(unsigned)(k & 0xffffffffu);
        if ((unsigned)pos >= (unsigned)n || (unsigned)idp >= (unsigned)N) break;      // (never: pos and idp name a row of the segment)
        const float4 P = pos < L ? l_box[pos] : sbox[seg0 + pos];
        const float area_p = __fmul_rn(__fsub_rn(P.z, P.x), __fsub_rn(P.w, P.y));
        if (tid == 0) { wscore[row0 + idp] = sp; keep[row0 + idp] = 1; }
        best = 0; best_pos = 0;
        const int n_lds = n < L ? n : L;
        for (int j = tid; j < n_lds; j += 256) {
            float s = l_s[j];
            if (!(s > floor_)) continue;
            if (j == pos) { l_s[j] = -1.0f; continue; }      // the picked row leaves the live set
            const float s2 = soft_decay<METHOD>(s, P, area_p, l_box[j], thr, sigma);
            if (__float_as_uint(s2) != __float_as_uint(s)) { l_s[j] = s2; s = s2; }
            if (s > floor_) {
                const u64 kk = soft_key(s, l_id[j]);
                if (kk > best) { best = kk; best_pos = j; }
            }
        }
        // the spilled rows, four of a lane's rows per round: their scores, boxes and ids are requested together (one after the other, every
        // row would wait a round trip to L2 for its score and another for its box and id)
        for (int j0 = L + tid; j0 < n; j0 += 1024) {
            float sv[4]; float4 rv[4]; int idv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t a = seg0 + (j0 + 256 * u < n ? j0 + 256 * u : j0);
                sv[u] = spill[a]; rv[u] = sbox[a]; idv[u] = bucket[a];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + 256 * u;
                float s = sv[u];
                if (j >= n || !(s > floor_)) continue;
                if (j == pos) { spill[seg0 + j] = -1.0f; continue; }
                const float s2 = soft_decay<METHOD>(s, P, area_p, rv[u], thr, sigma);
                if (__float_as_uint(s2) != __float_as_uint(s)) { spill[seg0 + j] = s2; s = s2; }
                if (s > floor_) {
                    const u64 kk = soft_key(s, idv[u]);
                    if (kk > best) { best = kk; best_pos = j; }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void soft_nms_kernel(const float* __restrict__ scores, const int32_t* __restrict__ seg_count,
                                                       const int32_t* __restrict__ seg_off, const int32_t* __restrict__ bucket,
                                                       const float4* __restrict__ sbox, const int32_t* __restrict__ seg_order, int N, int C,
                                                       int method, float thr, float sigma, float floor_, int32_t* __restrict__ keep,
                                                       float* __restrict__ wscore, float* spill)
{
    __shared__ SoftLds lds;
    const int b = blockIdx.x;
    const int c = seg_order ? seg_order[(size_t)b * C + blockIdx.y] : (int)blockIdx.y;      // large segments first (bucket_kernel's ranking)
    if (c < 0 || c >= C) return;                            // (never)
    const int n = seg_count[(size_t)b * C + c];
    if (n <= 0) return;
    const int off = seg_off[(size_t)b * C + c];
    if (off < 0 || n > N - off) return;                     // (never: the segments partition the list's rows)
    const size_t row0 = (size_t)b * N;                      // the list's first row in every [B][N] array
    const size_t seg0 = row0 + off;                         // the segment's first sorted slot
    // (method is a kernel argument: the branch is uniform, and each walk is compiled for its method alone)
    if (method == SOFT_GAUSSIAN) soft_walk<SOFT_GAUSSIAN>(lds, scores, bucket, sbox, N, n, row0, seg0, thr, sigma, floor_, keep, wscore, spill);
    else if (method == SOFT_LINEAR) soft_walk<SOFT_LINEAR>(lds, scores, bucket, sbox, N, n, row0, seg0, thr, sigma, floor_, keep, wscore, spill);
    else soft_walk<SOFT_HARD>(lds, scores, bucket, sbox, N, n, row0, seg0, thr, sigma, floor_, keep, wscore, spill);
}

__global__ __launch_bounds__(256) void soft_exp_kernel(const float* __restrict__ x, float* __restrict__ y, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = soft_exp(x[i]);
}

}  // namespace

void launch_soft_pipeline(const float* boxes, const float* scores, const int32_t* cls, int B, int N, int C, int method, float iou_thresh,
                          float sigma, float score_floor, const NmsWork& wk, const SoftWork& sw, float* out_boxes, float* out_scores,
                          int32_t* out_cls, int32_t* out_index, int32_t* count, hipStream_t s, const NmsHook* hook)
{
    auto mark = [&](const char* k) { if (hook && hook->fn) hook->fn(hook->ctx, k); };
    NmsPlan rec{};
    rec.B = B; rec.N = N; rec.C = C;
    const int32_t* seg_order = launch_nms_bucket_sort(boxes, scores, cls, B, N, C, wk, s, hook, rec);
    mark("soft_nms_kernel");
    hipLaunchKernelGGL(soft_nms_kernel, dim3(B, C), dim3(256), 0, s, scores, (const int32_t*)wk.seg_count, (const int32_t*)wk.seg_off,
                       (const int32_t*)wk.bucket, reinterpret_cast<const float4*>(wk.sbox), seg_order, N, C, method, iou_thresh, sigma, score_floor,
                       wk.keep, sw.wscore, sw.spill);
    mark("compact_kernel");
    launch_nms_compact(boxes, sw.wscore, cls, B, N, wk, out_boxes, out_scores, out_cls, out_index, count, s);
}

void launch_soft_exp(const float* x, float* y, long n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(soft_exp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n);
}

}  // namespace ynk
