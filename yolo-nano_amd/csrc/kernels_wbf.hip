// kernels_wbf.hip — weighted box fusion, the second merge rule of the merge lists (the rule is the package's own, restated in
// tests/wbf_oracle.py, and parity with the ensemble_boxes family is UNPINNED).
//
//   wbf_cluster_kernel   one 64-lane workgroup per (list, class) segment walks the segment's rows in the pick order the NMS chain's bucket + sort
//                        left (score descending, higher row first): per row the lanes evaluate the IoU against every cluster's FUSED box, a
//                        butterfly arg-max (largest ovr above the threshold, lowest cluster) picks one, lane 0 joins the row to it or founds a
//                        cluster.  At the end every cluster's box / score / votes go to side arrays at its founder's row and keep[row] is set:
//                        the chain's compact_kernel gathers them in ascending row order.
//   wbf_votes_kernel     the votes of the compacted clusters (compact_kernel gathers boxes, scores and classes; this is the fourth column)
//   fuse_append_kernel   yn_fuse_append: record rows to the end of their unit's merge list, score times weight
//
// Every value operation is one IEEE float32 operation written with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn (the file is built with
// -ffp-contract=off as well).  The IoU is kernels_post.hip's suppressed() without its division-free early outs: the VALUE of ovr decides here.
//
// One wavefront per segment: nothing is exchanged between wavefronts, so the walk needs no barrier, no ticket, no flag.  Its cost is
// rows x ceil(clusters / 64) lane steps with a serial dependence over the rows (wbf_cost; DESIGN.md 30 has the arithmetic).
#include <hip/hip_runtime.h>

#include "yn_internal.h"

namespace ynk {

namespace {

constexpr int WBF_NONE = 0x7fffffff;

// What lane 0 writes and the next row's lanes read inside the one wavefront.  A wavefront's LDS accesses execute in order, so for them a
// wavefront-scope fence (compiler ordering only) is enough, as in kernels_post.hip's tile_word_boxes; once clusters live in device memory
// (overflow) the fence has workgroup scope, which waits for those stores (the workgroup IS the wavefront).
__device__ __forceinline__ void wbf_publish(bool overflow)
{
    if (overflow) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// nms_stage_oracle.suppresses' ovr with the cluster's fused box in the place of bi (operand order kept) -> is it above thr, and its value.
// The division is left out where it cannot matter, by suppressed()'s argument (kernels_post.hip): rounding is monotonic, so
// inter < thr * un in real arithmetic - tested with a 1e-5 guard band for the rounding of the product - implies fl(inter / un) <= thr.
__device__ __forceinline__ bool wbf_above(const float4 f, const float4 b, float area_b, float thr, float& ovr)
{
    const float xx1 = fmaxf(f.x, b.x), yy1 = fmaxf(f.y, b.y);
    const float xx2 = fminf(f.z, b.z), yy2 = fminf(f.w, b.w);
    const float w = fmaxf(1e-28f, __fsub_rn(xx2, xx1));
    const float h = fmaxf(1e-28f, __fsub_rn(yy2, yy1));
    const float inter = __fmul_rn(w, h);
    const float area_f = __fmul_rn(__fsub_rn(f.z, f.x), __fsub_rn(f.w, f.y));
    const float un = __fsub_rn(__fadd_rn(area_f, area_b), inter);
    const float p = __fmul_rn(thr, un);
    if (un > 0.0f && p > 1e-30f && inter < __fmul_rn(p, 0.99999f)) return false;
    ovr = __fdiv_rn(inter, un);
    return ovr > thr;                                       // NaN: never above thr
}

// Cluster k of a segment lives in LDS below YN_WBF_LDS_CLUSTERS and in the overflow arrays from there on (slot seg0 + k: a segment has at most as
// many clusters as rows).  The overflow side is read and written with relaxed workgroup-scope atomics, word by word: it is lane-to-lane traffic
// through device memory, and the compiler can then not fold the two sides into one flat access (plain loads on both sides became
// flat_load_dwordx4 in the row loop).
template <class T> __device__ __forceinline__ T og_ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
template <class T> __device__ __forceinline__ void og_st(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ float4 og_ld4(const float4* p)
{
    const float* f = reinterpret_cast<const float*>(p);
    return make_float4(og_ld(f), og_ld(f + 1), og_ld(f + 2), og_ld(f + 3));
}
__device__ __forceinline__ void og_st4(float4* p, float4 v)
{
    float* f = reinterpret_cast<float*>(p);
    og_st(f, v.x); og_st(f + 1, v.y); og_st(f + 2, v.z); og_st(f + 3, v.w);
}

__global__ __launch_bounds__(64) void wbf_cluster_kernel(const float* __restrict__ scores, const int32_t* __restrict__ seg_count,
                                                         const int32_t* __restrict__ seg_off, const int32_t* __restrict__ bucket,
                                                         const float4* __restrict__ sbox, const int32_t* __restrict__ seg_order, int N, int C,
                                                         float thr, int expected, int32_t* __restrict__ keep, float4* wbox, float* wscore,
                                                         int32_t* wvotes, int32_t* assign, float4* ofb, float4* op, float* os, int32_t* on,
                                                         int32_t* ofounder)
{
    __shared__ float4 l_fb[YN_WBF_LDS_CLUSTERS];
    __shared__ float4 l_p[YN_WBF_LDS_CLUSTERS];
    __shared__ float l_s[YN_WBF_LDS_CLUSTERS];
    __shared__ int l_n[YN_WBF_LDS_CLUSTERS];
    __shared__ int l_founder[YN_WBF_LDS_CLUSTERS];
    const int b = blockIdx.x;
    const int c = seg_order ? seg_order[(size_t)b * C + blockIdx.y] : (int)blockIdx.y;      // large segments first (bucket_kernel's ranking)
    const int n = seg_count[(size_t)b * C + c];
    if (n <= 0) return;
    const int off = seg_off[(size_t)b * C + c];
    if (off < 0 || n > N - off) return;                     // (never: the segments partition the list's rows)
    const int lane = threadIdx.x;
    const size_t row0 = (size_t)b * N;                      // the list's first row in every [B][N] array
    const size_t seg0 = row0 + off;                         // the segment's first slot: sorted rows, and cluster k's overflow slot at seg0 + k
    float4* const g_fb = ofb + seg0; float4* const g_p = op + seg0;
    float* const g_s = os + seg0; int32_t* const g_n = on + seg0; int32_t* const g_founder = ofounder + seg0;
    constexpr int L = YN_WBF_LDS_CLUSTERS;
    static_assert(L % 64 == 0, "a lane keeps its residue across the LDS / overflow boundary");
    int K = 0;                                              // clusters so far (wavefront-uniform)
    for (int base = 0; base < n; base += 64) {
        const int m = min(64, n - base);
        // this chunk's 64 rows, one per lane, broadcast below
        const int j_mine = base + (lane < m ? lane : 0);
        const int my_id = bucket[seg0 + j_mine];
        const float4 my_box = sbox[seg0 + j_mine];
        const float my_score = scores[row0 + my_id];
        int my_founder = -1;                                // of this lane's row: stored after the chunk, so that no store sits in the serial walk
        for (int j = 0; j < m; ++j) {                       // (j is wavefront-uniform: the row travels through scalar registers)
            const int id = __builtin_amdgcn_readlane(my_id, j);
            const float sc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_score), j));
            float4 bx;
            bx.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_box.x), j));
            bx.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_box.y), j));
            bx.z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_box.z), j));
            bx.w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_box.w), j));
            const float area_b = __fmul_rn(__fsub_rn(bx.z, bx.x), __fsub_rn(bx.w, bx.y));
            // every cluster against the row: a lane's clusters ascend, so a strict compare keeps its lowest one among equals
            float best = 0.0f;
            int best_k = WBF_NONE;
            const int K_lds = K < L ? K : L;
            // four of a lane's clusters per step, their LDS loads issued together (one after the other, each step waits a full LDS round trip)
            for (int k0 = lane; k0 < K_lds; k0 += 256) {
                float4 f[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) f[u] = l_fb[k0 + 64 * u < K_lds ? k0 + 64 * u : k0];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + 64 * u;
                    float ovr;
                    if (k < K_lds && wbf_above(f[u], bx, area_b, thr, ovr) && (best_k == WBF_NONE || ovr > best)) { best = ovr; best_k = k; }
                }
            }
            for (int k = L + lane; k < K; k += 64) {        // (L is a multiple of 64: the lane's clusters go on ascending)
                float ovr;
                if (wbf_above(og_ld4(g_fb + k), bx, area_b, thr, ovr) && (best_k == WBF_NONE || ovr > best)) { best = ovr; best_k = k; }
            }
            // arg-max over the lanes that hold a match - mostly none or one, so they are walked by ballot on the scalar unit instead of a
            // six-step butterfly: largest ovr, lowest cluster among equals (lanes ascend, but a lane's cluster need not)
            unsigned long long holders = __ballot(best_k != WBF_NONE);
            float win = 0.0f;
            int win_k = WBF_NONE;
            while (holders) {
                const int l = __ffsll((long long)holders) - 1;
                holders &= holders - 1;
                const float ov = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best), l));
                const int ok = __builtin_amdgcn_readlane(best_k, l);
                if (win_k == WBF_NONE || ov > win || (ov == win && ok < win_k)) { win = ov; win_k = ok; }
            }
            best_k = win_k;                                 // (scalar: K stays a scalar)
            int founder;
            if (best_k == WBF_NONE) {                       // (wavefront-uniform) the row founds cluster K: its box bit for bit
                if (lane == 0) {
                    const float4 P = make_float4(__fmul_rn(sc, bx.x), __fmul_rn(sc, bx.y), __fmul_rn(sc, bx.z), __fmul_rn(sc, bx.w));
                    if (K < L) { l_fb[K] = bx; l_p[K] = P; l_s[K] = sc; l_n[K] = 1; l_founder[K] = id; }
                    else { og_st4(g_fb + K, bx); og_st4(g_p + K, P); og_st(g_s + K, sc); og_st(g_n + K, 1); og_st(g_founder + K, id); }
                }
                founder = id;
                ++K;
            } else {
                const bool in_lds = best_k < L;              // (wavefront-uniform)
                if (in_lds) founder = l_founder[best_k]; else founder = og_ld(g_founder + best_k);
                if (lane == 0) {
                    float S0; float4 P;
                    if (in_lds) { S0 = l_s[best_k]; P = l_p[best_k]; } else { S0 = og_ld(g_s + best_k); P = og_ld4(g_p + best_k); }
                    const float S = __fadd_rn(S0, sc);
                    P.x = __fadd_rn(P.x, __fmul_rn(sc, bx.x)); P.y = __fadd_rn(P.y, __fmul_rn(sc, bx.y));
                    P.z = __fadd_rn(P.z, __fmul_rn(sc, bx.z)); P.w = __fadd_rn(P.w, __fmul_rn(sc, bx.w));
                    const float4 F = make_float4(__fdiv_rn(P.x, S), __fdiv_rn(P.y, S), __fdiv_rn(P.z, S), __fdiv_rn(P.w, S));
                    if (in_lds) { l_fb[best_k] = F; l_p[best_k] = P; l_s[best_k] = S; l_n[best_k] += 1; }
                    else { og_st4(g_fb + best_k, F); og_st4(g_p + best_k, P); og_st(g_s + best_k, S); og_st(g_n + best_k, og_ld(g_n + best_k) + 1); }
                }
            }
            if (lane == j) my_founder = founder;
            wbf_publish(K > L);                             // the next row's lanes read what lane 0 wrote
        }
        if (assign && lane < m) assign[row0 + my_id] = my_founder;
    }
    // the clusters, at their founders' rows
    const float fe = (float)expected;
    for (int k = lane; k < K; k += 64) {
        int r, v; float S; float4 F;
        if (k < L) { r = l_founder[k]; v = l_n[k]; S = l_s[k]; F = l_fb[k]; }
        else { r = og_ld(g_founder + k); v = og_ld(g_n + k); S = og_ld(g_s + k); F = og_ld4(g_fb + k); }
        if (r < 0 || r >= N) continue;                      // (never: a founder is a row of the list)
        wbox[row0 + r] = F;
        wscore[row0 + r] = __fmul_rn(__fdiv_rn(S, (float)v), __fdiv_rn((float)(v < expected ? v : expected), fe));
        wvotes[row0 + r] = v;
        keep[row0 + r] = 1;
    }
}

// rows that are none (class -1) belong to no cluster
__global__ __launch_bounds__(256) void wbf_assign_clear_kernel(const int32_t* __restrict__ cls, long total, int32_t* __restrict__ assign)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total && cls[i] < 0) assign[i] = -1;
}

__global__ __launch_bounds__(256) void wbf_votes_kernel(const int32_t* __restrict__ wvotes, const int32_t* __restrict__ index,
                                                        const int32_t* __restrict__ count, int N, int32_t* __restrict__ out_votes)
{
    const int b = blockIdx.y;
    const int c = count[b];
    const int k = c < 0 ? -1 - c : c;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k || i >= N) return;
    const int r = index[(size_t)b * N + i];
    out_votes[(size_t)b * N + i] = wvotes[(size_t)b * N + (r >= 0 && r < N ? r : 0)];
}

__global__ __launch_bounds__(256) void fuse_append_kernel(const float* __restrict__ rec, const int32_t* __restrict__ offsets, int B, int C, int cap,
                                                          float weight, float* __restrict__ lboxes, float* __restrict__ lscores,
                                                          int32_t* __restrict__ lcls, int32_t* __restrict__ state)
{
    __shared__ int bad_s;
    const int b = blockIdx.x;
    const int last = offsets[B];
    const int total = last < 0 ? -1 - last : last;          // a negative offsets[B] is the range mark (pack_kernel)
    const int r0 = offsets[b], r1 = b + 1 < B ? offsets[b + 1] : total;
    const int n = r1 > r0 && r0 >= 0 ? r1 - r0 : 0;
    const int base = state[MERGE_STATE + b];
    if (threadIdx.x == 0) bad_s = 0;
    __syncthreads();                                        // every thread holds the cursor before thread 0 moves it
    if (threadIdx.x == 0) {
        const int end = base + n;
        state[MERGE_STATE + b] = end;
        if (end > cap) { atomicOr(&state[0], 1); atomicMax(&state[1], end); }
        if (last < 0 && b == 0) atomicOr(&state[2], 1);
    }
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int dst = base + i;
        if (dst >= cap) break;
        const float* r = rec + (size_t)(r0 + i) * 6;        // 24-byte records: 8-byte aligned
        const float2 a = *reinterpret_cast<const float2*>(r), bb = *reinterpret_cast<const float2*>(r + 2), sc = *reinterpret_cast<const float2*>(r + 4);
        const int ci = (sc.y >= 0.0f && sc.y < (float)C) ? (int)sc.y : -1;
        const bool ok = ci >= 0 && (float)ci == sc.y;       // an integer in 0 .. C - 1 (a NaN fails the first compare)
        bad += ok ? 0 : 1;
        const size_t d = (size_t)b * cap + dst;
        *reinterpret_cast<float4*>(lboxes + d * 4) = make_float4(a.x, a.y, bb.x, bb.y);
        lscores[d] = __fmul_rn(sc.x, weight);
        lcls[d] = ok ? ci : -1;
    }
    if (bad) atomicAdd(&bad_s, bad);
    __syncthreads();
    if (threadIdx.x == 0 && bad_s) atomicMax(&state[3], ((4095 - (b < 4095 ? b : 4095)) << 19) | (bad_s < (1 << 19) - 1 ? bad_s : (1 << 19) - 1));
}

}  // namespace

long long wbf_cost(long long n_rows, long long n_clusters)
{
    // sum over the rows i = 0 .. n_rows - 1 of max(1, ceil(min(i, n_clusters) / 64)): row i meets at most the clusters founded before it, 64 per
    // step, and a row that meets none still takes its step (the arg-max and the update)
    if (n_rows <= 0 || n_clusters <= 0) return 0;
    const long long kc = n_clusters < n_rows - 1 ? n_clusters : n_rows - 1;      // rows 1 .. kc meet i clusters
    long long steps = 1;                                    // row 0
    for (long long g = 0; g * 64 < kc; ++g) {               // rows 64 g + 1 .. min(64 (g + 1), kc): g + 1 steps each
        const long long hi = 64 * (g + 1) < kc ? 64 * (g + 1) : kc;
        steps += (g + 1) * (hi - 64 * g);
    }
    if (n_rows - 1 > n_clusters) steps += ((n_clusters + 63) / 64) * (n_rows - 1 - n_clusters);
    return steps;
}

void launch_wbf_pipeline(const float* boxes, const float* scores, const int32_t* cls, int B, int N, int C, float iou_thresh, int expected,
                         const NmsWork& wk, const WbfWork& ww, float* out_boxes, float* out_scores, int32_t* out_cls, int32_t* out_index,
                         int32_t* out_votes, int32_t* assign, int32_t* count, hipStream_t s)
{
    NmsPlan rec{};
    rec.B = B; rec.N = N; rec.C = C;
    const int32_t* seg_order = launch_nms_bucket_sort(boxes, scores, cls, B, N, C, wk, s, nullptr, rec);
    if (assign) {
        const long total = (long)B * N;
        hipLaunchKernelGGL(wbf_assign_clear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cls, total, assign);
    }
    hipLaunchKernelGGL(wbf_cluster_kernel, dim3(B, C), dim3(64), 0, s, scores, (const int32_t*)wk.seg_count, (const int32_t*)wk.seg_off,
                       (const int32_t*)wk.bucket, reinterpret_cast<const float4*>(wk.sbox), seg_order, N, C, iou_thresh, expected, wk.keep,
                       reinterpret_cast<float4*>(ww.wbox), ww.wscore, ww.wvotes, assign, reinterpret_cast<float4*>(ww.ofb),
                       reinterpret_cast<float4*>(ww.op), ww.os, ww.on, ww.ofounder);
    int32_t* index = out_index ? out_index : ww.windex;
    launch_nms_compact(ww.wbox, ww.wscore, cls, B, N, wk, out_boxes, out_scores, out_cls, index, count, s);
    if (out_votes)
        hipLaunchKernelGGL(wbf_votes_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, (const int32_t*)ww.wvotes, (const int32_t*)index,
                           (const int32_t*)count, N, out_votes);
}

void launch_fuse_append(const float* rec, const int32_t* offsets, int B, int C, int cap, float weight, float* lboxes, float* lscores, int32_t* lcls,
                        int32_t* state, hipStream_t st)
{
    hipLaunchKernelGGL(fuse_append_kernel, dim3(B), dim3(256), 0, st, rec, offsets, B, C, cap, weight, lboxes, lscores, lcls, state);
}

}  // namespace ynk
