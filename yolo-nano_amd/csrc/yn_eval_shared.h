// yn_eval_shared.h — what the two metric files (kernels_eval.hip: VOC mAP, kernels_coco.hip: COCO box AP) have in common: the
// evaluators' un-letterboxing of a detection box, a bitonic sort of unique keys, a block scan, a lower bound and the host-side error
// check (device memory is owned by DevBuf members, yn_devbuf.h).  Both files are built with -ffp-contract=off.  Everything here is `static` or a template: each file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace ynk {
namespace evs {

// bboxes -= offset; bboxes /= scale; bboxes *= size (vocapi_evaluator.py:72-74, cocoapi_evaluator.py:85-87): a float32 array with
// float64 operands, so each step is a float64 operation rounded to float32.  g = w0, h0, rw, rh, left, top, side of the image.
__device__ __forceinline__ void unletterbox(const float* __restrict__ r, const int32_t* __restrict__ g, float out[4])
{
    const double side = (double)g[6];
    const double off[2] = {(double)g[4] / side, (double)g[5] / side};   // ValTransforms.geometry: left/h, top/w
    const double sc[2] = {(double)g[2] / side, (double)g[3] / side};    //                         w/h, h/w (1. on the long side)
    const double size[2] = {(double)g[0], (double)g[1]};
    for (int c = 0; c < 4; ++c) {
        float v = r[c];
        v = (float)((double)v - off[c & 1]);
        v = (float)((double)v / sc[c & 1]);
        v = (float)((double)v * size[c & 1]);
        out[c] = v;
    }
}

// image b of record i: offsets[b] <= i < offsets[b+1]
__device__ __forceinline__ int image_of(const int32_t* __restrict__ offsets, int B, int64_t i)
{
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- bitonic sort of unique keys (ascending); K is uint64_t or a struct with operator> ------------------------------------------
constexpr int SORT_LOCAL = 2048;               // keys per workgroup in the LDS stages

template <typename K>
__device__ __forceinline__ void cswap(K& a, K& b, bool up)
{
    if ((a > b) == up) { const K t = a; a = b; b = t; }
}

// kfull != 0: sort each 2048-key tile completely (every stage k <= 2048); otherwise finish stage k (its steps j <= 1024) in LDS
template <typename K>
__global__ __launch_bounds__(1024) void bitonic_local_kernel(K* __restrict__ a, int64_t k, int kfull)
{
    __shared__ K s[SORT_LOCAL];
    const int64_t base = (int64_t)blockIdx.x * SORT_LOCAL;
    const int t = threadIdx.x;
    s[t] = a[base + t];
    s[t + 1024] = a[base + t + 1024];
    __syncthreads();
    const int64_t k0 = kfull ? 2 : k, k1 = kfull ? SORT_LOCAL : k;
    for (int64_t kk = k0; kk <= k1; kk <<= 1) {
        for (int j = (int)(kk / 2 < 1024 ? kk / 2 : 1024); j > 0; j >>= 1) {
            const int i = 2 * t - (t & (j - 1));
            cswap(s[i], s[i + j], ((base + i) & kk) == 0);
            __syncthreads();
        }
    }
    a[base + t] = s[t];
    a[base + t + 1024] = s[t + 1024];
}

template <typename K>
__global__ void bitonic_global_kernel(K* __restrict__ a, int64_t j, int64_t k, int64_t half)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= half) return;
    const int64_t i = 2 * t - (t & (j - 1));
    const K x = a[i], y = a[i + j];
    const bool up = (i & k) == 0;
    if ((x > y) == up) { a[i] = y; a[i + j] = x; }
}

template <typename K>
static void bitonic_sort(K* a, int64_t npow, hipStream_t s)      // npow: a power of two >= SORT_LOCAL
{
    const int tiles = (int)(npow / SORT_LOCAL);
    hipLaunchKernelGGL(bitonic_local_kernel<K>, dim3(tiles), dim3(1024), 0, s, a, (int64_t)0, 1);
    for (int64_t k = 2 * SORT_LOCAL; k <= npow; k <<= 1) {
        for (int64_t j = k / 2; j >= SORT_LOCAL; j >>= 1)
            hipLaunchKernelGGL(bitonic_global_kernel<K>, dim3((unsigned)((npow / 2 + 255) / 256)), dim3(256), 0, s, a, j, k, npow / 2);
        hipLaunchKernelGGL(bitonic_local_kernel<K>, dim3(tiles), dim3(1024), 0, s, a, k, 0);
    }
}

template <typename K>
__device__ __forceinline__ int64_t lower_bound(const K* a, int64_t n, K key)   // first index whose element is not below key
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// position of this thread's flagged element among the flagged elements of a 256-thread workgroup in thread order, and their
// number; wsum holds 4 ints
__device__ __forceinline__ int ordered_rank(bool flag, int* wsum, int& total)
{
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = wsum[w];
        if (w < wv) base += c;
        total += c;
    }
    __syncthreads();                            // wsum may be written again
    return base + r;
}

// inclusive scan over the 256 threads of a workgroup in thread order; lds holds 4 elements
template <typename T, typename Op>
__device__ __forceinline__ T block_scan_incl(T v, Op op, T* lds)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v = op(u, v);
    }
    if (lane == 63) lds[wv] = v;
    __syncthreads();
    T pre = lds[0];
    for (int w = 1; w < wv; ++w) pre = op(pre, lds[w]);
    if (wv > 0) v = op(pre, v);
    __syncthreads();
    return v;
}

// ---- host plumbing ----------------------------------------------------------------------------------------------------------------
#define EVCHK(expr)                                                                                         \
    do {                                                                                                    \
        const hipError_t e_ = (hipError_t)(expr);      /* a HIP call, or a DevBuf growth (its int is a hipError_t) */ \
        if (e_ != hipSuccess) { err = std::string(#expr " failed: ") + hipGetErrorString(e_); return 1; }   \
    } while (0)

}  // namespace evs
}  // namespace ynk
