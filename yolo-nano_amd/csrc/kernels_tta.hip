// kernels_tta.hip — test-time augmentation for whole batches (utils/misc.py:90-148, TestTimeAugmentation): the two kernels yn_tta_infer
// puts around the handle's own yn_infer, and the resize kernel on its own (yn_resize_batch; train.py:202-208's F.interpolate).
//
//   tta_resize_flip_kernel   utils/misc.py:108-111 (F.interpolate, mode 'bilinear', align_corners False) + :120 (torch.flip(x, [-1])),
//                            for every image of the batch: image 2b = resize of image b, image 2b + 1 = its horizontal mirror
//   tta_append_kernel        :114-118 and :121-130: a forward's kept detections go to the end of their image's merge list, the flipped
//                            forward's boxes mirrored back (:126, bboxes[:, 0::2] = 1.0 - bboxes[:, 2::-2])
//
// The resize arithmetic is DEFINED here (Test-time augmentation), because torch's own bilinear kernel gives different bits with
// different thread counts.  Per axis, with scale = (float)S0 / (float)s computed ONCE on the host:
//     src = max(fmaf(scale, d + 0.5f, -0.5f), 0)      one rounding
//     i0 = (int)src, i1 = i0 + (i0 < S0 - 1), l1 = src - i0, l0 = 1 - l1
//     v = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)      every multiply and add rounded on its own
// The value operations are written with __fmul_rn / __fadd_rn so that no compiler setting can contract them (the file is built with
// -ffp-contract=off as well).  s == S0 is a copy of the bits (the reference passes x itself, :106-107), not 1 * a + 0 * b, which would
// turn -0 into +0 and an infinity into a NaN.
//
// Both kernels stream: a thread of the resize produces four neighbouring pixels of a row and stores them as 16 bytes (twice with the
// mirror, from the same registers - every tap is read once); neighbouring threads read neighbouring taps.
#include <hip/hip_runtime.h>

#include "yn_internal.h"

namespace ynk {

namespace {

struct Tap { int i0, i1; float l0, l1; };

__device__ __forceinline__ Tap tta_tap(int d, float scale, int S0)
{
    const float src = fmaxf(__fmaf_rn(scale, (float)d + 0.5f, -0.5f), 0.0f);
    int i0 = (int)src;
    i0 = i0 < S0 - 1 ? i0 : S0 - 1;                         // never taken for d < s (src < S0 - 1/2); keeps every read inside the row
    Tap t;
    t.i0 = i0;
    t.i1 = i0 + (i0 < S0 - 1 ? 1 : 0);
    t.l1 = __fsub_rn(src, (float)i0);
    t.l0 = __fsub_rn(1.0f, t.l1);
    return t;
}

// x [planes / 3][3][S0][S0] -> out [(flip ? 2 : 1) * planes / 3][3][s][s]; VEC: s % 4 == 0 and both pointers 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void tta_resize_flip_kernel(const float* __restrict__ x, float* __restrict__ out, int planes, int S0, int s,
                                                              float scale, int flip)
{
    // workgroup = 32 quads x 8 rows of one plane: no index division, and a row's 32 lanes store 512 contiguous bytes
    const int q = blockIdx.x * 32 + threadIdx.x;
    const int y = blockIdx.y * 8 + threadIdx.y;
    const int p = blockIdx.z;                               // image * 3 + channel
    if (q >= ((s + 3) >> 2) || y >= s || p >= planes) return;
    const int b = p / 3, c = p - 3 * b;
    const int x0 = q * 4;
    const float* src = x + (size_t)p * S0 * S0;
    const size_t oplane = (size_t)s * s;
    float* o0 = out + ((size_t)(flip ? 2 * b : b) * 3 + c) * oplane + (size_t)y * s;
    float* o1 = o0 + 3 * oplane;                            // the same row of the mirrored image (flip only)
    float v[4];
    if (s == S0) {
        if (VEC) {
            const float4 t = *reinterpret_cast<const float4*>(src + (size_t)y * S0 + x0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = src[(size_t)y * S0 + (x0 + k < s ? x0 + k : s - 1)];
        }
    } else {
        const Tap ty = tta_tap(y, scale, S0);
        const float* r0 = src + (size_t)ty.i0 * S0;
        const float* r1 = src + (size_t)ty.i1 * S0;
        Tap tx[4];
        float ta[4], tb[4], tc[4], td[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                       // all sixteen loads are issued before the first use
            tx[k] = tta_tap(x0 + k < s ? x0 + k : s - 1, scale, S0);
            ta[k] = r0[tx[k].i0]; tb[k] = r0[tx[k].i1];
            tc[k] = r1[tx[k].i0]; td[k] = r1[tx[k].i1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float top = __fadd_rn(__fmul_rn(tx[k].l0, ta[k]), __fmul_rn(tx[k].l1, tb[k]));
            const float bot = __fadd_rn(__fmul_rn(tx[k].l0, tc[k]), __fmul_rn(tx[k].l1, td[k]));
            v[k] = __fadd_rn(__fmul_rn(ty.l0, top), __fmul_rn(ty.l1, bot));
        }
    }
    if (VEC) {
        *reinterpret_cast<float4*>(o0 + x0) = make_float4(v[0], v[1], v[2], v[3]);
        if (flip) *reinterpret_cast<float4*>(o1 + (s - 4 - x0)) = make_float4(v[3], v[2], v[1], v[0]);      // out[..., j] = resized[..., s - 1 - j]
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x0 + k < s) {
                o0[x0 + k] = v[k];
                if (flip) o1[s - 1 - x0 - k] = v[k];
            }
        }
    }
}

// One workgroup per image b.  The forward's outputs are yn_infer's: boxes [nb][N][4], scores / cls [nb][N], count [nb] (negative: the
// range mark, -1 - kept); with flip, image 2b is the plain and 2b + 1 the mirrored forward of b.  state = int32 [MERGE_STATE + max_batch]:
// the merge lists' flag words and the cursor of each image (yn_internal.h).  fstart [forwards][bstride]: where each forward's rows start
// in each image's list.  Rows past `cap` are counted and not written.
__global__ __launch_bounds__(256) void tta_append_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ cls,
                                                         const int32_t* __restrict__ count, int N, int flip, int cap, int bstride, int fwd,
                                                         float* __restrict__ lboxes, float* __restrict__ lscores, int32_t* __restrict__ lcls,
                                                         int32_t* __restrict__ state, int32_t* __restrict__ fstart)
{
    const int b = blockIdx.x;
    const int img0 = flip ? 2 * b : b;
    const int c0 = count[img0];
    const int c1 = flip ? count[img0 + 1] : 0;
    const bool bad = c0 < 0 || c1 < 0;
    int n0 = c0 < 0 ? -1 - c0 : c0, n1 = c1 < 0 ? -1 - c1 : c1;
    n0 = n0 < N ? n0 : N;
    n1 = n1 < N ? n1 : N;
    const int base = state[MERGE_STATE + b];
    __syncthreads();                                        // every thread holds the cursor before thread 0 moves it
    if (threadIdx.x == 0) {
        const int end = base + n0 + n1;
        state[MERGE_STATE + b] = end;
        fstart[(size_t)fwd * bstride + b] = base;
        if (flip) fstart[(size_t)(fwd + 1) * bstride + b] = base + n0;
        if (end > cap) { atomicOr(&state[0], 1); atomicMax(&state[1], end); }
        if (bad) atomicOr(&state[2], 1);
    }
    for (int i = threadIdx.x; i < n0 + n1; i += 256) {
        const int dst = base + i;
        if (dst >= cap) break;
        const bool mirrored = i >= n0;
        const size_t src = (size_t)(mirrored ? img0 + 1 : img0) * N + (mirrored ? i - n0 : i);
        float4 bx = *reinterpret_cast<const float4*>(boxes + src * 4);
        if (mirrored) {                                     // bboxes[:, 0::2] = 1.0 - bboxes[:, 2::-2] in float32
            const float x1 = __fsub_rn(1.0f, bx.z), x2 = __fsub_rn(1.0f, bx.x);
            bx.x = x1; bx.z = x2;
        }
        const size_t d = (size_t)b * cap + dst;
        *reinterpret_cast<float4*>(lboxes + d * 4) = bx;
        lscores[d] = scores[src];
        lcls[d] = cls[src];
    }
}

}  // namespace

void launch_tta_resize(const float* x, int B, int S0, int s, int flip, float* out, hipStream_t st)
{
    if (B <= 0) return;
    const int planes = B * 3;                               // grid z: at most 65535 planes (checked by the caller)
    const dim3 blocks((((s + 3) >> 2) + 31) / 32, (s + 7) / 8, planes), threads(32, 8);
    const float scale = (float)S0 / (float)s;               // one IEEE division on the host, the same value for every pixel
    const bool vec = (s % 4) == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0 && (s != S0 || (S0 % 4) == 0);
    if (vec) hipLaunchKernelGGL(tta_resize_flip_kernel<true>, blocks, threads, 0, st, x, out, planes, S0, s, scale, flip);
    else     hipLaunchKernelGGL(tta_resize_flip_kernel<false>, blocks, threads, 0, st, x, out, planes, S0, s, scale, flip);
}

void launch_tta_append(const float* boxes, const float* scores, const int32_t* cls, const int32_t* count, int B, int N, int flip, int cap,
                       int bstride, int fwd, float* lboxes, float* lscores, int32_t* lcls, int32_t* state, int32_t* fstart, hipStream_t st)
{
    if (B <= 0) return;
    hipLaunchKernelGGL(tta_append_kernel, dim3(B), dim3(256), 0, st, boxes, scores, cls, count, N, flip, cap, bstride, fwd, lboxes, lscores, lcls,
                       state, fstart);
}

}  // namespace ynk
