// yn_prep.h — the per-pixel body of ValTransforms on the device, shared by the kernels that write the network's input from uint8 frames:
// preprocess_kernel / preprocess_batch_kernel / preprocess_batch_rect_kernel (kernels_post.hip) and slice_tile_kernel (kernels_slice.hip).
// One definition, so that every one of them gives the same bits.  Both files are built with -ffp-contract=off.
//
// ValTransforms (data/transforms.py:59-70, 73-119, 394-398, 445-458): uint8 HWC BGR image -> letterbox resize (cv2.resize INTER_LINEAR,
// 8-bit fixed point: modules/imgproc/src/resize.cpp, restated in oracle/preprocess.py — the oracle's header says why this path's parity is
// UNPINNED) -> mean padding -> /255, -mean, /std -> RGB CHW float32.  mode: 0 copy, 1 exact 2:1 reduction (2x2 box), 2 linear.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace ynk {

struct PrepArgs {
    const unsigned char* img; int h0, w0;       // source: its top-left pixel and the extent the resize arithmetic sees
    int pitch;                                  // pixels from one source row to the next: w0 for a whole image, the frame's width for a tile read in place
    int rw, rh, left, top, side, mode;          // resized extent, placement inside the side x side square
    float mean[3], std[3];                      // BGR order, as the reference passes them
    float* out;                                 // [3][side][side], channel 0 = R
};

__host__ __device__ inline int prep_mode(int h0, int w0, int rw, int rh) { return (rw == w0 && rh == h0) ? 0 : ((w0 == 2 * rw && h0 == 2 * rh) ? 1 : 2); }

// the pixel at (rx, ry) of the resized extent's frame, BGR, before Normalize (outside [0, rw) x [0, rh): the pad value)
__device__ __forceinline__ void prep_sample(const PrepArgs& a, int ry, int rx, float v[3])
{
    if (ry >= 0 && ry < a.rh && rx >= 0 && rx < a.rw) {
        int u[3];
        if (a.mode == 0) {
            const unsigned char* p = a.img + ((size_t)ry * a.pitch + rx) * 3;
            u[0] = p[0]; u[1] = p[1]; u[2] = p[2];
        } else if (a.mode == 1) {
            const unsigned char* p = a.img + ((size_t)(2 * ry) * a.pitch + 2 * rx) * 3;
            const unsigned char* q = p + (size_t)a.pitch * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c] = (p[c] + p[3 + c] + q[c] + q[3 + c] + 2) >> 2;
        } else {
            // resizeGeneric_ (ksize 2): fx = (float)((dx + 0.5) * scale - 0.5), scale = 1 / (dsize / ssize) in double
            const double scx = 1.0 / ((double)a.rw / (double)a.w0), scy = 1.0 / ((double)a.rh / (double)a.h0);
            float fx = (float)(((double)rx + 0.5) * scx - 0.5), fy = (float)(((double)ry + 0.5) * scy - 0.5);
            int sx = (int)floorf(fx), sy = (int)floorf(fy);
            fx -= (float)sx; fy -= (float)sy;
            if (sx < 0) { fx = 0.0f; sx = 0; }
            if (sx >= a.w0 - 1) { fx = 0.0f; sx = a.w0 - 1; }
            const int a0 = __float2int_rn((1.0f - fx) * 2048.0f), a1 = __float2int_rn(fx * 2048.0f);   // cvRound -> short
            const int b0 = __float2int_rn((1.0f - fy) * 2048.0f), b1 = __float2int_rn(fy * 2048.0f);
            const int sx1 = min(sx + 1, a.w0 - 1);
            const int r0 = min(max(sy, 0), a.h0 - 1), r1 = min(max(sy + 1, 0), a.h0 - 1);
            const unsigned char* p0 = a.img + (size_t)r0 * a.pitch * 3;
            const unsigned char* p1 = a.img + (size_t)r1 * a.pitch * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s0 = p0[sx * 3 + c] * a0 + p0[sx1 * 3 + c] * a1;          // HResizeLinear (scale 2048)
                const int s1 = p1[sx * 3 + c] * a0 + p1[sx1 * 3 + c] * a1;
                const int r = (((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2;   // VResizeLinear 8u
                u[c] = min(max(r, 0), 255);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)u[c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = a.mean[c] * 255.0f;                     // Resize.mean = [v * 255 for v in mean]
    }
}

// Normalize on channel c (BGR index) of one pixel: image /= 255.; -= mean; /= std, each step rounded
__device__ __forceinline__ float prep_normalise(const PrepArgs& a, int c, float v)
{
    float t = v / 255.0f;
    t = t - a.mean[c];
    t = t / a.std[c];
    return t;
}

// the pixel at (rx, ry) of the resized extent's frame (outside [0, rw) x [0, rh): pad) -> element i of the three output planes
__device__ __forceinline__ void preprocess_at(const PrepArgs& a, int ry, int rx, size_t plane, int i)
{
    float v[3];
    prep_sample(a, ry, rx, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) a.out[(size_t)(2 - c) * plane + i] = prep_normalise(a, c, v[c]);      // ToTensor: BGR -> RGB, HWC -> CHW
}

}  // namespace ynk
