// kernels_aug.hip — the pixel work of TrainTransforms / ColorTransforms (data/transforms.py:402-442) in one pass per image: uint8 BGR
// frame -> crop (RandomSampleCrop :228-307) -> mirror (RandomMirror :310-317) -> photometric chain (PhotometricDistort :350-371 =
// RandomBrightness :215-225, RandomContrast :200-212, BGR->HSV, RandomSaturation :140-150, RandomHue :153-164, HSV->BGR) -> float
// cv2.resize + letterbox (Resize :73-119) -> Normalize (:59-70) -> ToTensor (:394-398, BGR -> RGB, CHW), written straight into one
// image slot of the network input.  Built with -ffp-contract=off: every float below is one rounding of the reference's sequence.
//
// The host draws every random parameter and does all box arithmetic (yolo_nano_amd/augment.py); no draw depends on a pixel value, so
// the device sees per image only the crop rectangle, the mirror bit, the four factors (float32(u) of the float64 draws) and flags.
//
// The chain is pointwise, so it is applied to each resize TAP before interpolation: the resize then reads exactly the values the
// reference's cv2.resize reads from its materialised distorted image.  The chain is recomputed per tap rather than staged in LDS:
// the kernel is a plain streaming pass (27 VGPRs, no LDS, no scratch, 8 waves per SIMD) and measures 135 us for 32 frames of
// 500x375 to 608, inside the 140 us budget (2 % of the fp16 training step).  It is bound by the chain's ALU work, not by HBM (0.15 of
// the floor): staging distorted source rows in LDS would cut the chains per output pixel from 4 to ~1 on up-scales, and is the next
// step if the budget tightens.
//
// cv2 pieces, restated from OpenCV 4.5.x sources (modules/imgproc/src/resize.cpp, color_hsv.simd.hpp), scalar operation order:
//   float resize      resizeGeneric_ coordinate set-up, HResizeLinear<float> then VResizeLinear<float> (multiply, multiply, add; no
//                     FMA), the INTER_AREA fast path resize() switches to for an exact 2:1 reduction, and a copy when dsize == ssize.
//   RGB2HSV_f         FLT_EPSILON in both divisions, 60./x in double, the v == r / v == g order, h < 0 -> += 360 (hrange 360: hscale 1).
//   HSV2RGB_native    s == 0 -> grey; h * (6/360), fmod 6, cvFloor sector, the {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0} table.
// Whether the SIMD builds of these functions fuse a multiply and an add cannot be settled without cv2: parity with cv2 is UNPINNED,
// as for the 8-bit path of ValTransforms.  tests/train_aug_oracle.py restates the same pieces in numpy.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "yn_internal.h"

namespace ynk {

namespace {

constexpr int AUG_MAX = 32;                    // images per launch: descriptors travel by value in the kernel arguments

struct AugImg {
    const unsigned char* img;                  // uint8 [h0][w0][3] BGR frame on the device
    int w0;                                    // frame row length in pixels
    int cx, cy, cw, ch;                        // crop rectangle in the frame (the uncropped image: 0, 0, w0, h0)
    int rw, rh, left, top;                     // Resize: resized extent and its place inside the side x side square
    int flags;                                 // AUG_* bits below
    float bright, contrast, sat, hue;          // float32(u) of each fired draw
    float pad[3];                              // letterbox pad, BGR: float32(float64(mean) * 255)
};

struct AugBatchArgs {
    AugImg im[AUG_MAX];
    int side;
    float mean[3], std[3];                     // BGR, float32 (Normalize's np.array(mean, dtype=np.float32))
    float* out;                                // [n][3][side][side], channel 0 = R
};

// the pointwise photometric chain on one BGR tap, in the reference's order (PhotometricDistort.__call__ :363-370)
__device__ __forceinline__ void photometric(const AugImg& d, float& b, float& g, float& r)
{
    const int f = d.flags;
    if (f & AUG_BRIGHT) { b += d.bright; g += d.bright; r += d.bright; }                    // RandomBrightness: image += delta
    if ((f & (AUG_CONTRAST | AUG_CONTRAST_FIRST)) == (AUG_CONTRAST | AUG_CONTRAST_FIRST)) {  // pd[:-1]: RandomContrast first
        b *= d.contrast; g *= d.contrast; r *= d.contrast;
    }
    // ConvertColor BGR->HSV: cv::RGB2HSV_f::operator() (bidx 0, hrange 360 -> hscale = 360 * (1.f/360.f) = 1.0f exactly)
    float v = r, vmin = r;
    if (v < g) v = g;
    if (v < b) v = b;
    if (vmin > g) vmin = g;
    if (vmin > b) vmin = b;
    float diff = v - vmin;
    float s = diff / (fabsf(v) + FLT_EPSILON);
    diff = (float)(60.0 / (double)(diff + FLT_EPSILON));
    float h;
    if (v == r) h = (g - b) * diff;
    else if (v == g) h = (b - r) * diff + 120.0f;
    else h = (r - g) * diff + 240.0f;
    if (h < 0.0f) h += 360.0f;
    if (f & AUG_SAT) s *= d.sat;                                                              // RandomSaturation: image[:, :, 1] *= u
    if (f & AUG_HUE) {                                                                        // RandomHue: += u, then the two wraps
        h += d.hue;
        if (h > 360.0f) h -= 360.0f;
        if (h < 0.0f) h += 360.0f;
    }
    // ConvertColor HSV->BGR: cv::HSV2RGB_native (hscale = 6.f / 360.f)
    if (s == 0.0f) {
        b = g = r = v;
    } else {
        float hh = h * (6.0f / 360.0f);
        // fmod(hh, 6.f): h is in [0, 360] here (RGB2HSV_f gives [0, 360], RandomHue's two wraps keep it there), so hh is in
        // [0, 6.0000005] and fmod is hh or the exact hh - 6 (Sterbenz) — without ocml's general fmodf reduction
        if (hh >= 6.0f) hh -= 6.0f;
        const int ii = (int)hh;
        int sector = ii - (ii > hh);                                                         // cvFloor
        hh -= (float)sector;
        if ((unsigned)sector >= 6u) { sector = 0; hh = 0.0f; }
        const float t0 = v, t1 = v * (1.0f - s), t2 = v * (1.0f - s * hh), t3 = v * (1.0f - s * (1.0f - hh));
        // sector_data {{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}} = (b, g, r) indices into tab
        switch (sector) {
        case 0:  b = t1; g = t3; r = t0; break;
        case 1:  b = t1; g = t0; r = t2; break;
        case 2:  b = t3; g = t0; r = t1; break;
        case 3:  b = t0; g = t2; r = t1; break;
        case 4:  b = t0; g = t1; r = t3; break;
        default: b = t2; g = t1; r = t0; break;
        }
    }
    if ((f & (AUG_CONTRAST | AUG_CONTRAST_FIRST)) == AUG_CONTRAST) {                          // pd[1:]: RandomContrast last
        b *= d.contrast; g *= d.contrast; r *= d.contrast;
    }
}

// one tap of the cropped, mirrored, distorted image: (x, y) in the crop frame after RandomMirror
__device__ __forceinline__ void tap(const AugImg& d, int x, int y, float p[3])
{
    const int fx = d.cx + ((d.flags & AUG_MIRROR) ? d.cw - 1 - x : x);                      // image[:, ::-1] of the crop
    const unsigned char* q = d.img + ((size_t)(d.cy + y) * d.w0 + fx) * 3;
    float b = (float)q[0], g = (float)q[1], r = (float)q[2];                                 // ConvertFromInts
    photometric(d, b, g, r);
    p[0] = b; p[1] = g; p[2] = r;
}

__global__ __launch_bounds__(256) void train_aug_kernel(AugBatchArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int side = a.side;
    if (i >= side * side) return;
    const AugImg& d = a.im[blockIdx.y];
    const int y = i / side, x = i - y * side;
    const int ry = y - d.top, rx = x - d.left;
    float v[3];
    if (ry >= 0 && ry < d.rh && rx >= 0 && rx < d.rw) {
        if (d.cw == d.rw && d.ch == d.rh) {
            // resize(): dsize == ssize -> copy; also Resize's square case h0 == size (image_ = image)
            tap(d, rx, ry, v);
        } else if (d.cw == 2 * d.rw && d.ch == 2 * d.rh) {
            // resize(): INTER_LINEAR with iscale 2 x 2 runs resizeAreaFast_: sum = 0; sum += S[ofs0] + S[ofs1] + S[ofs2] + S[ofs3]
            // (ofs in (sy, sx) order), D = sum * (1.f / 4)
            float p00[3], p01[3], p10[3], p11[3];
            tap(d, 2 * rx, 2 * ry, p00); tap(d, 2 * rx + 1, 2 * ry, p01);
            tap(d, 2 * rx, 2 * ry + 1, p10); tap(d, 2 * rx + 1, 2 * ry + 1, p11);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float sum = 0.0f;
                sum += p00[c] + p01[c] + p10[c] + p11[c];
                v[c] = sum * 0.25f;
            }
        } else {
            // resizeGeneric_ set-up (ksize 2): scale = 1. / inv_scale in double, fx = (float)((dx + 0.5) * scale - 0.5), sx = cvFloor
            const double scx = 1.0 / ((double)d.rw / (double)d.cw), scy = 1.0 / ((double)d.rh / (double)d.ch);
            float fx = (float)(((double)rx + 0.5) * scx - 0.5), fy = (float)(((double)ry + 0.5) * scy - 0.5);
            int sx = (int)floorf(fx), sy = (int)floorf(fy);
            fx -= (float)sx; fy -= (float)sy;
            if (sx < 0) { fx = 0.0f; sx = 0; }                                                // xmin border: alpha = (1, 0)
            const bool xmax = sx + 1 >= d.cw;                                                 // dx >= xmax: D = S[sx] * ONE
            if (xmax) { fx = 0.0f; sx = d.cw - 1; }
            const float a0 = 1.0f - fx, a1 = fx;                                              // cbuf[0] = 1.f - fx; cbuf[1] = fx
            const float b0 = 1.0f - fy, b1 = fy;                                              // y weights kept; rows clipped instead
            const int r0 = min(max(sy, 0), d.ch - 1), r1 = min(max(sy + 1, 0), d.ch - 1);
            float h0[3], h1[3];
            {
                float p[3];
                tap(d, sx, r0, p);
                if (xmax) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) h0[c] = p[c];
                } else {
                    float q[3];
                    tap(d, sx + 1, r0, q);
#pragma unroll
                    for (int c = 0; c < 3; ++c) h0[c] = p[c] * a0 + q[c] * a1;               // HResizeLinear: S0[sx]*a0 + S0[sx+cn]*a1
                }
            }
            if (r1 == r0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) h1[c] = h0[c];
            } else {
                float p[3];
                tap(d, sx, r1, p);
                if (xmax) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) h1[c] = p[c];
                } else {
                    float q[3];
                    tap(d, sx + 1, r1, q);
#pragma unroll
                    for (int c = 0; c < 3; ++c) h1[c] = p[c] * a0 + q[c] * a1;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = h0[c] * b0 + h1[c] * b1;                       // VResizeLinear: S0[x]*b0 + S1[x]*b1
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = d.pad[c];                                          // np.ones([s, s, 3]) * mean, as float32
    }
    float* out = a.out + (size_t)blockIdx.y * 3 * side * side;
    const size_t plane = (size_t)side * side;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = v[c] / 255.0f;                                                              // Normalize: /= 255.; -= mean; /= std
        t = t - a.mean[c];
        t = t / a.std[c];
        out[(size_t)(2 - c) * plane + i] = t;                                                 // ToTensor: BGR -> RGB, HWC -> CHW
    }
}

}  // namespace

void launch_train_aug_batch(int n, const unsigned char* const* imgs, const int* geom, const float* photo, int side, const float* mean,
                            const float* stdv, float* out, hipStream_t s)
{
    for (int i0 = 0; i0 < n; i0 += AUG_MAX) {
        const int m = n - i0 < AUG_MAX ? n - i0 : AUG_MAX;
        AugBatchArgs b{};
        for (int i = 0; i < m; ++i) {
            const int* g = geom + (size_t)(i0 + i) * AUG_GEOM;
            const float* p = photo + (size_t)(i0 + i) * AUG_PHOTO;
            AugImg& d = b.im[i];
            d.img = imgs[i0 + i]; d.w0 = g[1];
            d.cx = g[2]; d.cy = g[3]; d.cw = g[4]; d.ch = g[5];
            d.rw = g[7]; d.rh = g[8]; d.left = g[9]; d.top = g[10];
            d.flags = (g[11] & ~AUG_MIRROR) | (g[6] ? AUG_MIRROR : 0);
            d.bright = p[0]; d.contrast = p[1]; d.sat = p[2]; d.hue = p[3];
            d.pad[0] = p[4]; d.pad[1] = p[5]; d.pad[2] = p[6];
        }
        b.side = side; b.out = out + (size_t)i0 * 3 * side * side;
        for (int c = 0; c < 3; ++c) { b.mean[c] = mean[c]; b.std[c] = stdv[c]; }
        hipLaunchKernelGGL(train_aug_kernel, dim3((side * side + 255) / 256, m), dim3(256), 0, s, b);
    }
}

}  // namespace ynk
