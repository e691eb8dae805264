// kernels_aug.hip — the pixel work of TrainTransforms / ColorTransforms (data/transforms.py:402-442) in one pass per image: uint8 BGR
// frame -> crop (RandomSampleCrop :228-307) -> mirror (RandomMirror :310-317) -> photometric chain (PhotometricDistort :350-371 =
// RandomBrightness :215-225, RandomContrast :200-212, BGR->HSV, RandomSaturation :140-150, RandomHue :153-164, HSV->BGR) -> float
// cv2.resize + letterbox (Resize :73-119) -> Normalize (:59-70) -> ToTensor (:394-398, BGR -> RGB, CHW), written straight into one
// image slot of the network input.  Built with -ffp-contract=off: every float below is one rounding of the reference's sequence.
// The second kernel, mosaic_aug_kernel, does the same for a mosaic sample (data/voc.py:140-211 load_mosaic + ColorTransforms): four
// frames, their 8-bit cv2.resize and the canvas they are pasted into, all computed per tap of the canvas's Resize (further below).
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

// the pointwise photometric chain on one BGR tap, in the reference's order (PhotometricDistort.__call__ :363-370); D = AugImg or MosImg
template <class D>
__device__ __forceinline__ void photometric(const D& d, float& b, float& g, float& r)
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

// cv2.resize of a float sw x sh image to dw x dh, INTER_LINEAR, at destination pixel (rx, ry); tap(x, y, p) reads source pixel (x, y)
// as BGR floats and tap.quad(x, y, ...) the 2 x 2 block at (x, y).  The single-image pass and the mosaic pass share this body and
// differ in where a tap comes from.
template <class Tap>
__device__ __forceinline__ void resize_f32(const Tap& tap, int sw, int sh, int dw, int dh, int rx, int ry, float v[3])
{
    if (sw == dw && sh == dh) {
        // resize(): dsize == ssize -> copy; also Resize's square case h0 == size (image_ = image)
        tap(rx, ry, v);
    } else if (sw == 2 * dw && sh == 2 * dh) {
        // resize(): INTER_LINEAR with iscale 2 x 2 runs resizeAreaFast_: sum = 0; sum += S[ofs0] + S[ofs1] + S[ofs2] + S[ofs3]
        // (ofs in (sy, sx) order), D = sum * (1.f / 4)
        float p00[3], p01[3], p10[3], p11[3];
        tap.quad(2 * rx, 2 * ry, p00, p01, p10, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float sum = 0.0f;
            sum += p00[c] + p01[c] + p10[c] + p11[c];
            v[c] = sum * 0.25f;
        }
    } else {
        // resizeGeneric_ set-up (ksize 2): scale = 1. / inv_scale in double, fx = (float)((dx + 0.5) * scale - 0.5), sx = cvFloor
        const double scx = 1.0 / ((double)dw / (double)sw), scy = 1.0 / ((double)dh / (double)sh);
        float fx = (float)(((double)rx + 0.5) * scx - 0.5), fy = (float)(((double)ry + 0.5) * scy - 0.5);
        int sx = (int)floorf(fx), sy = (int)floorf(fy);
        fx -= (float)sx; fy -= (float)sy;
        if (sx < 0) { fx = 0.0f; sx = 0; }                                                    // xmin border: alpha = (1, 0)
        const bool xmax = sx + 1 >= sw;                                                       // dx >= xmax: D = S[sx] * ONE
        if (xmax) { fx = 0.0f; sx = sw - 1; }
        const float a0 = 1.0f - fx, a1 = fx;                                                  // cbuf[0] = 1.f - fx; cbuf[1] = fx
        const float b0 = 1.0f - fy, b1 = fy;                                                  // y weights kept; rows clipped instead
        const int r0 = min(max(sy, 0), sh - 1), r1 = min(max(sy + 1, 0), sh - 1);
        float h0[3], h1[3];
        {
            float p[3];
            tap(sx, r0, p);
            if (xmax) {
#pragma unroll
                for (int c = 0; c < 3; ++c) h0[c] = p[c];
            } else {
                float q[3];
                tap(sx + 1, r0, q);
#pragma unroll
                for (int c = 0; c < 3; ++c) h0[c] = p[c] * a0 + q[c] * a1;                   // HResizeLinear: S0[sx]*a0 + S0[sx+cn]*a1
            }
        }
        if (r1 == r0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) h1[c] = h0[c];
        } else {
            float p[3];
            tap(sx, r1, p);
            if (xmax) {
#pragma unroll
                for (int c = 0; c < 3; ++c) h1[c] = p[c];
            } else {
                float q[3];
                tap(sx + 1, r1, q);
#pragma unroll
                for (int c = 0; c < 3; ++c) h1[c] = p[c] * a0 + q[c] * a1;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = h0[c] * b0 + h1[c] * b1;                           // VResizeLinear: S0[x]*b0 + S1[x]*b1
    }
}

// Normalize (/= 255.; -= mean; /= std) and ToTensor (BGR -> RGB, HWC -> CHW) of output pixel i of one image slot
__device__ __forceinline__ void store_normalized(const float v[3], const float mean[3], const float stdv[3], float* out, size_t plane, int i)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = v[c] / 255.0f;
        t = t - mean[c];
        t = t / stdv[c];
        out[(size_t)(2 - c) * plane + i] = t;
    }
}

struct AugTap {
    const AugImg& d;
    __device__ __forceinline__ void operator()(int x, int y, float p[3]) const { tap(d, x, y, p); }
    __device__ __forceinline__ void quad(int x, int y, float p00[3], float p01[3], float p10[3], float p11[3]) const
    {
        tap(d, x, y, p00); tap(d, x + 1, y, p01);
        tap(d, x, y + 1, p10); tap(d, x + 1, y + 1, p11);
    }
};

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
        resize_f32(AugTap{d}, d.cw, d.ch, d.rw, d.rh, rx, ry, v);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = d.pad[c];                                          // np.ones([s, s, 3]) * mean, as float32
    }
    const size_t plane = (size_t)side * side;
    store_normalized(v, a.mean, a.std, a.out + (size_t)blockIdx.y * 3 * plane, plane, i);
}

// ---- mosaic (data/voc.py:140-211 load_mosaic, then ColorTransforms) ----------------------------------------------------------------
// The reference resizes four uint8 frames with cv2's 8-bit INTER_LINEAR, pastes a rectangle of each into a float64 2M x 2M canvas
// filled with mean * 255, and hands the canvas to ColorTransforms: ConvertFromInts (float32), the photometric chain on the whole
// canvas (the fill included), RandomMirror, the float Resize of the square canvas to side, Normalize, ToTensor.  Here the canvas
// is never built: a canvas tap is either one pixel of a frame's 8-bit resize, computed from its four source bytes, or the fill,
// and the chain of the fill is computed once per workgroup (it is three constants per mosaic) and shared through LDS.
constexpr int MOS_MAX = 14;                    // mosaics per launch: 14 descriptors of 288 bytes fit the 4 KB of kernel arguments

struct MosFrame {
    const unsigned char* img;                  // uint8 [h0][w0][3] BGR frame on the device
    int h0, w0;                                // frame shape
    int rw, rh;                                // cv2.resize extent (int(w0 * r), int(h0 * r)); = w0, h0 when r == 1
    int x1a, y1a, x2a, y2a;                    // canvas rectangle mosaic_img[y1a:y2a, x1a:x2a]
    int dx, dy;                                // canvas -> resized frame: x1b - x1a, y1b - y1a (= -padw, -padh)
    double scx, scy;                           // resizeGeneric_'s scale per axis: 1. / (rw / w0), 1. / (rh / h0) in double
};

struct MosImg {
    MosFrame f[4];
    int flags;                                 // AUG_* bits, AUG_MIRROR included
    float bright, contrast, sat, hue;
    float fill[3];                             // canvas fill, BGR: float32(float64(mean) * 255)
};

struct MosBatchArgs {
    MosImg im[MOS_MAX];
    int side, m2;                              // output side; canvas side 2M
    float mean[3], std[3];
    float* out;
};
static_assert(sizeof(MosBatchArgs) <= 4096, "mosaic descriptors must fit HIP's kernel-argument limit");

// one axis of resizeGeneric_'s set-up for the 8-bit path (ksize 2): the two source indices and their fixed-point weights
struct Axis8 { int i0, i1, w0, w1; };

__device__ __forceinline__ Axis8 axis_x8(double scale, int src, int dx)
{
    float fx = (float)(((double)dx + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.0f; sx = 0; }
    if (sx >= src - 1) { fx = 0.0f; sx = src - 1; }
    return {sx, min(sx + 1, src - 1), __float2int_rn((1.0f - fx) * 2048.0f), __float2int_rn(fx * 2048.0f)};   // cvRound -> short
}

__device__ __forceinline__ Axis8 axis_y8(double scale, int src, int dy)
{
    float fy = (float)(((double)dy + 0.5) * scale - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;                                                                         // weights kept; the rows are clipped
    return {min(max(sy, 0), src - 1), min(max(sy + 1, 0), src - 1), __float2int_rn((1.0f - fy) * 2048.0f), __float2int_rn(fy * 2048.0f)};
}

// HResizeLinear / VResizeLinear<uchar> in fixed point for one pixel (kernels_post.hip's preprocess_pixel has the same body)
__device__ __forceinline__ void frame_linear_u8(const MosFrame& f, const Axis8& ax, const Axis8& ay, float& b, float& g, float& r)
{
    const unsigned char* p0 = f.img + (size_t)ay.i0 * f.w0 * 3;
    const unsigned char* p1 = f.img + (size_t)ay.i1 * f.w0 * 3;
    int u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // every factor is below 2^16 (bytes, weights <= 2048, s >> 4 <= 32640): the 24-bit multiplier is exact and full rate
        const int s0 = __mul24(p0[ax.i0 * 3 + c], ax.w0) + __mul24(p0[ax.i1 * 3 + c], ax.w1);   // HResizeLinear (scale 2048)
        const int s1 = __mul24(p1[ax.i0 * 3 + c], ax.w0) + __mul24(p1[ax.i1 * 3 + c], ax.w1);
        const int t = ((__mul24(ay.w0, s0 >> 4) >> 16) + (__mul24(ay.w1, s1 >> 4) >> 16) + 2) >> 2;   // VResizeLinear 8u
        u[c] = min(max(t, 0), 255);
    }
    b = (float)u[0]; g = (float)u[1]; r = (float)u[2];                                       // ConvertFromInts
}

__device__ __forceinline__ bool frame_is_copy(const MosFrame& f) { return f.rw == f.w0 && f.rh == f.h0; }
__device__ __forceinline__ bool frame_is_area(const MosFrame& f) { return f.w0 == 2 * f.rw && f.h0 == 2 * f.rh; }

// pixel (px, py) of cv2.resize(frame, (rw, rh)) for a uint8 frame, 8-bit INTER_LINEAR: a copy when dsize == ssize, the 2 x 2
// INTER_AREA fast path for an exact 2:1 reduction, else the fixed-point linear pass
__device__ __forceinline__ void frame_pixel_u8(const MosFrame& f, int px, int py, float& b, float& g, float& r)
{
    if (frame_is_copy(f)) {
        const unsigned char* p = f.img + ((size_t)py * f.w0 + px) * 3;
        b = (float)p[0]; g = (float)p[1]; r = (float)p[2];
    } else if (frame_is_area(f)) {
        const unsigned char* p = f.img + ((size_t)(2 * py) * f.w0 + 2 * px) * 3;
        const unsigned char* q = p + (size_t)f.w0 * 3;
        b = (float)((p[0] + p[3] + q[0] + q[3] + 2) >> 2);
        g = (float)((p[1] + p[4] + q[1] + q[4] + 2) >> 2);
        r = (float)((p[2] + p[5] + q[2] + q[5] + 2) >> 2);
    } else {
        frame_linear_u8(f, axis_x8(f.scx, f.w0, px), axis_y8(f.scy, f.h0, py), b, g, r);
    }
}

// the source of the mosaic pass's taps: canvas pixel (x, y) after RandomMirror and the photometric chain
struct MosTap {
    const MosImg& d;
    int m2;
    const float* fillc;                                                                      // the chain of the fill (LDS)

    __device__ __forceinline__ int column(int x) const { return (d.flags & AUG_MIRROR) ? m2 - 1 - x : x; }   // image[:, ::-1]

    // the frame whose canvas rectangle holds (cx, y): frames 0..3 in order, a later paste overwrites; -1 = the fill
    __device__ __forceinline__ int frame_at(int cx, int y) const
    {
        int k = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const MosFrame& f = d.f[j];
            if (cx >= f.x1a && cx < f.x2a && y >= f.y1a && y < f.y2a) k = j;
        }
        return k;
    }

    __device__ __forceinline__ void finish(bool hit, float b, float g, float r, float p[3]) const
    {
        if (hit) {
            photometric(d, b, g, r);
            p[0] = b; p[1] = g; p[2] = r;
        } else {
            p[0] = fillc[0]; p[1] = fillc[1]; p[2] = fillc[2];
        }
    }

    __device__ __forceinline__ void raw(int cx, int y, bool& hit, float& b, float& g, float& r) const
    {
        const int k = frame_at(cx, y);
        hit = k >= 0;
        b = g = r = 0.0f;
        if (hit) {
            const MosFrame& f = d.f[k];
            frame_pixel_u8(f, cx + f.dx, y + f.dy, b, g, r);
        }
    }

    __device__ __forceinline__ void operator()(int x, int y, float p[3]) const
    {
        bool hit;
        float b, g, r;
        raw(column(x), y, hit, b, g, r);
        finish(hit, b, g, r, p);
    }

    // the 2 x 2 block of the exact-2:1 canvas resize.  Nearly always its four pixels come from one frame: the frame is then found
    // once, and a linearly resized frame sets up its two columns and two rows once instead of once per pixel.
    __device__ __forceinline__ void quad(int x, int y, float p00[3], float p01[3], float p10[3], float p11[3]) const
    {
        const int c0 = column(x), c1 = column(x + 1);
        const int k = frame_at(c0, y);
        bool hit[4];
        float b[4], g[4], r[4];
        if (k >= 0 && frame_at(c1, y) == k && frame_at(c0, y + 1) == k && frame_at(c1, y + 1) == k) {
            const MosFrame& f = d.f[k];
            const int px0 = c0 + f.dx, px1 = c1 + f.dx, py0 = y + f.dy;
            hit[0] = hit[1] = hit[2] = hit[3] = true;
            if (frame_is_copy(f) || frame_is_area(f)) {
                frame_pixel_u8(f, px0, py0, b[0], g[0], r[0]); frame_pixel_u8(f, px1, py0, b[1], g[1], r[1]);
                frame_pixel_u8(f, px0, py0 + 1, b[2], g[2], r[2]); frame_pixel_u8(f, px1, py0 + 1, b[3], g[3], r[3]);
            } else {
                const Axis8 ax0 = axis_x8(f.scx, f.w0, px0), ax1 = axis_x8(f.scx, f.w0, px1);
                const Axis8 ay0 = axis_y8(f.scy, f.h0, py0), ay1 = axis_y8(f.scy, f.h0, py0 + 1);
                frame_linear_u8(f, ax0, ay0, b[0], g[0], r[0]); frame_linear_u8(f, ax1, ay0, b[1], g[1], r[1]);
                frame_linear_u8(f, ax0, ay1, b[2], g[2], r[2]); frame_linear_u8(f, ax1, ay1, b[3], g[3], r[3]);
            }
        } else {
            raw(c0, y, hit[0], b[0], g[0], r[0]); raw(c1, y, hit[1], b[1], g[1], r[1]);
            raw(c0, y + 1, hit[2], b[2], g[2], r[2]); raw(c1, y + 1, hit[3], b[3], g[3], r[3]);
        }
        finish(hit[0], b[0], g[0], r[0], p00); finish(hit[1], b[1], g[1], r[1], p01);
        finish(hit[2], b[2], g[2], r[2], p10); finish(hit[3], b[3], g[3], r[3], p11);
    }
};

__global__ __launch_bounds__(256) void mosaic_aug_kernel(MosBatchArgs a)
{
    // The mosaic's descriptor goes to LDS first: a tap picks its frame per lane, and a per-lane address into the kernel arguments
    // makes the compiler copy the whole 4 KB argument block to scratch once such addresses meet in a select.
    __shared__ MosImg d;
    __shared__ float fillc[3];
    constexpr int WORDS = sizeof(MosImg) / 4;
    static_assert(sizeof(MosImg) % 4 == 0 && WORDS <= 256, "one dword per thread copies the descriptor");
    if (threadIdx.x < WORDS) reinterpret_cast<int*>(&d)[threadIdx.x] = reinterpret_cast<const int*>(&a.im[blockIdx.y])[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {                                                                  // the fill's chain: once per workgroup
        float b = d.fill[0], g = d.fill[1], r = d.fill[2];
        photometric(d, b, g, r);
        fillc[0] = b; fillc[1] = g; fillc[2] = r;
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int side = a.side, m2 = a.m2;
    if (i >= side * side) return;
    const int y = i / side, x = i - y * side;
    float v[3];
    resize_f32(MosTap{d, m2, fillc}, m2, m2, side, side, x, y, v);
    const size_t plane = (size_t)side * side;
    store_normalized(v, a.mean, a.std, a.out + (size_t)blockIdx.y * 3 * plane, plane, i);
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

void launch_mosaic_aug_batch(int n, const unsigned char* const* imgs, const int* geom, const float* photo, int mosaic_size, int side,
                             const float* mean, const float* stdv, float* out, hipStream_t s)
{
    for (int i0 = 0; i0 < n; i0 += MOS_MAX) {
        const int m = n - i0 < MOS_MAX ? n - i0 : MOS_MAX;
        MosBatchArgs b{};
        for (int i = 0; i < m; ++i) {
            const int* g = geom + (size_t)(i0 + i) * MOS_GEOM;
            const float* p = photo + (size_t)(i0 + i) * AUG_PHOTO;
            MosImg& d = b.im[i];
            for (int k = 0; k < 4; ++k) {
                const int* q = g + 12 * k;
                MosFrame& f = d.f[k];
                f.img = imgs[(size_t)(i0 + i) * 4 + k];
                f.h0 = q[0]; f.w0 = q[1]; f.rw = q[2]; f.rh = q[3];
                f.x1a = q[4]; f.y1a = q[5]; f.x2a = q[6]; f.y2a = q[7];
                f.dx = q[8] - q[4]; f.dy = q[9] - q[5];
                f.scx = 1.0 / ((double)f.rw / (double)f.w0);                                 // resize(): inv_scale = dsize / ssize, scale = 1. / inv_scale
                f.scy = 1.0 / ((double)f.rh / (double)f.h0);
            }
            d.flags = (g[49] & AUG_FLAGS_ALL) | (g[48] ? AUG_MIRROR : 0);
            d.bright = p[0]; d.contrast = p[1]; d.sat = p[2]; d.hue = p[3];
            d.fill[0] = p[4]; d.fill[1] = p[5]; d.fill[2] = p[6];
        }
        b.side = side; b.m2 = 2 * mosaic_size; b.out = out + (size_t)i0 * 3 * side * side;
        for (int c = 0; c < 3; ++c) { b.mean[c] = mean[c]; b.std[c] = stdv[c]; }
        hipLaunchKernelGGL(mosaic_aug_kernel, dim3((side * side + 255) / 256, m), dim3(256), 0, s, b);
    }
}

}  // namespace ynk
