// kernels_slice.hip — sliced inference: a frame larger than the network input runs as overlapping tiles at native resolution (plus the whole
// frame once), every tile's detections go back into the frame and are merged per frame (DESIGN.md 28 is the specification).  The two kernels
// yn_slice_infer puts around the handle's own yn_infer:
//
//   slice_tile_kernel     ValTransforms of the tile frame[y:y+th, x:x+tw], read IN PLACE by the frame's row pitch: the per-pixel body is
//                         yn_prep.h's, the one yn_preprocess_batch runs, so a tile holds the bits that call writes for a contiguous copy of the crop
//   slice_append_kernel   a forward's kept boxes -> frame coordinates -> the end of their frame's merge list, in table order of the tiles
//
// The tile kernel streams.  The common tile is tw == th == rw == rh == side: a crop + normalise + HWC-to-CHW move, 3 bytes read and 12 written
// per pixel.  There a thread takes FOUR neighbouring pixels of a row: their 12 source bytes are three aligned dwords (four when the tile's
// origin is no multiple of 4 bytes, joined by a funnel shift - an aligned dword that holds one byte of the frame lies inside the frame's
// page), and each of the three planes gets one 16-byte store; a wavefront reads 768 contiguous bytes and writes three runs of 1 KiB.  Every
// other tile (resize, 2:1 reduction, pad, a side that is no multiple of 4) goes pixel by pixel through preprocess_at, in the same launch:
// the kind is decided per tile, since every frame's table opens with its full-frame tile and a chunk always holds both kinds.
//
// The append arithmetic is float32 with every step rounded on its own (__fadd_rn / __fsub_rn / __fdiv_rn; the file is built with
// -ffp-contract=off as well); tests/slice_oracle.py restates it in numpy.
#include <hip/hip_runtime.h>

#include "yn_internal.h"
#include "yn_prep.h"
#include "yn_eval_shared.h"

namespace ynk {

namespace {

struct SliceTile { const unsigned char* src; int pitch, tw, th, rw, rh, left, top; };      // src = the tile's top-left pixel inside its frame
struct SliceTileArgs { SliceTile tile[SLICE_CHUNK]; int side, vec; float mean[3], std[3]; float* out; };

// blockIdx.y = tile of the launch; a workgroup covers 1024 pixels of it either way, so one grid serves both kinds of tile.  vec: side % 4 == 0
// and the output is 16-byte aligned - then a common tile takes the four-pixel path.
__global__ __launch_bounds__(256) void slice_tile_kernel(SliceTileArgs b)
{
    const SliceTile& d = b.tile[blockIdx.y];
    PrepArgs a;
    a.img = d.src; a.h0 = d.th; a.w0 = d.tw; a.pitch = d.pitch; a.rw = d.rw; a.rh = d.rh; a.left = d.left; a.top = d.top; a.side = b.side;
    a.mode = prep_mode(d.th, d.tw, d.rw, d.rh);
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.mean[c] = b.mean[c]; a.std[c] = b.std[c]; }
    const size_t plane = (size_t)b.side * b.side;
    a.out = b.out + (size_t)blockIdx.y * 3 * plane;
    if (b.vec && d.tw == b.side && d.th == b.side && d.rw == b.side && d.rh == b.side) {      // (then left == top == 0; uniform over the workgroup)
        const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
        if ((size_t)i >= plane) return;
        const int y = i / b.side, x = i - y * b.side;      // side % 4 == 0: the four pixels share the row
        const uintptr_t p = (uintptr_t)(a.img + ((size_t)y * a.pitch + x) * 3);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p & ~(uintptr_t)3);
        const unsigned sh = (unsigned)(p & 3) * 8;
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = sh ? w[3] : 0u;      // (the fourth dword holds a byte of the quad only when shifted)
        uint32_t q[3];
        q[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
        q[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
        q[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
        float v[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int byte = 3 * k + c;
                v[c][k] = prep_normalise(a, c, (float)((q[byte >> 2] >> ((byte & 3) * 8)) & 0xFFu));
            }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(a.out + (size_t)(2 - c) * plane + i) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        return;
    }
    for (int k = 0; k < 4; ++k) {                               // four rounds of 256 neighbouring pixels: every store of a round is coalesced
        const int t = (blockIdx.x * 4 + k) * 256 + threadIdx.x;
        if ((size_t)t >= plane) return;
        const int y = t / b.side, x = t - y * b.side;
        preprocess_at(a, y - a.top, x - a.left, plane, t);
    }
}

struct SliceRow { int frame, x, y, tw, th, rw, rh, left, top, h0, w0; };
struct SliceAppendArgs { SliceRow row[SLICE_CHUNK]; int n, t0, side; };

// One workgroup per frame f: the tiles of the launch that belong to f, in table order; a tile's surviving rows keep their candidate order (a
// block-wide ordered compaction per 256 candidates).  The forward's outputs are yn_infer's: boxes [n][N][4], scores / cls [n][N], count [n]
// (negative: the range mark - none of that tile's rows is appended).  state = int32 [MERGE_STATE + max_frames]: the merge lists' flag words and
// the cursor of each frame (yn_internal.h).  tstart [T]: where each tile's rows start in its frame's list.  Rows past `cap` are counted and
// not written.
__global__ __launch_bounds__(256) void slice_append_kernel(SliceAppendArgs a, const float* __restrict__ boxes, const float* __restrict__ scores,
                                                           const int32_t* __restrict__ cls, const int32_t* __restrict__ count, int N, int cap, float margin,
                                                           float* __restrict__ lboxes, float* __restrict__ lscores, int32_t* __restrict__ lcls,
                                                           int32_t* __restrict__ state, int32_t* __restrict__ tstart)
{
    __shared__ int wave_kept[4];
    const int f = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cursor = state[MERGE_STATE + f];
    bool bad = false;
    for (int j = 0; j < a.n; ++j) {
        const SliceRow& r = a.row[j];
        if (r.frame != f) continue;                             // (uniform over the workgroup)
        if (threadIdx.x == 0) tstart[a.t0 + j] = cursor;
        int cnt = count[j];
        if (cnt < 0) { bad = true; continue; }
        cnt = cnt < N ? cnt : N;
        const int32_t g[7] = {r.tw, r.th, r.rw, r.rh, r.left, r.top, a.side};
        const float fx = (float)r.x, fy = (float)r.y, fw = (float)r.w0, fh = (float)r.h0;
        const float fm = (float)(r.h0 > r.w0 ? r.h0 : r.w0);
        for (int base = 0; base < cnt; base += 256) {
            const int i = base + (int)threadIdx.x;
            bool keep = i < cnt;
            float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (keep) {
                const float4 bx = *reinterpret_cast<const float4*>(boxes + ((size_t)j * N + i) * 4);
                const float in[4] = {bx.x, bx.y, bx.z, bx.w};
                float p[4];
                evs::unletterbox(in, g, p);                     // the tile as an image: bboxes -= offset; /= scale; *= size
                q[0] = __fadd_rn(p[0], fx); q[1] = __fadd_rn(p[1], fy); q[2] = __fadd_rn(p[2], fx); q[3] = __fadd_rn(p[3], fy);
                if (margin >= 0.0f) {                           // a box that touches a cut side of its tile belongs to the neighbour (strict compares)
                    if (r.x > 0 && q[0] < __fadd_rn(fx, margin)) keep = false;
                    if (r.x + r.tw < r.w0 && q[2] > __fsub_rn((float)(r.x + r.tw), margin)) keep = false;
                    if (r.y > 0 && q[1] < __fadd_rn(fy, margin)) keep = false;
                    if (r.y + r.th < r.h0 && q[3] > __fsub_rn((float)(r.y + r.th), margin)) keep = false;
                }
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) wave_kept[wave] = __popcll(m);
            __syncthreads();
            int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (w < wave) before += wave_kept[w];
                total += wave_kept[w];
            }
            __syncthreads();                                    // wave_kept is read before the next round writes it
            const int dst = cursor + before;
            if (keep && dst < cap) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float hi = (c & 1) ? fh : fw;
                    const float v = q[c] < 0.0f ? 0.0f : (q[c] > hi ? hi : q[c]);      // clamp to the frame (a NaN stays one)
                    q[c] = __fdiv_rn(v, fm);
                }
                const size_t d = (size_t)f * cap + dst;
                *reinterpret_cast<float4*>(lboxes + d * 4) = make_float4(q[0], q[1], q[2], q[3]);
                lscores[d] = scores[(size_t)j * N + i];
                lcls[d] = cls[(size_t)j * N + i];
            }
            cursor += total;
        }
    }
    if (threadIdx.x == 0) {
        state[MERGE_STATE + f] = cursor;
        if (cursor > cap) { atomicOr(&state[0], 1); atomicMax(&state[1], cursor); }
        if (bad) atomicOr(&state[2], 1);
    }
}

}  // namespace

void launch_slice_tiles(int T, const unsigned char* const* frames, const int* shapes, const int* tiles, int side, const float* mean,
                        const float* stdv, float* out, hipStream_t st)
{
    const size_t plane = (size_t)side * side;
    for (int t0 = 0; t0 < T; t0 += SLICE_CHUNK) {
        const int m = T - t0 < SLICE_CHUNK ? T - t0 : SLICE_CHUNK;
        SliceTileArgs b{};
        b.side = side; b.out = out + (size_t)t0 * 3 * plane;
        for (int c = 0; c < 3; ++c) { b.mean[c] = mean[c]; b.std[c] = stdv[c]; }
        b.vec = ((side % 4) == 0 && ((uintptr_t)b.out & 15) == 0) ? 1 : 0;
        for (int i = 0; i < m; ++i) {
            const int* r = tiles + (size_t)(t0 + i) * SLICE_ROW;
            const int w0 = shapes[2 * r[0] + 1];
            b.tile[i] = SliceTile{frames[r[0]] + ((size_t)r[2] * w0 + r[1]) * 3, w0, r[3], r[4], r[5], r[6], r[7], r[8]};
        }
        hipLaunchKernelGGL(slice_tile_kernel, dim3((unsigned)((plane + 1023) / 1024), m), dim3(256), 0, st, b);
    }
}

void launch_slice_append(int F, const int* shapes, const int* tiles, int t0, int n, int side, const float* boxes, const float* scores, const int32_t* cls,
                         const int32_t* count, int N, int cap, float margin, float* lboxes, float* lscores, int32_t* lcls, int32_t* state,
                         int32_t* tstart, hipStream_t st)
{
    if (F <= 0) return;
    for (int j0 = 0; j0 < n; j0 += SLICE_CHUNK) {               // launches of one stream run in order: the lists keep table order
        const int m = n - j0 < SLICE_CHUNK ? n - j0 : SLICE_CHUNK;
        SliceAppendArgs a{};
        a.n = m; a.t0 = t0 + j0; a.side = side;
        for (int i = 0; i < m; ++i) {
            const int* r = tiles + (size_t)(t0 + j0 + i) * SLICE_ROW;
            a.row[i] = SliceRow{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], shapes[2 * r[0]], shapes[2 * r[0] + 1]};
        }
        hipLaunchKernelGGL(slice_append_kernel, dim3(F), dim3(256), 0, st, a, boxes + (size_t)j0 * N * 4, scores + (size_t)j0 * N, cls + (size_t)j0 * N,
                           count + j0, N, cap, margin, lboxes, lscores, lcls, state, tstart);
    }
}

}  // namespace ynk
