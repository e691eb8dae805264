// yn_unit_tile.h — the pieces of the persistent stride-1 unit kernels' tile body that are written once.  unit_pipe_kernel (kernels_pipe.hip: one
// unit per launch, a static tile walk) and stage_pipe_kernel (kernels_stage.hip: a stage's units in one launch, tickets and ready flags) run
// them under their own schedules; pw_pipe_kernel takes the ones it shares.  Here: the tap-valid bits of a tile row, split2, the clamped
// fragment offsets, the step of the panel walk, the window's DMA issue loop - each compiles to the instructions of the code it replaced.
// NOT here, and still written out in both kernels line for line the same (whoever changes one changes the other): the depthwise phase,
// the first epilogue, the pass-through rows' DMA loop, the K-tail zeroing, the transposing store of stage_pipe_kernel's second epilogue.
// As functions - by value, by reference, or a lambda around the unchanged statements - each made hipcc schedule the code around it
// differently (the first two: other address arithmetic, up to 6 more registers, an occupancy step in the 48-channel forms): DESIGN 4.3d.
#pragma once
#include "yn_device.h"

namespace ynk {

// ---- tap-valid bits of tile row t: which of the nine taps of flat pixel m0 + t fall inside its image (zero padding; rows past M:
//      none).  Written a tile ahead, read by the depthwise phase.  q / W and yy / H as multiplications (exact below 2^16). ----
template <int BM>
__device__ __forceinline__ void write_tap_bits(int* mtab, int m0, int t, int M, int H, int W, int HW, float inv_w, float inv_h)
{
    if (t < BM) {
        const int rem0 = m0 % HW;
        const int y0 = rem0 / W, x0 = rem0 - y0 * W;
        const int q = x0 + t;
        const int dy = (int)(((float)q + 0.5f) * inv_w);
        const int x = q - dy * W;
        const int yy = y0 + dy;
        const int y = yy - (int)(((float)yy + 0.5f) * inv_h) * H;       // rows past the image's last one continue in the next image
        const int yb = (y >= 1 ? 1 : 0) | 2 | (y + 1 < H ? 4 : 0), xb = (x >= 1 ? 1 : 0) | 2 | (x + 1 < W ? 4 : 0);
        int bits = 0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
            if ((yb >> ky) & 1) bits |= xb << (3 * ky);
        mtab[t] = m0 + t < M ? bits : 0;
    }
}

// ---- two adjacent channels c, c + 1 of plane row r -> both planes ----
template <int PS>
__device__ __forceinline__ void split2(h16* Ph, h16* Pl, int r, int c, float v0, float v1, float& amax)
{
    float v[2] = {v0, v1};
    split_store<2>(Ph + r * PS + c, Pl + r * PS + c, v, amax);
}

// ---- byte offset of a lane's B fragment of k-step s in a pack [KQ octets][npad columns][8 halves].  No masks on fragment loads (a masked
//      load is waited for where it is issued and needs a temporary per load in flight): the octet past the matrix and the columns past npad
//      read the nearest valid ones - finite weights against the planes' zero K tail; columns >= the width are never stored.
//      frag_step_off: from lw = frag_off of k-step 0, ONE lane offset for all k-steps (per-step 64-bit lane addresses are hoisted out of
//      the tile loop, spilled, and reloaded through vmcnt(0)); callers make lw opaque per GEMM for the same reason. ----
template <int KQ>
__device__ __forceinline__ unsigned frag_off(int s, int h, int n, int npad)
{
    const int kq = s * 2 + h < KQ ? s * 2 + h : KQ - 1;
    return ((unsigned)kq * (unsigned)npad + (unsigned)(n < npad ? n : npad - 1)) * 16u;
}
template <int KQ, unsigned NPAD>
__device__ __forceinline__ unsigned frag_step_off(unsigned lw, int s, int h)
{
    const unsigned kq = (unsigned)(s * 2 + h < KQ ? s * 2 + h : KQ - 1);
    return (s * 2 + 1 < KQ) ? lw + (unsigned)s * (2u * NPAD * 16u) : lw - (unsigned)h * (NPAD * 16u) + kq * (NPAD * 16u);
}

// ---- the register-panel walk: k-step s of this lane's A rows (ahp / alp: its plane row + h * 8) against the panel's fragments of that step.
//      The kernels keep the loop and their refill loads around it; split_join after the walk. ----
__device__ __forceinline__ void panel_step(const h16* ahp, const h16* alp, int s, const h16x8 bh, const h16x8 bl, f32x16& acc0, f32x16& acc1)
{
    const h16x8 ah = *reinterpret_cast<const h16x8*>(ahp + s * 16);
    const h16x8 al = *reinterpret_cast<const h16x8*>(alp + s * 16);
    split_mfma(ah, al, bh, bl, acc0, acc1);
}

// ---- the window's LDS-DMA pieces: flat pixels [m0 - W - 1, m0 + BM + W + 1) x BF floats of the dense tensor t1, from the 16-byte boundary
//      below the first byte (window_lead: 0, or 8 for channel pairs and an odd first pixel); pieces past either end of t1 are clamped (those
//      pixels' taps are masked; t1_lim = the last piece that holds a byte of t1).  Addresses come from an OPAQUE copy of the thread index:
//      as loop invariants they are hoisted out of the tile loop (14 registers), spilled, and a scratch reload's vmcnt(0) retires the DMA
//      pieces in flight.  SC1: dma16. ----
template <int BF>
__device__ __forceinline__ int window_lead(int m0, int W) { return (BF * 4u) % 16u == 0 ? 0 : (((m0 - W - 1) * (BF * 4)) & 15); }
template <int BF>
__device__ __forceinline__ int window_t1_lim(int M) { return ((M * (BF * 4) + 15) & ~15) - 16; }    // (M * BF * 8 < 2^32 is a launch condition)
template <int BF, int NTHR, bool SC1>
__device__ __forceinline__ void issue_window_pieces(const float* t1, int t1_lim, int m0, int W, unsigned win_bytes, unsigned lds_win, int t, int wave)
{
    constexpr unsigned ROWB = BF * 4u;
    int tt = t;
    asm volatile("" : "+v"(tt));
    const int g0 = (m0 - W - 1) * (int)ROWB;                // first byte of the window
    const int sh = ROWB % 16u == 0 ? 0 : (g0 & 15);
    const int gs = g0 - sh + tt * 16;
    const int nch = (int)((win_bytes + (unsigned)sh + 15u) >> 4);
    for (int c0 = 0; c0 < nch; c0 += NTHR) {
        int src = gs + c0 * 16;
        src = src < 0 ? 0 : (src > t1_lim ? t1_lim : src);
        if (c0 + tt < nch) dma16<SC1>(t1, (unsigned)src, lds_win + (unsigned)(c0 + wave * 64) * 16u);
    }
}

}  // namespace ynk
