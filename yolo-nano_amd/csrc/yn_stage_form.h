// yn_stage_form.h — the form rule of stage_pipe_kernel (kernels_stage.hip): tile height per (channels, wavefronts), its LDS, and which form
// launch_stage_pipe takes for a stage; the LDS sizes of unit_pipe_kernel and pw_pipe_kernel (kernels_pipe.hip) beside it.  Plain C++ with no HIP dependence, so that tests/test_stage_form_cpu.py can compile it into a host
// driver and sweep every map size without a GPU.  plane_stride lives here because the LDS formula needs it (constexpr: hipcc makes it
// callable from device code as well).
#pragma once
#include <cstddef>

namespace ynk {

// Row stride (halves) of an operand plane [rows][C] in LDS that 16-byte fragment reads walk row by row (lane = row): a
// ds_read_b128 is served in groups of 16 lanes, conflict-free when their 16-byte pieces tile the 64 banks, i.e. when the stride is an
// ODD multiple of 16 bytes.  ceil(C/8)*8 + 8 is one only for an even octet count: C = 116 (15 octets) gave 256 bytes - all 16 lanes
// on the same four banks (SQ_LDS_BANK_CONFLICT = 88 % of the stage-3 chain's LDS cycles, profiles/r04_sq_counters.txt) - and C = 232 a
// two-way conflict.  The columns [C, stride) stay zero (K tail).
constexpr int plane_stride(int C) { return ((((C + 7) >> 3) + 1) & ~1) * 8 + 8; }

// stage_pipe_kernel<BF, NW>: rows per tile.  WN = 2 (bf <= 64) or 4 wavefronts share a tile's columns, the other NW / WN stack 32-row blocks.
constexpr int stage_pipe_bm(int bf, int nw) { return 32 * (nw / (bf <= 64 ? 2 : 4)); }

// ---- dynamic LDS of the persistent kernels: the launchers size it with these, the kernels carve it up in the same order and static_assert
//      the part behind the window against the same function (the window depends on the map width, a run-time value). ----
// fp32 window of a bm-row tile: flat pixels [m0 - W - 1, m0 + bm + W + 1) x bf floats (+ `lead` bytes in front), in whole 16-byte pieces
constexpr size_t pipe_window_lds(int bf, int W, int bm, int lead) { return ((size_t)(bm + 2 * W + 2) * bf * 4 + lead + 15) & ~(size_t)15; }
constexpr size_t pipe_row_lds(int c) { return (((size_t)c * 4 + 15) / 16) * 16; }                       // one fp32 row of c channels, 16-byte padded
constexpr size_t pipe_planes_lds(int c, int bm) { return (size_t)2 * bm * plane_stride(c) * 2; }          // hi and lo operand planes [bm][plane_stride(c)]
// unit_pipe_kernel: window (up to 8 bytes of lead-in: channel pairs), pass-through rows, planes, tap bits, taps + bias; pw_pipe_kernel: rows, planes
constexpr size_t unit_pipe_lds_fixed(int bf, int bm) { return bm * pipe_row_lds(bf) + pipe_planes_lds(bf, bm) + (size_t)bm * 4 + (size_t)10 * bf * 4; }
constexpr size_t unit_pipe_lds(int bf, int W, int bm) { return pipe_window_lds(bf, W, bm, 8) + unit_pipe_lds_fixed(bf, bm); }
constexpr size_t pw_pipe_lds(int k, int bm) { return bm * pipe_row_lds(k) + pipe_planes_lds(k, bm); }
// stage_pipe_kernel: window, pass-through rows, planes, tap bits, taps + bias and two (b2, b1n) pairs (14 rows), control words (+ YN_EXP_STAGE_TIMING's sums)
constexpr size_t stage_pipe_lds_fixed(int bf, int bm) { return (size_t)bm * bf * 4 + pipe_planes_lds(bf, bm) + (size_t)bm * 4 + (size_t)14 * bf * 4 + 64 + 192; }
constexpr size_t stage_pipe_lds(int bf, int W, int bm) { return pipe_window_lds(bf, W, bm, 0) + stage_pipe_lds_fixed(bf, bm); }

struct StagePipeForm {
    int nw, bm;                 // nw = 0: no form
    size_t lds, lds_max;
};

// The form launch_stage_pipe takes for a stage of bf channels on W-wide maps: the four-wavefront one where its LDS fits two workgroups per CU
// (80 KB each), else the eight-wavefront one (one per CU, 160 KB, twice the rows per tile).  A form is taken ONLY when W + 1 <= BM: item
// (u, T) waits for the ready flags of tiles T-1, T, T+1 of unit u-1, and its window [m0 - W - 1, m0 + BM + W + 1) lies inside those tiles
// only then - wider, it reads rows of T-2 / T+2 nobody waited for, and (u+1, T) may overwrite them through the ping-pong buffers while
// (u, T+-2) still reads them.  W == BM is rejected too (safe only because the out-of-tile corner pixels are masked).  No form: the
// units run one launch each.
inline StagePipeForm stage_pipe_form(int bf, int W)
{
    if (bf != 24 && bf != 48 && bf != 96 && bf != 116) return {0, 0, 0, 0};     // the instantiated widths
    for (int nw = 4; nw <= 8; nw += 4) {
        const int bm = stage_pipe_bm(bf, nw);
        const size_t lds = stage_pipe_lds(bf, W, bm), lds_max = (size_t)(nw == 4 ? 80 : 160) * 1024;
        if (lds <= lds_max && W + 1 <= bm) return {nw, bm, lds, lds_max};
    }
    return {0, 0, 0, 0};
}

}  // namespace ynk
