// yn_lateral_grid.h — the grid rule of pw_pipe_group_kernel (kernels_pipe.hip): how many walking workgroups each member of a grouped pointwise
// launch gets, and which row tiles a workgroup walks.  Plain C++ with no HIP dependence, so that tests/test_lateral_pipe_grid_cpu.py can compile it
// into a host driver and sweep member sizes without a GPU; the launcher sizes the grid with it and the kernel decodes its walk with the same
// function (constexpr: hipcc makes it callable from device code as well).
//
// A member's unit of work is a (row tile, K chunk) pair: LAT_BM rows x up to LAT_CK input channels staged through LDS.  A tile of a K = 464 member
// costs four units, one of K = 116 a single one.  Where the members' tiles do not all fit the resident slots (four workgroups of three
// wavefronts per CU), the slots are dealt by work: the smallest S for which every workgroup walks at most S units' worth of whole tiles.
#pragma once

namespace ynk {

constexpr int LAT_BM = 32;              // rows per tile
constexpr int LAT_CK = 128;             // input channels per LDS chunk (a multiple of 16: whole k-steps)
constexpr int LAT_MAX_CHUNKS = 4;
constexpr unsigned LAT_SLOTS = 1024;    // 256 CUs x 4 workgroups
constexpr int LAT_MEMBERS = 3;

constexpr int lateral_chunks(int K) { return (K + LAT_CK - 1) / LAT_CK; }
constexpr int lateral_chunk_len(int K, int c) { return K - c * LAT_CK < LAT_CK ? K - c * LAT_CK : LAT_CK; }
constexpr unsigned lateral_tiles(int M) { return (unsigned)((M + LAT_BM - 1) / LAT_BM); }
// dynamic LDS of a workgroup: one chunk of fp32 rows, the hi and lo operand planes of a chunk (row stride = plane_stride(LAT_CK) = 136 halves)
constexpr unsigned LAT_PLANE_STRIDE = 136;
constexpr unsigned LAT_LDS = LAT_BM * LAT_CK * 4 + 2 * LAT_BM * LAT_PLANE_STRIDE * 2;

// The K triples pw_pipe_group_kernel is instantiated for (members in this order: longest K first)
constexpr int LAT_TRIPLES[2][LAT_MEMBERS] = {{464, 232, 116}, {192, 96, 48}};
constexpr int lateral_triple(int k0, int k1, int k2)
{
    for (int i = 0; i < 2; ++i)
        if (LAT_TRIPLES[i][0] == k0 && LAT_TRIPLES[i][1] == k1 && LAT_TRIPLES[i][2] == k2) return i;
    return -1;
}

// Whether the members' tiles exceed the resident slots, i.e. whether any workgroup WALKS: below that every workgroup takes one tile, nothing amortises its
// fragment loads and no next tile's rows fly under a GEMM - the group autotuner times the persistent form only where this holds (a forced index runs it
// at every size).
inline bool lateral_walks(const int* M, int n)
{
    unsigned tot = 0;
    for (int p = 0; p < n && p < LAT_MEMBERS; ++p) tot += 8u * ((lateral_tiles(M[p]) + 7u) >> 3);
    return tot > LAT_SLOTS;
}

// Walking workgroups per member: a multiple of 8 each (XCD-contiguous tile ranges), never more than one per tile (rounded up to 8), LAT_SLOTS in all
// at the most.  M[p] >= 1.
inline void lateral_grid(const int* M, const int* K, int n, unsigned (&wgs)[LAT_MEMBERS])
{
    unsigned TL[LAT_MEMBERS] = {}, ch[LAT_MEMBERS] = {}, work = 0, tot = 0;      // TL: tiles per XCD range
    for (int p = 0; p < LAT_MEMBERS; ++p) {
        wgs[p] = 0;
        if (p >= n) continue;
        const unsigned tiles = lateral_tiles(M[p]);
        TL[p] = (tiles + 7u) >> 3;
        ch[p] = (unsigned)lateral_chunks(K[p]);
        wgs[p] = 8u * TL[p];
        work += 8u * TL[p] * ch[p];
        tot += wgs[p];
    }
    if (tot <= LAT_SLOTS) return;
    for (unsigned S = (work + LAT_SLOTS - 1) / LAT_SLOTS;; ++S) {
        unsigned used = 0;
        for (int p = 0; p < n; ++p) { const unsigned per = S / ch[p] ? S / ch[p] : 1u; used += 8u * ((TL[p] + per - 1) / per); }
        if (used > LAT_SLOTS) continue;                     // (ends: 8 n workgroups at the latest)
        for (int p = 0; p < n; ++p) { const unsigned per = S / ch[p] ? S / ch[p] : 1u; wgs[p] = 8u * ((TL[p] + per - 1) / per); }
        return;
    }
}

// The tiles workgroup `local` of a member's `nb` (a multiple of 8) walks: first, first + step, ... below end.  XCD x (= local % 8) owns the
// contiguous range [x TX, (x + 1) TX) with TX = ceil(tiles / 8); its nb / 8 workgroups take the range round-robin.
struct LateralWalk { int first, end, step; };
constexpr LateralWalk lateral_walk(unsigned tiles, unsigned nb, unsigned local)
{
    const unsigned TX = (tiles + 7u) >> 3, x = local & 7u;
    const unsigned end = (x + 1u) * TX < tiles ? (x + 1u) * TX : tiles;
    return LateralWalk{(int)(x * TX + (local >> 3)), (int)end, (int)(nb >> 3)};
}

}  // namespace ynk
