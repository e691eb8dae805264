// yn_head_tile_map.h — which pixels a workgroup of head_tail_group_kernel (kernels_post.hip) works on.  Plain C++ with no HIP dependence, so that
// tests/test_head_tile_map_cpu.py can compile it into a host driver and sweep every map size without a GPU; the launcher sizes the grid with it and
// the kernel decodes its tile with the same function (constexpr: hipcc makes it callable from device code as well).
//
// The unit of work is the RUN: four x-consecutive pixels of one image row (a depthwise worker's 3 x 6 window).  RW = ceil(W / 4) runs per row; a
// row's last run is short when W % 4 != 0.  A level's runs are listed image by image and, inside an image, band by band (band = four rows, the
// last one H % 4 rows when that is not zero); inside a band run-column major, row minor.  A TILE is eight consecutive entries of that list, so an
// aligned group of eight is an 8 x 4 pixel block (two run columns x four rows: the windows of a tile overlap in L1 as they did when a tile WAS
// such a block), tiles at band ends, image ends and the list's end take other shapes, and no tile lies outside the image: ceil(B H RW / 8) tiles
// where 8 x 4 blocks took B ceil(H / 4) ceil(W / 8).
#pragma once

namespace ynk {

struct HeadTileMap {
    unsigned runs, tiles;           // list size B * H * RW; ceil(runs / 8)
    unsigned ri, rb;                // runs per image (H * RW) and per full band (4 * RW)
    unsigned mi, mb;                // ceil(2^32 / ri), ceil(2^32 / rb); 0 stands for 2^32 (divisor 1)
    unsigned ml;                    // ceil(2^16 / rows of the last band)
    int H, W, hl;                   // hl = rows of the last band: H % 4, or 4
};

struct HeadTileRun { int b, y, x0, valid; };     // image, row, first column, pixels inside the row (0: a slot behind the list's end; b = y = x0 = 0 then)

constexpr int HEAD_TILE_RUNS = 8, HEAD_RUN_PIXELS = 4;

// n / d by multiplication, m = ceil(2^32 / d): exact for n * d <= 2^32 (m d = 2^32 + k with k < d, and the error n k / (d 2^32) stays below 1 / d)
constexpr unsigned head_tile_div(unsigned n, unsigned m) { return m ? (unsigned)(((unsigned long long)n * m) >> 32) : n; }

// Whether head_tile_run's multiplications are exact for this shape: the largest slot number times either divisor stays below 2^32, and a band's run
// number below 2^15 (n / 3 == (n * 21846) >> 16 up to there).  The shapes of this network are orders of magnitude inside (416 x 416, bs 32: 2.3e7).
constexpr bool head_tile_map_ok(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1 || W > 8192) return false;
    const unsigned long long rw = (unsigned long long)(W + 3) / 4, ri = rw * H, slots = (ri * B + 7) / 8 * 8;
    return slots * ri <= 0xffffffffull && ri * 4 * rw <= 0xffffffffull;
}

constexpr HeadTileMap head_tile_map(int B, int H, int W)
{
    const unsigned rw = (unsigned)(W + 3) / 4, ri = rw * (unsigned)H, rb = 4 * rw, hl = (H & 3) ? (unsigned)(H & 3) : 4u;
    const unsigned runs = ri * (unsigned)B;
    return HeadTileMap{runs, (runs + 7) / 8, ri, rb,
                       (unsigned)((0xffffffffull + ri) / ri), (unsigned)((0xffffffffull + rb) / rb), (65535u + hl) / hl, H, W, (int)hl};
}

// entry e of the list (e = tile * 8 + slot)
constexpr HeadTileRun head_tile_run(const HeadTileMap& m, unsigned e)
{
    if (e >= m.runs) return HeadTileRun{0, 0, 0, 0};
    const unsigned b = head_tile_div(e, m.mi), r = e - b * m.ri;
    const unsigned band = head_tile_div(r, m.mb), q = r - band * m.rb;
    const bool full = (int)(band * 4 + 4) <= m.H;
    const unsigned col = full ? q >> 2 : (q * m.ml) >> 16, row = q - col * (full ? 4u : (unsigned)m.hl);
    const int x0 = (int)(col * 4), left = m.W - x0;
    return HeadTileRun{(int)b, (int)(band * 4 + row), x0, left < HEAD_RUN_PIXELS ? left : HEAD_RUN_PIXELS};
}

}  // namespace ynk
