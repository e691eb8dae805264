"""The tile map of head_tail_group_kernel (yolo-nano_amd/csrc/yn_head_tile_map.h) swept on the host: no GPU needed.

A workgroup of that kernel takes eight consecutive entries of a level's run list (run = four x-consecutive pixels of one image row; the list goes
image by image, band of four rows by band, inside a band run-column major and row minor).  The kernel decodes an entry with head_tile_run - by
multiplications with host-computed reciprocals, not by division - and the launcher sizes the grid with head_tile_map.  A tiny host driver compiled
against the header dumps every slot of every tile for every H, W in 1 ... 64 and B in 1, 2, 3; the test compares them with the rule written down
here a second time (plain loops, plain division) and checks what the kernel relies on: every pixel exactly once, no run across a row end, empty slots
only behind a row's end and behind the list's end, aligned groups of eight = 8 x 4 blocks, ceil(B H RW / 8) tiles."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo-nano_amd", "csrc")
SMAX = 64
BS = (1, 2, 3)
FLAGSHIP = ((32, 52, 52), (32, 26, 26), (32, 13, 13))      # 1.0x, 416 x 416, bs 32

DRIVER = r"""
#include "yn_head_tile_map.h"
#include <cstdio>
#include <cstring>
using namespace ynk;
int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "dump")) {          // every slot of every tile, four bytes each: image, row, first column, pixels
        for (int B = 1; B <= 3; ++B)
            for (int H = 1; H <= %(smax)d; ++H)
                for (int W = 1; W <= %(smax)d; ++W) {
                    const HeadTileMap m = head_tile_map(B, H, W);
                    for (unsigned e = 0; e < m.tiles * HEAD_TILE_RUNS; ++e) {
                        const HeadTileRun r = head_tile_run(m, e);
                        const unsigned char v[4] = {(unsigned char)r.b, (unsigned char)r.y, (unsigned char)r.x0, (unsigned char)r.valid};
                        std::fwrite(v, 1, 4, stdout);
                    }
                }
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "exact")) {         // B H W triples: entries that differ from the rule written with / and %%
        for (int i = 2; i + 2 < argc; i += 3) {
            int B, H, W;
            std::sscanf(argv[i], "%%d", &B); std::sscanf(argv[i + 1], "%%d", &H); std::sscanf(argv[i + 2], "%%d", &W);
            const HeadTileMap m = head_tile_map(B, H, W);
            const unsigned rw = (W + 3) / 4, ri = rw * H;
            unsigned long long bad = 0;
            for (unsigned e = 0; e < m.runs; ++e) {
                const unsigned b = e / ri, r = e %% ri, band = r / (4 * rw), q = r %% (4 * rw), rows = H - 4 * band < 4 ? H - 4 * band : 4;
                const int y = (int)(4 * band + q %% rows), x0 = (int)(q / rows * 4);
                const HeadTileRun g = head_tile_run(m, e);
                bad += !(g.b == (int)b && g.y == y && g.x0 == x0 && g.valid == (W - x0 < 4 ? W - x0 : 4));
            }
            std::printf("%%u %%llu\n", m.runs, bad);
        }
        return 0;
    }
    for (int i = 1; i + 2 < argc; i += 3) {                  // B H W triples: ok, runs, tiles, and the last run of the list
        int B, H, W;
        std::sscanf(argv[i], "%%d", &B); std::sscanf(argv[i + 1], "%%d", &H); std::sscanf(argv[i + 2], "%%d", &W);
        const bool ok = head_tile_map_ok(B, H, W);
        if (!ok) { std::printf("%%d %%d %%d 0\n", B, H, W); continue; }
        const HeadTileMap m = head_tile_map(B, H, W);
        const HeadTileRun r = head_tile_run(m, m.runs - 1), z = head_tile_run(m, m.runs);
        std::printf("%%d %%d %%d 1 %%u %%u %%d %%d %%d %%d %%d\n", B, H, W, m.runs, m.tiles, r.b, r.y, r.x0, r.valid, z.valid);
    }
    return 0;
}
""" % {"smax": SMAX}


@pytest.fixture(scope="module")
def driver():
    d = tempfile.mkdtemp(prefix="yn_tilemap_")
    src, exe = os.path.join(d, "map.cpp"), os.path.join(d, "map")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    return exe


def _image_runs(H, W):
    """the run list of one image by the rule, written with plain loops: [(y, x0, valid)]"""
    rw = (W + 3) // 4
    out = []
    for y0 in range(0, H, 4):
        rows = min(4, H - y0)
        for col in range(rw):
            for row in range(rows):
                out.append((y0 + row, 4 * col, min(4, W - 4 * col)))
    return np.asarray(out, np.int64).reshape(-1, 3)


@pytest.fixture(scope="module")
def slots(driver):
    """{(B, H, W): int array [tiles * 8, 4]} of what the header answers"""
    raw = np.frombuffer(subprocess.check_output([driver, "dump"]), np.uint8).astype(np.int64).reshape(-1, 4)
    out, o = {}, 0
    for B in BS:
        for H in range(1, SMAX + 1):
            for W in range(1, SMAX + 1):
                n = (B * H * ((W + 3) // 4) + 7) // 8 * 8
                out[(B, H, W)] = raw[o:o + n]
                o += n
    assert o == len(raw), "tiles != ceil(B * H * RW / 8) somewhere: %d slots dumped, %d expected" % (len(raw), o)
    return out


def test_every_slot_is_the_rules_entry(slots):
    """entry e of the list, for every shape: the multiplications of head_tile_run give what plain loops give; slots behind the list's end are empty"""
    for H in range(1, SMAX + 1):
        for W in range(1, SMAX + 1):
            img = _image_runs(H, W)
            for B in BS:
                want = np.concatenate([np.concatenate([np.full((len(img), 1), b), img], 1) for b in range(B)])
                got = slots[(B, H, W)]
                assert len(got) - 8 < len(want) <= len(got), (B, H, W)
                assert np.array_equal(got[:len(want)], want), (B, H, W)
                assert not got[len(want):].any(), (B, H, W)


def test_every_pixel_once_and_no_run_across_a_row_end(slots):
    for (B, H, W), s in slots.items():
        b, y, x0, v = s.T
        live = v > 0
        assert live.sum() == B * H * ((W + 3) // 4), (B, H, W)
        assert not live[int(live.sum()):].any(), "an empty slot in front of the list's end: %r" % ((B, H, W),)
        assert (x0 % 4 == 0).all() and (v <= 4).all() and ((x0 + v)[live] <= W).all() and (y[live] < H).all() and (b[live] < B).all(), (B, H, W)
        short = live & (v < 4)                               # a short run is a row's last one, and only where W is no multiple of 4
        assert ((x0 + v)[short] == W).all() and (x0[live & ~short] + 4 <= W).all(), (B, H, W)
        pix = np.concatenate([((b * H + y) * W + x0 + o)[live & (v > o)] for o in range(4)])
        assert len(pix) == B * H * W and len(np.unique(pix)) == B * H * W, (B, H, W)


def test_aligned_groups_of_eight_are_8x4_blocks(slots):
    """a tile that starts on an even run column of a full band with two run columns to go is that band's 8 x 4 block (what a tile was when tiles were
    laid over the image); on maps of whole blocks every tile is one, in the old order and number"""
    blocks = 0
    dy, dx = np.tile(np.arange(4), 2), np.repeat([0, 4], 4)
    for (B, H, W), s in slots.items():
        rw = (W + 3) // 4
        t = s.reshape(-1, 8, 4)
        b0, y0, x0, v0 = t[:, 0].T
        al = (v0 > 0) & (y0 % 4 == 0) & (y0 + 4 <= H) & (x0 % 8 == 0) & (x0 // 4 + 2 <= rw)
        blocks += int(al.sum())
        t = t[al]
        assert (t[:, :, 0] == t[:, :1, 0]).all() and (t[:, :, 1] == t[:, :1, 1] + dy).all() and (t[:, :, 2] == t[:, :1, 2] + dx).all(), (B, H, W)
        assert (t[:, :4, 3] == 4).all() and (t[:, 4:, 3] == np.minimum(4, W - t[:, 4:, 2])).all(), (B, H, W)
        if H % 4 == 0 and W % 8 == 0:
            assert len(s) // 8 == B * (H // 4) * (W // 8), (B, H, W)
            b, y, x0, v = s.T
            assert (v == 4).all(), (B, H, W)
            first = s[::8]
            assert np.array_equal(first[:, 1] % 4, np.zeros(len(first))) and np.array_equal(first[:, 2] % 8, np.zeros(len(first))), (B, H, W)
    assert blocks > 100000


def _counts(driver, shapes):
    args = [str(v) for s in shapes for v in s]
    return [[int(x) for x in ln.split()] for ln in subprocess.check_output([driver] + args).decode().split("\n") if ln]


def test_tile_counts(driver):
    shapes = [(B, H, W) for B in BS for H in range(1, SMAX + 1, 3) for W in range(1, SMAX + 1)] + list(FLAGSHIP) + [(128, 76, 76), (8, 256, 256)]
    for (B, H, W), v in zip(shapes, _counts(driver, shapes)):
        rw = (W + 3) // 4
        assert v[:4] == [B, H, W, 1], v
        assert v[4] == B * H * rw and v[5] == (B * H * rw + 7) // 8, v
        # the last run of the list: the last image's last row (the last band's last run column, last row), short where W % 4 != 0; one further: empty
        assert v[6:] == [B - 1, H - 1, 4 * (rw - 1), W - 4 * (rw - 1), 0], v
    flag = dict(zip(FLAGSHIP, _counts(driver, FLAGSHIP)))
    assert [flag[s][5] for s in FLAGSHIP] == [2704, 728, 208]
    assert [flag[s][4] for s in FLAGSHIP] == [21632, 5824, 1664]
    # what 8 x 4 blocks laid over every image took at that shape, and what the pixels need
    assert [B * ((H + 3) // 4) * ((W + 7) // 8) for B, H, W in FLAGSHIP] == [2912, 896, 256]
    assert [-(-B * H * W // 32) for B, H, W in FLAGSHIP] == [2704, 676, 169]


def test_shapes_beyond_the_exact_range_are_refused(driver):
    """head_tile_map_ok is the kernel's precondition (head_tail_ok asks it): slots * runs-per-image <= 2^32 - 1, W <= 8192"""
    shapes = [(1, 1, 8192), (1, 1, 8193), (0, 4, 4), (4, 0, 4), (4, 4, 0), (1, 255, 1024), (1, 256, 1024), (255, 128, 128), (256, 128, 128)]
    got = [v[3] for v in _counts(driver, shapes)]
    want = []
    for B, H, W in shapes:
        rw = (W + 3) // 4
        ri = rw * H
        want.append(int(B >= 1 and H >= 1 and 1 <= W <= 8192 and ((ri * B + 7) // 8 * 8) * ri <= 2 ** 32 - 1 and ri * 4 * rw <= 2 ** 32 - 1))
    assert got == want and 0 in got[5:] and 1 in got[5:], (got, want)


def test_large_shapes_decode_exactly(driver):
    """the reciprocal multiplications at the benchmark shapes and at the edge of what head_tile_map_ok admits: every entry, against / and %"""
    shapes = list(FLAGSHIP) + [(128, 76, 76), (8, 256, 256), (1, 255, 1024), (255, 128, 128), (1, 3, 8192), (7, 2, 8191), (100000, 1, 1), (5000, 1, 5)]
    assert all(v[3] == 1 for v in _counts(driver, shapes))
    out = subprocess.check_output([driver, "exact"] + [str(v) for s in shapes for v in s]).decode().split("\n")
    for (B, H, W), ln in zip(shapes, out):
        assert [int(x) for x in ln.split()] == [B * H * ((W + 3) // 4), 0], ((B, H, W), ln)


def test_the_gpu_tests_restatement_is_the_headers_order(slots):
    """tests/test_gpu_head_tail_packed.py steers its data by a restatement of the packed order (packed_slots: tile rows) and counts what the packed
    wavefronts do with it; that restatement against the header, and its steered data against the regimes it must reach (raw = activation + bias
    exactly under the selection weights, so the CPU can count them)"""
    import decode_cases as dc
    import test_gpu_head_tail_packed as tp
    for B, h, w in ((1, 12, 12), (3, 6, 6), (3, 3, 3), (3, 20, 28), (2, 52, 52), (1, 28, 12), (3, 5, 7), (2, 13, 13)):
        rows = tp.packed_slots(B, h, w)
        s = slots[(B, h, w)]
        assert rows.shape == (len(s) // 8, 32, 4)
        r = rows.reshape(-1, 4, 4)                           # [slot, pixel of the run, (b, y, x, inside)]
        inside = r[..., 3] > 0
        assert np.array_equal(inside.sum(-1), s[:, 3]), (B, h, w)
        live = s[:, 3] > 0
        assert np.array_equal(r[live, 0, :3], s[live, :3]) and (r[..., 2][inside] == (s[:, 2:3] + np.arange(4))[inside]).all(), (B, h, w)
    for name in ("s96-b1", "s160-b3", "r160x224-b3"):
        H, W, B = tp.CASES[name]
        raws = [dc.tail_ref(x, *dc.selection_layers(tp.C), dtype=np.float32) for x in tp._steered_acts(B, H, W)]
        tp._steering_reached(name, raws, B, H, W, dc.CONF_STEERED)


def test_the_kernel_and_the_launcher_use_the_header():
    post = open(os.path.join(CSRC, "kernels_post.hip")).read()
    assert '#include "yn_head_tile_map.h"' in post
    body = post[post.index("void head_tail_block("):post.index("void launch_decode_boxes(")]
    assert "head_tile_run(a.tm," in body and "head_tile_map(a[p].B, a[p].H, a[p].W)" in body and "head_tile_map_ok(" in body
    assert "tm.tiles" in body
    # the old rule is gone from the kernel and its launcher: no tile grid of ceil(H / 4) x ceil(W / 8) blocks
    assert not re.search(r"\(a(\[p\])?\.W \+ (7|TW - 1)\) / (8|TW)", body) and "tx_n" not in body and "ty_n" not in body
