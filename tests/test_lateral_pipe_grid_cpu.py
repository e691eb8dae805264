"""The grid rule of pw_pipe_group_kernel (yolo-nano_amd/csrc/yn_lateral_grid.h) swept on the host: no GPU needed.

The launcher sizes the grid with lateral_grid (workgroups per member, dealt by work = row tiles x K chunks where the members' tiles do not all fit
the 1 024 resident slots) and the kernel decodes its walk with lateral_walk.  A tiny host driver compiled against the header answers, for a sweep
of (M5, M4, M3) and both instantiated K triples: the workgroups per member, how many workgroups own each (tile, chunk) - a tile's chunks are walked
by the tile's owner, so that is the tile's owner count -, and the fewest / most tiles a workgroup of each member walks.  The test checks what
the kernel relies on - every tile exactly once, a multiple of 8 per member, the total within the slots - against the rule written down here a
second time, and that the shapes of tests/test_gpu_lateral_pipe.py's walk case do reach three tiles per workgroup in every member."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo-nano_amd", "csrc")
TRIPLES = ((464, 232, 116), (192, 96, 48))
SLOTS, BM, CK = 1024, 32, 128
FLAGSHIP = (5408, 21632, 86528)                              # 1.0x, 416 x 416, bs 32: the stride-32 / 16 / 8 maps

DRIVER = r"""
#include "yn_lateral_grid.h"
#include <cstdio>
#include <vector>
using namespace ynk;
int main(int argc, char** argv)
{
    static_assert(LAT_BM == 32 && LAT_CK == 128 && LAT_SLOTS == 1024 && LAT_CK % 16 == 0, "the test restates these");
    static_assert(lateral_triple(464, 232, 116) == 0 && lateral_triple(192, 96, 48) == 1 && lateral_triple(116, 232, 464) < 0 && lateral_triple(96, 96, 96) < 0, "");
    static_assert(lateral_chunks(464) == 4 && lateral_chunk_len(464, 3) == 80 && lateral_chunks(232) == 2 && lateral_chunk_len(232, 1) == 104 && lateral_chunks(116) == 1, "");
    for (int i = 1; i + 5 < argc; i += 6) {                  // M0 M1 M2 K0 K1 K2 -> per member: workgroups, tiles not owned exactly once, min and max tiles per workgroup
        int M[3], K[3];
        for (int p = 0; p < 3; ++p) { std::sscanf(argv[i + p], "%d", &M[p]); std::sscanf(argv[i + 3 + p], "%d", &K[p]); }
        unsigned wgs[LAT_MEMBERS];
        lateral_grid(M, K, 3, wgs);
        for (int p = 0; p < 3; ++p) {
            const unsigned tiles = lateral_tiles(M[p]);
            std::vector<int> own(tiles, 0);
            unsigned mn = ~0u, mx = 0, outside = 0;
            for (unsigned l = 0; l < wgs[p]; ++l) {
                const LateralWalk w = lateral_walk(tiles, wgs[p], l);
                unsigned n = 0;
                if (w.step < 1) { ++outside; continue; }
                for (int t = w.first; t < w.end; t += w.step, ++n) { if (t < 0 || (unsigned)t >= tiles) ++outside; else ++own[t]; }
                mn = n < mn ? n : mn; mx = n > mx ? n : mx;
            }
            unsigned bad = outside;
            for (unsigned t = 0; t < tiles; ++t) bad += own[t] != 1;
            std::printf("%u %u %u %u ", wgs[p], bad, mn, mx);
        }
        std::printf("%d\n", (int)lateral_walks(M, 3));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver():
    d = tempfile.mkdtemp(prefix="yn_latgrid_")
    src, exe = os.path.join(d, "grid.cpp"), os.path.join(d, "grid")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    return exe


def _ask(driver, cases):
    """cases: [(Ms, Ks)] -> [[(workgroups, bad, min tiles, max tiles) per member] + [lateral_walks]]"""
    out = []
    for o in range(0, len(cases), 500):
        args = [str(v) for Ms, Ks in cases[o:o + 500] for v in tuple(Ms) + tuple(Ks)]
        for ln in subprocess.check_output([driver] + args).decode().split("\n"):
            if ln.strip():
                v = [int(x) for x in ln.split()]
                out.append([tuple(v[4 * p:4 * p + 4]) for p in range(3)] + [v[12]])
    assert len(out) == len(cases)
    return out


def _rule(Ms, Ks):
    """the rule a second time: one workgroup per tile (rounded up to 8 per XCD range) where that fits the slots; else the smallest S for which
    every workgroup walks whole tiles worth at most S (tile, chunk) units - at least one tile - and all members fit together"""
    TL = [-(-(-(-M // BM)) // 8) for M in Ms]
    ch = [-(-K // CK) for K in Ks]
    if 8 * sum(TL) <= SLOTS:
        return [8 * t for t in TL]
    S = -(-sum(8 * t * c for t, c in zip(TL, ch)) // SLOTS)
    while True:
        w = [8 * -(-t // max(1, S // c)) for t, c in zip(TL, ch)]
        if sum(w) <= SLOTS:
            return w
        S += 1


SWEEP_M = (64, 65, 95, 97, 333, 1200, 5408, 8191, 21632, 30001, 86528, 100000, 200000, 700001)


def test_every_tile_once_within_the_slots(driver):
    cases = [((a, b, c), Ks) for Ks in TRIPLES for a in SWEEP_M for b in SWEEP_M for c in SWEEP_M]
    capped = 0
    for (Ms, Ks), got in zip(cases, _ask(driver, cases)):
        got, walks = got[:3], got[3]
        assert walks == int(8 * sum(-(-(-(-M // BM)) // 8) for M in Ms) > SLOTS), (Ms, walks)
        wgs = [g[0] for g in got]
        assert wgs == _rule(Ms, Ks), (Ms, Ks, wgs)
        assert all(w % 8 == 0 and w >= 8 for w in wgs) and sum(wgs) <= SLOTS, (Ms, Ks, wgs)
        assert all(g[1] == 0 for g in got), "a tile owned by no workgroup, or by two: %r" % ((Ms, Ks, got),)
        for M, w in zip(Ms, wgs):
            assert w <= 8 * -(-(-(-M // BM)) // 8), "more workgroups than tiles (rounded up to 8): %r" % ((Ms, Ks, wgs),)
        capped += sum(wgs) > SLOTS - 24 and any(g[3] > 1 for g in got)
    assert capped > 100, "the sweep hardly reaches the dealt regime"


def test_work_is_dealt_by_tiles_times_chunks(driver):
    """the flagship shape: a workgroup of the K = 464 member (four chunks per tile) walks one tile where one of the K = 116 member walks six"""
    (got,) = _ask(driver, [(FLAGSHIP, TRIPLES[0])])
    got = got[:3]
    assert [g[0] for g in got] == [176, 232, 456], got
    assert [g[3] for g in got] == [1, 3, 6], got
    units = [g[3] * c for g, c in zip(got, (4, 2, 1))]
    assert max(units) <= 6, units


def test_the_gpu_walk_case_reaches_three_tiles_per_workgroup(driver):
    import test_gpu_lateral_pipe as tg
    assert tg.K10 == TRIPLES[0] and tg.K05 == TRIPLES[1]
    (got,) = _ask(driver, [(tg.WALK_M, tg.K10)])
    assert got[3] == 1 and all(g[1] == 0 and g[2] >= 3 for g in got[:3]), got
    # ... and the ragged cases leave every member with fewer tiles than workgroups
    for Ms in ((64, 65, 95), (97, 333, 64), (333, 95, 97), (65, 64, 333)):
        (got,) = _ask(driver, [(Ms, tg.K10)])
        assert got[3] == 0 and all(-(-M // BM) < g[0] and g[2] == 0 and g[3] == 1 for M, g in zip(Ms, got[:3])), (Ms, got)


def test_the_tuner_times_the_walk_only_where_there_is_one(driver):
    """lateral_walks: the members' tiles exceed the resident slots.  The benchmark shapes do; small maps (one tile per workgroup, nothing amortised, and
    the shapes whose launch plans tests/wide_cases.py and tests/range_cases.py pin to a tile with the autotuner on) do not."""
    shapes = {(5408, 21632, 86528): 1, (11552, 46208, 184832): 1,          # 416 x 416 and 608 x 608, bs 32
              (75, 300, 1200): 0, (540, 2160, 8640): 0, (338, 1352, 5408): 0, (64, 64, 64): 0}      # 160 x 160 x 3, 192 x 192 x 15, 416 x 416 x 2
    got = _ask(driver, [(Ms, TRIPLES[0]) for Ms in shapes])
    assert [g[3] for g in got] == list(shapes.values()), got
    api = open(os.path.join(CSRC, "yn_api.hip")).read()
    assert "!pw_pipe_group_candidate(a, n)) continue;" in api


def test_the_kernel_and_the_launcher_use_the_header():
    pipe = open(os.path.join(CSRC, "kernels_pipe.hip")).read()
    assert '#include "yn_lateral_grid.h"' in pipe
    body = pipe[pipe.index("void pw_pipe_group_block("):]
    assert "lateral_walk(lateral_tiles(a.M), nb, local)" in body and "lateral_grid(M, K, n, wgs)" in body and "lateral_triple(" in body
    assert "(size_t)LAT_LDS" in body and "return lateral_walks(M, n);" in body
