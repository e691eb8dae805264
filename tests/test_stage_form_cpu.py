"""The form rule of stage_pipe_kernel (stage_pipe_form, yolo-nano_amd/csrc/yn_stage_form.h) swept on the host: no GPU needed.

Item (u, T) of the one-launch stage waits for the ready flags of tiles T-1, T, T+1 of unit u-1 only.  Its depthwise window, flat pixels
[m0 - W - 1, m0 + BM + W + 1), stays inside those tiles only when W + 1 <= BM; a wider map would read rows nobody waited for and let the
ping-pong buffers be overwritten under a reader.  A tiny host driver compiled against the header prints the rule's answer
for every stage width and every map width W = S / 8, S / 16, S / 32 of S = 32 ... 2048 (all of W = 1 ... 256); the test checks that
every form taken is safe and fits its LDS, that the guard takes away only unsafe forms, and pins the forms of the BASELINE shapes."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo-nano_amd", "csrc")
WIDTHS = (24, 48, 96, 116)           # the instantiated stage widths: 0.5x stages 2 / 3 / 4, 1.0x stage 3
OTHER = (58, 232)                    # 1.0x stages 2 and 4: no stage_pipe_kernel instance
WMAX = 2048 // 8

DRIVER = r"""
#include "yn_stage_form.h"
#include <cstdio>
int main()
{
    const int widths[] = {24, 48, 96, 116, 58, 232};
    for (int bf : widths)
        for (int W = 1; W <= %d; ++W) {
            const ynk::StagePipeForm f = ynk::stage_pipe_form(bf, W);
            std::printf("%%d %%d %%d %%d %%zu %%zu", bf, W, f.nw, f.bm, f.lds, f.lds_max);
            for (int nw = 4; nw <= 8; nw += 4) std::printf(" %%d %%zu", ynk::stage_pipe_bm(bf, nw), ynk::stage_pipe_lds(bf, W, ynk::stage_pipe_bm(bf, nw)));
            std::printf("\n");
        }
    return 0;
}
""" % WMAX


@pytest.fixture(scope="module")
def forms():
    """{(bf, W): (nw, bm, lds, lds_max, {nw: (bm, lds)})} from the header, compiled the way the library is (hipcc, C++17)."""
    d = tempfile.mkdtemp(prefix="yn_form_")
    src, exe = os.path.join(d, "form.cpp"), os.path.join(d, "form")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    out = {}
    for ln in subprocess.check_output([exe]).decode().split("\n"):
        if ln:
            v = [int(x) for x in ln.split()]
            out[(v[0], v[1])] = (v[2], v[3], v[4], v[5], {4: (v[6], v[7]), 8: (v[8], v[9])})
    assert len(out) == (len(WIDTHS) + len(OTHER)) * WMAX
    return out


def _form(forms, bf, W):
    nw, bm = forms[(bf, W)][:2]
    return (nw, bm) if nw else None


def test_every_form_taken_keeps_the_window_inside_the_three_waited_tiles(forms):
    taken = 0
    for bf in WIDTHS:
        for S in range(32, 2049, 32):
            for W in (S // 8, S // 16, S // 32):
                nw, bm, lds, lds_max, per = forms[(bf, W)]
                if not nw:
                    continue
                taken += 1
                assert bm == 32 * nw // (2 if bf <= 64 else 4) == per[nw][0], (bf, W, nw, bm)
                assert W + 1 <= bm, "bf %d, W %d (S %d): form <%d,%d> with %d-row tiles - its window reaches past tiles T-1..T+1" % (bf, W, S, bf, nw, bm)
                assert lds == per[nw][1] and lds <= lds_max == (80 if nw == 4 else 160) * 1024, (bf, W, nw, lds, lds_max)
    assert taken > 0


def test_the_guard_takes_away_only_unsafe_forms(forms):
    """Against the rule without the guard (the first form whose LDS fits): where that form is safe it is still the one taken (no shape that
    ran one launch per stage loses it or changes form); where it is not, the eight-wavefront form is taken if it is safe and fits, else none."""
    for (bf, W), (nw, bm, lds, lds_max, per) in forms.items():
        if bf in OTHER:
            continue
        fits = [n for n in (4, 8) if per[n][1] <= (80 if n == 4 else 160) * 1024]
        safe = [n for n in fits if W + 1 <= per[n][0]]
        old = fits[0] if fits else 0
        if old and W + 1 <= per[old][0]:
            assert nw == old, (bf, W, nw, old)
        else:
            assert nw == (safe[0] if safe else 0), (bf, W, nw, safe)


def test_forms_of_the_named_shapes(forms):
    # the BASELINE shapes (1.0x stage 3): 416 -> W 26, two four-wavefront workgroups per CU; 608 -> W 38, one of eight (the window's LDS)
    assert _form(forms, 116, 416 // 16) == (4, 32)
    assert _form(forms, 116, 608 // 16) == (8, 64)
    # 1.0x stage 3 at 992 / 1024 / 1056: W = BM - 2, BM, BM + 2 of the eight-wavefront form
    assert _form(forms, 116, 992 // 16) == (8, 64)
    assert _form(forms, 116, 1024 // 16) is None
    assert _form(forms, 116, 1056 // 16) is None
    # 0.5x stage 2 (bf 24): <24,4> up to W 60 (480), the eight-wavefront form from W 64 (512, W == BM) to 124 (992), none from 1024
    assert _form(forms, 24, 480 // 8) == (4, 64)
    assert _form(forms, 24, 512 // 8) == (8, 128)
    assert _form(forms, 24, 608 // 8) == (8, 128)
    assert _form(forms, 24, 992 // 8) == (8, 128)
    assert _form(forms, 24, 1024 // 8) is None
    # 0.5x stage 3 (bf 48: W = BM - 2, BM) and stage 4 (bf 96: W = BM - 1, BM, BM + 1) around their four-wavefront tile heights
    assert _form(forms, 48, 992 // 16) == (4, 64)
    assert _form(forms, 48, 1024 // 16) == (8, 128)
    assert _form(forms, 96, 992 // 32) == (4, 32)
    assert _form(forms, 96, 1024 // 32) == (8, 64)
    assert _form(forms, 96, 1056 // 32) == (8, 64)
    assert _form(forms, 96, 2048 // 32) is None
    # widths without a kernel instance take no form
    assert not any(forms[(bf, W)][0] for bf in OTHER for W in range(1, WMAX + 1))
