"""pw_pipe_group_kernel's launch geometry (no GPU needed): four workgroups of three wavefronts per CU - three wavefronts on every SIMD, 168
registers - and hand-counted waits for LDS-DMA pieces that tolerate no scratch (a reload's s_waitcnt vmcnt(0) retires every piece in
flight).  One symbol has one register count for its three members: the K = 232 and K = 464 forms must fit the K = 116 form's budget.  Read
from the BUILT library's metadata, as tests/test_isa_dwpw_cpu.py does; the dynamic LDS size is the header's (yn_lateral_grid.h)."""
import os
import subprocess
import tempfile

from test_isa_cpu import _vgprs, kernel_meta  # noqa: F401  (the fixture)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yolo-nano_amd", "csrc")
WORKGROUPS_PER_CU = 4
LDS_PER_CU = 160 * 1024


def _header_lds():
    d = tempfile.mkdtemp(prefix="yn_latlds_")
    src, exe = os.path.join(d, "lds.cpp"), os.path.join(d, "lds")
    with open(src, "w") as f:
        f.write('#include "yn_lateral_grid.h"\n#include <cstdio>\nint main() { std::printf("%u %u\\n", ynk::LAT_LDS, ynk::LAT_SLOTS); return 0; }\n')
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", CSRC, src, "-o", exe])
    return [int(v) for v in subprocess.check_output([exe]).decode().split()]


def test_pw_pipe_group_kernel_168_registers_no_scratch(kernel_meta):  # noqa: F811
    mine = {n: v for n, v in kernel_meta.items() if n.split("<")[0] == "pw_pipe_group_kernel"}
    assert len(mine) == 2, sorted(mine)                      # the 1.0x and the 0.5x K triples
    for name, v in mine.items():
        assert int(v["private_segment_fixed_size"]) == 0, "%s uses %s bytes of scratch" % (name, v["private_segment_fixed_size"])
        assert _vgprs(v) <= 168, "%s: %d registers, three wavefronts per SIMD need <= 168" % (name, _vgprs(v))
        assert int(v["group_segment_fixed_size"]) == 0, "%s: static LDS in front of the dynamic carve (rows + planes start at byte 0)" % name
        assert int(v["max_flat_workgroup_size"]) == 192, name


def test_the_launchers_lds_fits_four_workgroups_per_cu():
    lds, slots = _header_lds()
    assert lds == 32 * 128 * 4 + 2 * 32 * 136 * 2            # one chunk of fp32 rows + the hi and lo planes of a chunk
    assert WORKGROUPS_PER_CU * lds <= LDS_PER_CU, lds
    assert slots == 256 * WORKGROUPS_PER_CU
