"""dwpw_pipe_group_kernel's launch geometry (no GPU needed): the kernel is built for three wavefronts per SIMD - 168 registers - so that its two
resident workgroups per CU (1.5 wavefronts per SIMD) leave room for another stream's kernel beside them, and its hand-counted waits for
LDS-DMA pieces tolerate no scratch (a reload's s_waitcnt vmcnt(0) retires every piece in flight).  Read from the BUILT library's metadata,
as tests/test_isa_cpu.py does for the whole family (which only asks for 256 registers here)."""
from test_isa_cpu import _vgprs, kernel_meta  # noqa: F401  (the fixture)


def test_dwpw_pipe_group_kernel_168_registers_no_scratch(kernel_meta):  # noqa: F811
    mine = {n: v for n, v in kernel_meta.items() if n.split("<")[0] == "dwpw_pipe_group_kernel"}
    assert len(mine) == 1, sorted(mine)
    for name, v in mine.items():
        assert int(v["private_segment_fixed_size"]) == 0, "%s uses %s bytes of scratch" % (name, v["private_segment_fixed_size"])
        assert _vgprs(v) <= 168, "%s: %d registers, three wavefronts per SIMD need <= 168" % (name, _vgprs(v))
        assert int(v["group_segment_fixed_size"]) == 0, "%s: static LDS in front of the dynamic carve (planes + two windows start at byte 0)" % name
