"""stem_pool_kernel<24> as the toolchain builds it (no GPU needed): the kernel is sized for six workgroups per CU - six wavefronts per SIMD, at most
80 registers, at most 160 KB / 6 of LDS, no scratch - and its speed rests on three things hipcc does not promise: the conv tile leaves as 16-byte
LDS writes (as 24 scalars the accumulators went out in 4- and 8-byte writes, eight lanes to a bank), the paired input path issues 9 eight-byte loads
and 9 single ones where the other path issues 27, and no scalar register is spilled to vector lanes (the weights are 648 scalar operands; left to
itself the compiler loaded them far ahead and spilled 182).  Metadata from the BUILT library as tests/test_isa_cpu.py reads it, the assembly from
kernels_conv.hip with the flags of yolo_nano_amd/build.py."""
import re

from test_isa_cpu import _assemble, _vgprs, kernel_meta  # noqa: F401  (the fixture)

import pytest


def test_stem_pool_kernel_six_workgroups_per_cu(kernel_meta):  # noqa: F811
    mine = {n: v for n, v in kernel_meta.items() if n.split("<")[0] == "stem_pool_kernel"}
    assert sorted(mine) == ["stem_pool_kernel<24>"], sorted(mine)
    v = mine["stem_pool_kernel<24>"]
    assert int(v["private_segment_fixed_size"]) == 0, "%s bytes of scratch" % v["private_segment_fixed_size"]
    assert _vgprs(v) <= 80, "%d registers: six wavefronts per SIMD need <= 80 of the 512" % _vgprs(v)
    assert int(v["group_segment_fixed_size"]) * 6 <= 160 * 1024, "%s bytes of LDS: six workgroups per CU need <= 27 306" % v["group_segment_fixed_size"]
    assert int(v["group_segment_fixed_size"]) == 256 * 24 * 4                 # one 24-channel slot per thread


@pytest.fixture(scope="module")
def stem_asm():
    body, on = [], False
    for ln in open(_assemble("kernels_conv.hip")):
        if re.match(r"^_ZN3ynk16stem_pool_kernelILi24EEE\w+:", ln):
            on = True
        if on:
            body.append(ln)
            if ".Lfunc_end" in ln:
                break
    assert len(body) > 500, "stem_pool_kernel<24> not found in the assembly of kernels_conv.hip"
    return body


def _ops(lines, pattern):
    return [ln.split()[0] for ln in lines if re.match(r"^\s+(%s)\b" % pattern, ln)]


def test_tile_leaves_in_16_byte_lds_writes(stem_asm):
    """six ds_write_b128 per thread, standing once in each of the three activation branches; no narrower LDS write anywhere"""
    writes = _ops(stem_asm, r"ds_write\w*")
    assert writes == ["ds_write_b128"] * 18, sorted(set(writes))
    reads = _ops(stem_asm, r"ds_read\w*")
    assert reads == ["ds_read_b128"] * 9, reads                                # the pooling window


def test_paired_path_loads(stem_asm):
    """between the YN_STEM_PAIRED markers: 9 eight-byte loads and 9 single loads (the lanes without a left neighbour), 9 DPP shifts; the rest of the
    kernel holds the 27 single loads of the odd-W path and nothing else from memory"""
    i0 = [i for i, ln in enumerate(stem_asm) if "YN_STEM_PAIRED_BEGIN" in ln]
    i1 = [i for i, ln in enumerate(stem_asm) if "YN_STEM_PAIRED_END" in ln]
    assert len(i0) == 1 and len(i1) == 1 and i0[0] < i1[0]
    inside, outside = stem_asm[i0[0]:i1[0]], stem_asm[:i0[0]] + stem_asm[i1[0]:]
    vm = r"(global|buffer|flat|scratch)_load\w*"
    got = sorted(_ops(inside, vm))
    assert len(got) <= 18 and got == ["global_load_dword"] * 9 + ["global_load_dwordx2"] * 9, got
    assert len([ln for ln in inside if "v_mov_b32_dpp" in ln and "wave_shr:1" in ln]) == 9
    assert _ops(outside, vm) == ["global_load_dword"] * 27, _ops(outside, vm)


def test_no_scalar_spills_and_packed_fmas(stem_asm):
    assert not _ops(stem_asm, r"v_writelane_b32|v_readlane_b32|scratch_\w+"), "scalar registers spilled to vector lanes"
    assert len(_ops(stem_asm, r"v_pk_fma_f32")) == 27 * 12                     # 24 channels in pairs, every product
    assert len(_ops(stem_asm, r"v_max_f32")) == 24                             # ReLU: one max per channel
