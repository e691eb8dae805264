"""down_unit_pipe_kernel<CIN, BF, RELU> (stage 2's stride-2 unit as one launch, widths as template parameters) against the five-launch
path, through the C ABI: bit for bit at every tile geometry the 8 x 4 output tile can meet, for both instantiated widths
((cin, bf) = (24, 58) at 1.0x and (24, 24) at 0.5x), three fused runs each (a race on the reused LDS planes shows as differing bits).

The network only takes input sizes that are multiples of 32, so stage 2's output map is always a multiple of 4: the maps of S = 48 (6 x 6:
narrower than a tile, a ragged last tile ROW) and S = 80 (10 x 10: ragged in x and y) cannot come from a handle.  Those two shapes run the
unit alone on the stage-2 input map such a size would give (S / 4): yn_op_down_unit (the fused kernel on any even map) against
yn_op_shuffle_block (the five launches); there is no tap and no head at those sizes, the unit's own output is compared."""
import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu

WALK_CAP = 1024                          # launch_down_unit's walking workgroups: beyond that many tiles a workgroup walks more than one
KERNEL = {"1.0x": "down_unit_pipe_kernel<24,58,true>", "0.5x": "down_unit_pipe_kernel<24,24,true>"}


@pytest.fixture(scope="module")
def capi():
    from yolo_nano_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return c


def _handle(capi, backbone, S, B):
    h = capi.Handle(S, 20, arch.MULTI_ANCHOR_SIZE, backbone, 0.001, 0.5, max_batch=B)
    h.load_state_dict(weights.make_state_dict(backbone, 20))
    h.fold_bn()
    return h


def _unit_kernels(h):
    return [r[1] for r in h.profile_records() if r[1].startswith(("down_unit_pipe_kernel", "down2_kernel"))]


def _network_case(capi, backbone, S, B):
    """stage 2's tap and the three raw heads, five launches vs the fused kernel (three runs); returns the unit kernels of the fused run"""
    h = _handle(capi, backbone, S, B)
    try:
        x = torch.as_tensor(weights.make_input(B, S, seed=11)).cuda()
        h.down_fuse(False)
        tap0 = h.forward_taps(x)[0].clone()
        raw0 = [t.clone() for t in h.forward_raw(x)]
        h.down_fuse(True)
        h.profile_enable(True)
        raw1 = [t.clone() for t in h.forward_raw(x)]
        kernels = _unit_kernels(h)
        h.profile_enable(False)
        assert torch.equal(h.forward_taps(x)[0], tap0)
        for a, b in zip(raw0, raw1):
            assert torch.equal(a, b)
        for _ in range(2):                                   # the second and third fused run
            assert torch.equal(h.forward_taps(x)[0], tap0)
            for a, b in zip(raw0, h.forward_raw(x)):
                assert torch.equal(a, b)
        return kernels
    finally:
        h.close()


# S, B: 64 x 2 = 8 x 8 map, exact tiles, tiles of two images adjacent in the walk; 96 x 1 = 12 x 12, whole tile rows and a ragged last tile
# column; 64 x 513 = two tiles per image, 1026 tiles for 1024 walking workgroups: the smallest batch at which a workgroup walks two tiles
@pytest.mark.parametrize("backbone", ["1.0x", "0.5x"])
@pytest.mark.parametrize("S,B", [(64, 2), (96, 1), (64, WALK_CAP // 2 + 1)])
def test_fused_unit_matches_five_launches(capi, backbone, S, B):
    if B > 2:
        assert B * ((S // 8 + 3) // 4) * ((S // 8 + 7) // 8) == WALK_CAP + 2
    kernels = _network_case(capi, backbone, S, B)
    assert kernels[0] == KERNEL[backbone], kernels


# S = 48 -> 12 x 12 input, 6 x 6 output map: narrower than a tile, last tile row ragged; S = 80 -> 20 x 20 input, 10 x 10: ragged in x and y
@pytest.mark.parametrize("backbone", ["1.0x", "0.5x"])
@pytest.mark.parametrize("S,B", [(48, 1), (80, 3)])
def test_fused_unit_matches_five_launches_ragged_rows(capi, backbone, S, B):
    h = _handle(capi, backbone, 64, B)
    try:
        cin, cout = 24, arch.STAGE_CH[backbone][0]
        rs = np.random.RandomState(S)
        x = torch.as_tensor(np.abs(rs.randn(B, S // 4, S // 4, cin)).astype(np.float32)).cuda()      # the stem's output is behind a ReLU and a max pool
        h.profile_enable(True)
        ref = h.op_shuffle_block("backbone.stage2.0", x, cout, 2).clone()
        five = [r[1] for r in h.profile_records()]
        assert len(five) == 5 and not any(k.startswith("down_unit_pipe_kernel") for k in five), five
        for _ in range(3):
            h.profile_enable(True)
            y = h.op_down_unit("backbone.stage2.0", x, cout)
            kernels = [r[1] for r in h.profile_records()]
            assert kernels == [KERNEL[backbone]], kernels
            assert torch.equal(y, ref)
        assert ref.shape == (B, S // 8, S // 8, cout) and float(ref.abs().max()) > 0.0
    finally:
        h.profile_enable(False)
        h.close()


def test_wide_stage_still_takes_down2(capi):
    """1.5x: bf = 88 is no instantiated width - pw1 + down2_kernel at all three stages (stage 4: five launches), same bits as unfused"""
    kernels = _network_case(capi, "1.5x", 64, 2)
    assert kernels and all(k.startswith("down2_kernel") for k in kernels), kernels


def test_only_instantiated_widths_are_accepted(capi):
    """Each width pair runs its own instantiation, exactly once per forward; a block of another width (stage 3: cin = bf = 116) is refused by
    the kernel's own entry instead of running some other form of it"""
    seen = {}
    for backbone in ("1.0x", "0.5x"):
        h = _handle(capi, backbone, 64, 1)
        try:
            x = torch.as_tensor(weights.make_input(1, 64, seed=3)).cuda()
            h.profile_enable(True)
            h.forward_raw(x)
            seen[backbone] = [k for k in _unit_kernels(h) if k.startswith("down_unit_pipe_kernel")]
            h.profile_enable(False)
            if backbone == "1.0x":
                x3 = torch.zeros((1, 8, 8, arch.STAGE_CH[backbone][0]), dtype=torch.float32).cuda()
                with pytest.raises(capi.YnError):
                    h.op_down_unit("backbone.stage3.0", x3, arch.STAGE_CH[backbone][1])
        finally:
            h.close()
    assert seen == {b: [KERNEL[b]] for b in KERNEL}, seen
