"""stage_pipe_kernel (kernels_stage.hip) at the map widths where its halo geometry matters.

Item (u, T) of the one-launch stage waits for the ready flags of tiles T-1, T, T+1 of unit u-1; its depthwise window, flat pixels
[m0 - W - 1, m0 + BM + W + 1), stays inside those tiles only when W + 1 <= BM.  The shapes are chosen from that geometry:
0.5x stage 2 (bf 24) at W = 64 ... 80 (512 ... 640) where the four-wavefront form's 64-row tiles are too short, 992 / 1024 / 1056 where
W crosses BM - 1, BM, BM + 1 of stage 4 (bf 96) and stage 3 (bf 48 / 116), batches of 1 ... 4 (fewer tiles than workgroups: all of
unit u-1 in flight while unit u starts), default size rule and mode 2, both publish modes.  Per shape:

  (a) raw heads bit for bit against one launch per unit (stage_fuse(0)) on the same handle, five repetitions;
  (b) every stage_pipe_kernel<BF,NW,...> the profiler saw ran with W + 1 <= BM (BM from BF and NW, W from the stage in the layer name) -
      deterministic, whether or not a race would have fired - and the forms taken are the ones named below;
  (c) at one large shape per backbone, raw heads against the torch-CPU oracle at the suite's tolerance (nothing above 608 was checked
      against it before)."""
import re

import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu

ATOL = 1e-4

# forms under mode 2 (every size): {stage: "<BF,NW>" or None (the units run one launch each)}.  launch_stage_pipe also needs a multiple of
# eight pixels per stage (B * W * W): the batches of 992 / 1056 (B 8) and 1.0x 992 (B 2) are chosen so that stages 3 and 4 qualify.
FORMS = {
    ("0.5x", 512): {2: "24,8", 3: "48,4", 4: "96,4"},     # stage 2: W 64 == BM of <24,4>
    ("0.5x", 544): {2: "24,8", 3: "48,4", 4: "96,4"},
    ("0.5x", 608): {2: "24,8", 3: "48,4", 4: "96,4"},     # W 76: <24,4> reached two tiles each side
    ("0.5x", 640): {2: "24,8", 3: "48,4", 4: "96,4"},
    ("0.5x", 992): {2: "24,8", 3: "48,4", 4: "96,4"},     # stage 4: W 31 = BM - 1 of <96,4>
    ("0.5x", 1024): {2: None, 3: "48,8", 4: "96,8"},      # W = BM of <48,4> / <96,4>; stage 2 W 128 = BM of <24,8>
    ("0.5x", 1056): {2: None, 3: "48,8", 4: "96,8"},
    ("1.0x", 992): {3: "116,8"},                           # W 62
    ("1.0x", 1024): {3: None},                             # W 64 = BM of <116,8>
    ("1.0x", 1056): {3: None},
}

SHAPES = ([("0.5x", S, B) for S in (512, 544, 608, 640) for B in (1, 2, 3, 4)] +
          [("0.5x", 992, 8), ("0.5x", 1024, 1), ("0.5x", 1056, 8), ("1.0x", 992, 2), ("1.0x", 1024, 1), ("1.0x", 1056, 2)])


@pytest.fixture(scope="module")
def capi():
    from yolo_nano_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return c


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def stage_launches(h, x, S):
    """{stage: (BF, NW, W, BM)} of the stage_pipe_kernel launches of one profiled forward."""
    h.profile_enable(True)
    h.forward_raw(x)
    recs = h.profile_records()
    h.profile_enable(False)
    out = {}
    for name, kern, _, _, _ in recs:
        m = re.match(r"stage_pipe_kernel<(\d+),(\d+),(true|false)>", kern)
        if not m:
            continue
        bf, nw = int(m.group(1)), int(m.group(2))
        st = int(re.match(r"backbone\.stage(\d)\.", name).group(1))
        W = S // (8 << (st - 2))
        out[st] = (bf, nw, W, 32 * nw // (2 if bf <= 64 else 4))
    return out


@pytest.mark.parametrize("backbone,S,B", SHAPES)
def test_stage_pipe_halo_geometry(capi, backbone, S, B):
    h = capi.Handle(S, 20, arch.MULTI_ANCHOR_SIZE, backbone, 0.001, 0.5, max_batch=B)
    h.load_state_dict(weights.make_state_dict(backbone, 20))
    h.fold_bn()
    x = dev(weights.make_input(B, S, seed=S + 3 * B))
    h.stage_fuse(0)
    h.chain_pipe(0)
    ref = [t.clone() for t in h.forward_raw(x)]
    h.chain_pipe(1)
    for mode, early in ((1, False), (1, True), (2, False), (2, True)):          # the default first
        tag = "%s S=%d B=%d stage_fuse(%d, publish_early=%s)" % (backbone, S, B, mode, early)
        h.stage_fuse(mode, early)
        got = stage_launches(h, x, S)
        for st, (bf, nw, W, bm) in sorted(got.items()):                        # (b) before (a): it holds whether or not a race fires
            assert W + 1 <= bm, "%s: stage %d ran stage_pipe_kernel<%d,%d> with %d-row tiles on %d-wide maps - its window reaches past the tiles it waits for" % (
                tag, st, bf, nw, bm, W)
        forms = {st: "%d,%d" % v[:2] for st, v in got.items()}
        if mode == 2:
            want = {st: f for st, f in FORMS[(backbone, S)].items() if f and B * (S // (8 << (st - 2))) ** 2 % 8 == 0}
            assert forms == want, (tag, forms)
        else:                                                                   # the size rule only drops stages, never changes a form
            assert all(FORMS[(backbone, S)][st] == f for st, f in forms.items()), (tag, forms)
        for rep in range(5):                                                    # (a)
            out = [t.clone() for t in h.forward_raw(x)]
            for u, v in zip(out, ref):
                assert torch.equal(u, v), "%s, repetition %d" % (tag, rep)
        assert h.range_status() == (False, False), tag
    h.close()


@pytest.mark.parametrize("backbone,S,B", [("0.5x", 640, 2), ("1.0x", 1056, 2)])
def test_large_maps_vs_torch_oracle(capi, backbone, S, B):
    """(c): one launch per unit and the one-launch stages against the torch-CPU oracle."""
    from oracle.torch_port import TorchNet
    sd = weights.make_state_dict(backbone, 20)
    xn = weights.make_input(B, S, seed=S + 1)
    ref = TorchNet(sd, backbone, 20).forward_raw(xn)
    h = capi.Handle(S, 20, arch.MULTI_ANCHOR_SIZE, backbone, 0.001, 0.5, max_batch=B)
    h.load_state_dict(sd)
    h.fold_bn()
    x = dev(xn)
    for mode in (0, 1, 2):
        h.stage_fuse(mode)
        for g, r in zip(h.forward_raw(x), ref):
            np.testing.assert_allclose(g.permute(0, 3, 1, 2).cpu().numpy(), np.asarray(r), atol=ATOL, rtol=0,
                                       err_msg="%s S=%d B=%d stage_fuse(%d)" % (backbone, S, B, mode))
    assert h.range_status() == (False, False)
    h.close()
