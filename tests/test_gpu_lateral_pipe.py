"""pw_pipe_group_kernel (kernels_pipe.hip): the three FPN laterals as one launch of the persistent pointwise walk, against the tile route of
the same grouped launch (gemm_split_group_kernel under the first index of the split family).  Same 16-deep k-steps into the same accumulators,
same epilogue: every output element of every member must have the same bits (torch.equal).  Every case runs twice - a race between an LDS-DMA
piece and a read shows up as bits that differ from run to run.

Shapes come from the kernel's geometry (yn_lateral_grid.h): 32-row tiles, K walked in LDS chunks of 128 channels (K = 464: 3 x 128 + 80, streamed
fragment panel; K = 232: 128 + 104, streamed; K = 116: one chunk, register-resident matrix), XCD-contiguous tile ranges of ceil(tiles / 8),
1 024 resident workgroup slots dealt by (tiles x chunks).
  ragged     M in {64, 65, 95, 97, 333}: a partial last tile, clamped rows; every member has fewer tiles than workgroups;
  walk       WALK_M: every member's workgroups walk at least three tiles (tests/test_lateral_pipe_grid_cpu.py asks the header) - the peeled
             first tile, the steady state, the last tile, and the streamed panel coming round to its first chunk again;
  NaN        the rows inside a NaN-filled buffer: a K tail of 4 (116) / 8 (232) behind the last full k-step - a pad column not re-zeroed for the
             short last chunk, a piece read past a row or a clamped row taken from behind the tensor all end in a NaN;
  strided    the right half of a wider map (in_ld = 2 K, in_off = K) into a column range of a wider output;
  range      one 7e4 in each member in turn, in the first and in the last K chunk: the split-f16 range flag rises; quiet input: it does not;
  0.5x       the (192, 96, 48) triple of the 0.5x backbone;
  network    forward_raw with the index forced: same raw heads, the kernel in the launch records; nothing forced: the tile, with the autotuner off
             (the heuristic) and on (at these sizes no workgroup would walk: lateral_walks keeps the persistent form out of its candidates)."""
import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu

K10 = (464, 232, 116)
K05 = (192, 96, 48)
N = 96
WALK_M = (60001, 60003, 60005)           # members in the kernel's order: K = 464, 232, 116
KERNEL = "pw_pipe_group_kernel<"
TILE = "gemm_split_group_kernel<"


@pytest.fixture(scope="module")
def capi():
    from yolo_nano_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return c


@pytest.fixture(scope="module")
def hvoc(capi):
    h = capi.Handle(320, 20, arch.MULTI_ANCHOR_SIZE, "1.0x", 0.001, 0.5, max_batch=2)
    h.load_state_dict(weights.make_state_dict("1.0x", 20))
    h.fold_bn()
    yield h
    h.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _weights(rs, Ks):
    return [(dev((rs.standard_normal((N, K, 1, 1)) / np.sqrt(K)).astype(np.float32)), dev(rs.standard_normal((N,)).astype(np.float32))) for K in Ks]


def _inputs(rs, Ms, Ks):
    return [dev(rs.standard_normal((M, K)).astype(np.float32)) for M, K in zip(Ms, Ks)]


def _run(h, cfg, xs, wb, act=1, out=None):
    """one grouped launch under the pinned index -> (outputs, the kernel symbols recorded)"""
    h.set_pw_config(cfg)
    h.profile_enable(True)
    try:
        ys = h.op_pwconv_group([(x, w, b) for x, (w, b) in zip(xs, wb)], act, out)
        torch.cuda.synchronize()
        names = [r[1] for r in h.profile_records()]
    finally:
        h.profile_enable(False)
    return ys, names


def _same_bits(h, xs, wb, what, out_pair=None):
    """reference = the first split tile, subject = the pipe index, twice; out_pair: (reference outputs, subject outputs) as (wide, off) lists"""
    _, fam = h.pw_families()
    try:
        ref, names = _run(h, fam[0], xs, wb, out=out_pair[0] if out_pair else None)
        assert len(names) == 1 and names[0].startswith(TILE), names
        ref = [r.clone() for r in ref]
        for rep in range(2):
            got, names = _run(h, fam[-1], xs, wb, out=out_pair[1] if out_pair else None)
            assert len(names) == 1 and names[0].startswith(KERNEL), names
            for p, (a, b) in enumerate(zip(ref, got)):
                assert a.shape == b.shape and bool(torch.isfinite(a).all()), (what, p)
                assert torch.equal(a, b), "%s, run %d: member %d differs in %d values" % (what, rep, p, int((a != b).sum().item()))
        assert h.range_status() == (False, False), what
    finally:
        h.set_pw_config(-1)
    return ref


@pytest.mark.parametrize("Ms", [(64, 65, 95), (97, 333, 64), (333, 95, 97), (65, 64, 333)])
def test_ragged_members_bit_identical(hvoc, Ms):
    rs = np.random.RandomState(sum(Ms))
    _same_bits(hvoc, _inputs(rs, Ms, K10), _weights(rs, K10), "M = %r" % (Ms,))


def test_multi_tile_walks_bit_identical(hvoc):
    rs = np.random.RandomState(7)
    _same_bits(hvoc, _inputs(rs, WALK_M, K10), _weights(rs, K10), "walk")


@pytest.mark.parametrize("Ks", [K10, K05])
def test_nan_surround_never_leaks_in(hvoc, Ks):
    Ms = (97, 333, 65)
    rs = np.random.RandomState(11 + Ks[0])
    plain = _inputs(rs, Ms, Ks)
    inside = []
    for x in plain:
        buf = torch.full((x.numel() + 8192,), float("nan"), dtype=torch.float32, device="cuda")
        v = buf[4096:4096 + x.numel()].view(x.shape)
        v.copy_(x)
        inside.append(v)
    wb = _weights(rs, Ks)
    ref = _same_bits(hvoc, inside, wb, "NaN surround")
    ref2 = _same_bits(hvoc, plain, wb, "plain allocation")
    for a, b in zip(ref, ref2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("out_off", [96, 2])
def test_strided_members_bit_identical(hvoc, out_off):
    """in_ld = 2 K with in_off = K (even); out_ld = 200 > N, out_off a multiple of four (16-byte stores) and not (scalar stores).  The columns of the
    wide output the launch does not own keep their bits."""
    Ms = (97, 333, 200)
    rs = np.random.RandomState(out_off)
    wide = [dev(rs.standard_normal((M, 2 * K)).astype(np.float32)) for M, K in zip(Ms, K10)]
    xs = [(w, K) for w, K in zip(wide, K10)]
    wb = _weights(rs, K10)
    outs = [[(torch.full((M, 200), -7.0, dtype=torch.float32, device="cuda"), out_off) for M in Ms] for _ in range(2)]
    _same_bits(hvoc, xs, wb, "strided", out_pair=outs)
    for (a, _), (b, _) in zip(*outs):
        assert torch.equal(a, b)
        rest = torch.cat([a[:, :out_off], a[:, out_off + N:]], 1)
        assert bool((rest == -7.0).all())
    dense = _same_bits(hvoc, [w[:, K:].contiguous() for w, K in zip(wide, K10)], wb, "the same rows, dense")
    for (a, _), d in zip(outs[0], dense):
        assert torch.equal(a[:, out_off:out_off + N], d)


def test_range_flag_from_every_member_and_chunk(hvoc):
    Ms = (97, 333, 200)
    rs = np.random.RandomState(3)
    xs = [dev(rs.uniform(-3.0e4, 3.0e4, (M, K)).astype(np.float32)) for M, K in zip(Ms, K10)]
    wb = _weights(rs, K10)
    _, fam = hvoc.pw_families()
    hvoc.exact_f32(False)
    hvoc.range_status()
    try:
        _, names = _run(hvoc, fam[-1], xs, wb)
        assert names[0].startswith(KERNEL) and hvoc.range_status() == (False, False)
        for p, (M, K) in enumerate(zip(Ms, K10)):
            for r, c in ((0, 0), (M - 1, K - 1), (M // 2, K - 1 - (K - 1) % 128)):      # first chunk; last chunk's last column; its first one
                hot = [x.clone() for x in xs]
                hot[p][r, c] = 7.0e4
                _, names = _run(hvoc, fam[-1], hot, wb)
                assert names[0].startswith(KERNEL), names
                assert hvoc.range_status() == (False, True), "7e4 in member %d at row %d, channel %d did not raise the flag" % (p, r, c)
                assert hvoc.range_status() == (False, False)
    finally:
        hvoc.set_pw_config(-1)


def test_half_width_triple_bit_identical(hvoc):
    rs = np.random.RandomState(5)
    for Ms in ((65, 97, 333), (20001, 20003, 40005)):
        _same_bits(hvoc, _inputs(rs, Ms, K05), _weights(rs, K05), "0.5x M = %r" % (Ms,))


def test_a_group_without_a_form_takes_the_tile(hvoc):
    """another K triple, a member below 64 rows: the pipe index runs the heuristic tile, as before"""
    _, fam = hvoc.pw_families()
    rs = np.random.RandomState(9)
    try:
        for Ms, Ks in (((97, 97, 97), (96, 96, 96)), ((63, 97, 97), K10), ((97, 97, 97), (116, 232, 464))):
            xs, wb = _inputs(rs, Ms, Ks), _weights(rs, Ks)
            ref, names = _run(hvoc, fam[0], xs, wb)
            ref = [r.clone() for r in ref]
            got, names = _run(hvoc, fam[-1], xs, wb)
            assert len(names) == 1 and names[0].startswith(TILE), names
            for a, b in zip(ref, got):
                assert torch.equal(a, b)
    finally:
        hvoc.set_pw_config(-1)


@pytest.mark.parametrize("S,B", [(160, 3), (416, 2)])
def test_in_the_network(capi, S, B):
    h = capi.Handle(S, 20, arch.MULTI_ANCHOR_SIZE, "1.0x", 0.001, 0.5, max_batch=B)
    h.load_state_dict(weights.make_state_dict("1.0x", 20))
    h.fold_bn()
    x = dev(weights.make_input(B, S, seed=S + B))
    _, fam = h.pw_families()

    def lateral_kernels():
        h.profile_enable(True)
        h.forward_raw(x)
        recs = [(r[0], r[1]) for r in h.profile_records()]
        h.profile_enable(False)
        return [k for n, k in recs if n == "conv1x1_*"]
    try:
        h.forward_raw(x)                                                      # (the tuner times its candidates on an unprofiled call)
        assert [k[:len(TILE)] for k in lateral_kernels()] == [TILE]          # the autotuner's pick: no workgroup would walk at these sizes, it times the tiles only
        h.autotune(False)
        assert [k[:len(TILE)] for k in lateral_kernels()] == [TILE]          # untuned, nothing forced: the heuristic tile
        h.set_pw_config(fam[0])
        ref = [t.clone() for t in h.forward_raw(x)]
        h.set_pw_config(fam[-1])
        for rep in range(2):
            for u, v in zip(h.forward_raw(x), ref):
                assert torch.equal(u, v), rep
        ks = lateral_kernels()
        assert len(ks) == 1 and ks[0].startswith(KERNEL + "464,232,116>"), ks
        assert h.range_status() == (False, False)
    finally:
        h.set_pw_config(-1)
        h.close()
