"""The split-f16 range guard (csrc/yn_split.h) at every place where a kernel splits an activation, through the whole network.

tests/range_cases.py heats ONE site of the network at a time (its producer's output f times larger, its consumers' weights f times smaller: the same
network downstream) so that, by the float64 oracle alone, a quiet image keeps what that site splits in (16 376, 32 752] and a loud image takes it beyond
131 008, with every other layer below 32 752 in both (tests/test_range_cases_cpu.py asserts all of this without a GPU).  Per site, and per launch-switch row
that moves the site into another kernel (range_cases.rows):

  ARMED   the loud image at index 0, in the middle and at B - 1 of an otherwise quiet batch: range_status() == (False, True), a second read (False, False), and
          the profile records hold the row's (layer record, kernel) pairs - the kernel whose tracking statement is under test really ran.  Only the site
          under test can have raised the flag: everything else is in range, and the NaN the overflowing split leaves downstream never raises it.
  QUIET   all images quiet: range_status() == (False, False), and every image's raw heads within f64_bar.bar (4 * e32 + 4 ulp, e32 from the float32 TorchNet)
          of the float64 TorchNet on the SAME heated state dict - fp32-class accuracy with an intermediate at up to half the f16 range (the rows that run
          yn_infer assert the flag and the counts; their heads are the raw rows' heads).
  GRAPH   one site per persistent kernel under yn_use_graph: the armed input raises the flag on a REPLAY, the quiet input in between does not.

The small cases (range_cases.SMALL) run 192 x 192 x 4 on 1.0x and 0.5x, and 128 x 128 x 3 with 80 classes (the head-tail kernel exists for 32 < C <= 80);
the persistent cases (range_cases.PERSISTENT) run each persistent kernel at the smallest batch of 224 x 224 images at which a workgroup walks two tiles.

Worst err / bar of the quiet runs per kernel family (the family of the row's kernel; all 915 RATIO lines of one MI355X run of this file, none above 0.27 - the
level of tests/test_gpu_wide.py's unheated networks, 0.22 ... 0.28: an intermediate at half the f16 range, read through weights 2^-9 ... 2^-11 of their usual
size, costs the split nothing):
  RATIO conv3x3_split_kernel    neck.p4p5  1.0x head8   err 1.539e-05  e32 1.562e-05  ulp 9.537e-07  err/bar 0.232
  RATIO down2_kernel            s3.0.b2.dw 1.0x head16  err 1.571e-05  e32 1.362e-05  ulp 9.537e-07  err/bar 0.269
  RATIO down_unit_pipe_kernel   stem       1.0x head8   err 1.538e-05  e32 1.595e-05  ulp 9.537e-07  err/bar 0.227
  RATIO dwpw_pipe_group_kernel  head1.0    1.0x head8   err 1.864e-05  e32 1.607e-05  ulp 1.907e-06  err/bar 0.259
  RATIO gemm_split_group_kernel head1.3    1.0x head8   err 1.719e-05  e32 1.607e-05  ulp 1.907e-06  err/bar 0.239
  RATIO gemm_split_kernel       head1.0    1.0x head8   err 1.864e-05  e32 1.607e-05  ulp 1.907e-06  err/bar 0.259
  RATIO pw_pipe_kernel          head1.0    1.0x head8   err 1.864e-05  e32 1.607e-05  ulp 1.907e-06  err/bar 0.259
  RATIO stage_pipe_kernel       s3.4.b2.dw 1.0x head8   err 1.775e-05  e32 1.595e-05  ulp 9.537e-07  err/bar 0.263
  RATIO unit_chain2_kernel      s2.3.b2.dw 1.0x head8   err 1.599e-05  e32 1.562e-05  ulp 9.537e-07  err/bar 0.241
  RATIO unit_pipe_kernel        s3.1.b2.dw 1.0x head16  err 1.464e-05  e32 1.362e-05  ulp 9.537e-07  err/bar 0.251
(head_tail_group_kernel, head_decode_group_kernel and head_decode_kernel run inside yn_infer and return candidates, not raw heads: their rows assert the flag, not this bar;
tests/test_gpu_decode_ops.py holds them to it on O(1) data.)

SENSITIVITY.  Tried once against three libraries that each drop ONE range_track statement (value-only changes); on each, the inference GPU files that existed before
this one (683 tests of test_gpu_parity, _infer_ops, _wide, _stage_geometry, _dwpw_pipe, _rect, _decode_ops, _down_unit_widths, _extras, _tta) all passed, and of the
125 tests of this file and the operator-level guard tests exactly these failed, every one with "did not raise the flag":
  (1) dwpw_pipe_block's depthwise output: head{1,2,3}.0 and head{1,2,3}.2 of all three small cases (the default rows, dwpw_pipe_group_kernel) and both persistent
      dwpw_pipe_group_kernel cases - 20 tests; head*.3 and everything else passed.
  (2) stage_pipe_kernel's depthwise output o[j]: the unit.dw sites of every stage that has a stage form - 1.0x s3.1 / s3.4, 0.5x s2.1 / s2.2 / s3.1 / s3.4 / s4.1 / s4.2 - at their
      yn_stage_fuse(2) rows, and both persistent stage_pipe_kernel b2.dw cases - 10 tests; the x2' sites of the same kernel (split2 kept its tracking) passed.
  (3) head_tail_block's second site (layer .3's output): head{1,2,3}.3 of the 80-class case at their yn_infer / head_tail_group_kernel row - 3 tests; head*.2 through the
      same kernel (its first site) passed.
"""
import functools

import numpy as np
import pytest
import torch

import range_cases as rc
from f64_bar import bar
from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def capi():
    from yolo_nano_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return c


@pytest.fixture(scope="module")
def stream():
    return torch.cuda.Stream()                               # graph capture needs a stream of the handle's own


_handles = {}


@pytest.fixture(scope="module")
def handles(capi, stream):
    """one handle per (backbone, classes, S, B), reloaded and refolded per site"""
    def get(bb, C, S, B):
        key = (bb, C, S, B)
        if key not in _handles:
            with torch.cuda.stream(stream):
                h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE_COCO if C == 80 else arch.MULTI_ANCHOR_SIZE, bb, 0.001, 0.5, max_batch=B)
            h.autotune(False)                                # the heuristic tile unless a row pins one: which kernel runs is the row's statement
            _handles[key] = h
        return _handles[key]
    yield get
    for h in _handles.values():
        h.close()
    _handles.clear()


@functools.lru_cache(maxsize=None)
def _state(bb, C):
    return weights.make_state_dict(bb, C)


@functools.lru_cache(maxsize=8)
def _problem(bb, C, S, name):
    """(f, the heated state dict, the quiet image's float64 heads NHWC [1, ...], the same in float32)"""
    from oracle.torch_port import TorchNet
    site = rc.site_by_name(bb, name)
    f, hot, pk, heads = rc.choose_f(_state(bb, C), site, bb, S, C)
    specs = {s.name: s for s in arch.conv_specs(bb, C)}
    assert rc.margins(site, pk, specs) is None, rc.margins(site, pk, specs)      # (test_range_cases_cpu.py's statement, on this machine's oracle)
    r32 = TorchNet(hot, bb, C).forward_raw(rc.pattern(S))
    nhwc = lambda t: t[:1].permute(0, 2, 3, 1).contiguous()
    return f, hot, [nhwc(t) for t in heads], [nhwc(t) for t in r32]


@functools.lru_cache(maxsize=2)
def _inputs(S, B):
    """the quiet batch and the loud image on the device: an armed batch is the quiet one with one image replaced"""
    p = torch.as_tensor(rc.pattern(S)).cuda()
    return p.expand(B, -1, -1, -1).contiguous(), (p * rc.LOUD)[0]


def _armed(S, B, at):
    quiet, loud = _inputs(S, B)
    x = quiet.clone()
    x[at] = loud
    return x


def _apply(h, sw):
    s = dict(rc.DEFAULTS)
    s.update(sw)
    h.unit_chain(s["unit_chain"]); h.chain_pipe(s["chain_pipe"]); h.stage_fuse(*s["stage_fuse"]); h.down_fuse(s["down_fuse"])
    h.group_launch(s["group_launch"]); h.tail_fuse(s["tail_fuse"]); h.fuse_decode(s["fuse_decode"])
    f32, split = h.pw_families()
    assert len(split) == rc.N_SPLIT_CONFIGS + 1, "the split family has %d configurations: restate range_cases.N_SPLIT_CONFIGS" % len(split)
    pc = s["pw_config"]
    h.set_pw_config(-1 if pc is None else (split[-1] if pc == "pipe" else split[pc]))


def _run(h, route, x):
    """one forward by the row's route -> (raw heads or None, counts or None)"""
    if route == "raw":
        return h.forward_raw(x), None
    out = h.infer(x)
    return None, out[4]


def _load(h, hot):
    h.load_state_dict(hot)
    h.fold_bn()
    assert h.range_status() == (False, False), "a folded weight of the heated network left the f16 range"


def _check_site(h, bb, C, S, B, name, row_list, graph=False):
    f, hot, r64, r32 = _problem(bb, C, S, name)
    _load(h, hot)
    quiet, _ = _inputs(S, B)
    tag0 = "%s %dx%dx%d %s f=%g" % (bb, S, S, B, name, f)
    try:
        for sw, route, expect in row_list:
            tag = "%s %s %s" % (tag0, sw, route)
            _apply(h, sw)
            # ---- armed ----
            for i, at in enumerate(rc.positions(B)):
                x = _armed(S, B, at)
                h.profile_enable(i == 0)
                try:
                    _run(h, route, x)
                    st = h.range_status()
                    recs = [(r[0], r[1]) for r in h.profile_records()] if i == 0 else None
                finally:
                    h.profile_enable(False)
                assert st == (False, True), "%s: the loud image at index %d of %d did not raise the flag" % (tag, at, B)
                assert h.range_status() == (False, False), "%s: the flag survived its read" % tag
                if recs is not None:
                    for rec, kern in expect:
                        assert any(n == rec and k.startswith(kern) for n, k in recs), "%s: no record %s with a %s...\n%s" % (tag, rec, kern, recs)
            # ---- quiet ----
            heads, counts = _run(h, route, quiet)
            assert h.range_status() == (False, False), "%s: a false alarm on the all-quiet batch" % tag
            if counts is not None:
                assert bool((counts >= 0).all()), tag
            else:
                fam = expect[0][1].split("<")[0]              # the RATIO lines carry the row's kernel family
                for hd, (got, a, b) in enumerate(zip(heads, r64, r32)):
                    bar(fam, "%s %s head%d" % (name, bb, 8 << hd), got.cpu(), a.expand(B, -1, -1, -1), b.expand(B, -1, -1, -1))
            # ---- graph replay: capture on the quiet input, then replays ----
            if graph and route == "raw":
                xb = quiet.clone()
                out = [torch.empty_like(t) for t in heads]
                h.use_graph(True)
                try:
                    h.forward_raw(xb, out=out)                                   # captured and launched
                    assert h.range_status() == (False, False), tag
                    for at in rc.positions(B):
                        xb.copy_(_armed(S, B, at)); torch.cuda.synchronize()
                        h.forward_raw(xb, out=out)                               # a replay
                        assert h.range_status() == (False, True), "%s: replay with the loud image at %d did not raise the flag" % (tag, at)
                        xb.copy_(quiet); torch.cuda.synchronize()
                        h.forward_raw(xb, out=out)
                        assert h.range_status() == (False, False), "%s: replay with the quiet batch raised the flag" % tag
                    for got, want in zip(out, heads):
                        assert torch.equal(got, want), "%s: the replayed quiet heads differ from the eager ones" % tag
                finally:
                    h.use_graph(False)
    finally:
        _apply(h, {})
        h.range_status()


def _small_ids():
    out = []
    for bb, C, S, B in rc.SMALL:
        for s in rc.sites(bb):
            if C == 80 and not s.kind.startswith("head."):
                continue                                     # the 80-class case is there for the heads' tail kernels
            out.append(pytest.param(bb, C, S, B, s.name, id="%s-c%d-%d-%s" % (bb, C, S, s.name)))
    return out


@pytest.mark.parametrize("bb,C,S,B,name", _small_ids())
def test_site_raises_the_flag(handles, stream, bb, C, S, B, name):
    site = rc.site_by_name(bb, name)
    with torch.cuda.stream(stream):
        _check_site(handles(bb, C, S, B), bb, C, S, B, name, rc.rows(site, bb, S, B, C))


def _persistent_ids():
    return [pytest.param(kern, name, id="%s-%s" % (kern, name)) for kern, v in list(rc.PERSISTENT.items()) + list(rc.LARGE.items()) for name in v[2]]


@pytest.mark.parametrize("kernel,name", _persistent_ids())
def test_persistent_walks_raise_the_flag(handles, stream, kernel, name):
    """The same at the batch where a workgroup of the persistent kernel walks two tiles: an amax reset per tile, or a report only the last tile reaches, loses the
    loud image when its tiles are not the last of their walk.  The first site of each kernel also runs under yn_use_graph.
    (range_cases.LARGE rides along: down2_kernel's unchained form, which only a large batch reaches.)"""
    bb, B, names, sw = rc.PERSISTENT.get(kernel) or rc.LARGE[kernel]
    S, C = rc.PERSISTENT_S, 20
    site = rc.site_by_name(bb, name)
    mine = [r for r in rc.rows(site, bb, S, B, C) if any(k.startswith(kernel) for _, k in r[2]) and all(r[0].get(k) == v for k, v in sw.items())]
    assert mine, "no row of %s runs %s under %s" % (name, kernel, sw)
    with torch.cuda.stream(stream):
        _check_site(handles(bb, C, S, B), bb, C, S, B, name, mine[:1], graph=name == names[0] and kernel in rc.PERSISTENT)
