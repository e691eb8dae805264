"""Rectangular inference on the device: grids set with yn_set_grid_rect - the H x W window at (left, top) of a letterboxed side x side square - through
the network, the decode front ends, yn_infer, the preprocess window and the consumers of the packed records.  tests/rect_cases.py holds the
convention restated in float64 (tied to decode_cases.decode_ref by tests/test_rect_cases_cpu.py), the data and the case tables.

Bars: raw heads against the torch-CPU oracle at test_size_sweep_vs_torch_oracle's 1e-4; scores and boxes inside f64_bar.bar (4 e32 + 4 ulp, e32 from the
float32 numpy evaluation of rect_ref), as tests/test_gpu_decode_ops.py applies them to square grids; everything else exact."""
import functools

import numpy as np
import pytest
import torch

import decode_cases as dc
import rect_cases as rc
from f64_bar import bar
from oracle import oracle as orc
from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu

ATOL = 1e-4                                                 # tests/test_gpu_parity.py: test_size_sweep_vs_torch_oracle


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def nchw_np(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    ia, ib = a.view(np.int32), b.view(np.int32)
    if not np.array_equal(ia, ib):
        bad = np.argwhere(ia != ib)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: %r against %r" % (what, len(bad), a.size, i, a[i], b[i]))


def _ran(h, fn):
    h.profile_enable(True)
    try:
        y = fn()
        torch.cuda.synchronize()
        names = [r[1] for r in h.profile_records()]
    finally:
        h.profile_enable(False)
    return [t.cpu().numpy() for t in y], names


def _names(h, fn):
    h.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[1] for r in h.profile_records()]
    finally:
        h.profile_enable(False)


@pytest.fixture(scope="module")
def capi():
    from yolo_nano_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return c


@functools.lru_cache(maxsize=None)
def _state_dict(backbone, C):
    return weights.make_state_dict(backbone, C)


@functools.lru_cache(maxsize=None)
def _torch_net(backbone, C):
    from oracle.torch_port import TorchNet
    return TorchNet(_state_dict(backbone, C), backbone, C)


@pytest.fixture(scope="module")
def net_handle(capi):
    """a handle per backbone with the weights loaded, autotuning off (every configuration gives the same bits; timing them would dominate)"""
    cache = {}

    def get(backbone, C):
        if (backbone, C) not in cache:
            anchors = arch.MULTI_ANCHOR_SIZE_COCO if C == 80 else arch.MULTI_ANCHOR_SIZE
            h = capi.Handle(128, C, anchors, backbone, 0.001, 0.5, max_batch=3)
            h.autotune(False)
            h.load_state_dict(_state_dict(backbone, C))
            h.fold_bn()
            cache[(backbone, C)] = h
        return cache[(backbone, C)]
    yield get
    for h in cache.values():
        h.close()


# =====================================================================================================================================
# 1. the network
# =====================================================================================================================================
@pytest.mark.parametrize("H,W,B", rc.NET_SHAPES)
@pytest.mark.parametrize("backbone,C", rc.NET_BACKBONES)
def test_network_vs_torch_oracle(net_handle, backbone, C, H, W, B):
    h = net_handle(backbone, C)
    h.set_grid_rect(H, W)
    assert h.shape == (H, W) + rc.default_window(H, W) and h.S is None and h.N == rc.num_pred(H, W)
    x = rc.make_input(B, H, W, seed=H // 32 + 31 * (W // 32))
    ref = _torch_net(backbone, C).forward_raw(x)
    got = h.forward_raw(dev(x))
    for s, (g, r) in enumerate(zip(got, ref)):
        assert tuple(g.shape) == (B, H // arch.STRIDES[s], W // arch.STRIDES[s], 3 * (5 + C))
        np.testing.assert_allclose(nchw_np(g), np.asarray(r), atol=ATOL, rtol=0, err_msg="%s %dx%d B=%d scale %d" % (backbone, H, W, B, s))
    assert h.range_status() == (False, False)
    taps = h.forward_taps(dev(x))
    assert [tuple(t.shape[1:3]) for t in taps] == [(H // s, W // s) for s in arch.STRIDES]


# =====================================================================================================================================
# 2. the forms that are pinned bit-identical on square grids
# =====================================================================================================================================
@pytest.mark.parametrize("H,W,B", rc.FORM_SHAPES)
@pytest.mark.parametrize("backbone,C", rc.NET_BACKBONES)
def test_forms_are_bit_identical(capi, backbone, C, H, W, B):
    anchors = arch.MULTI_ANCHOR_SIZE_COCO if C == 80 else arch.MULTI_ANCHOR_SIZE
    h = capi.Handle(128, C, anchors, backbone, 0.001, 0.5, max_batch=B)
    try:
        h.autotune(False)
        h.load_state_dict(_state_dict(backbone, C))
        h.fold_bn()
        h.set_grid_rect(H, W, 640, 16, 48)
        x = dev(rc.make_input(B, H, W, seed=H + 3 * B))
        tag = "%s %dx%d" % (backbone, H, W)
        # ---- unit_pipe_kernel / stage_pipe_kernel against one unit_chain2_kernel launch per unit
        h.stage_fuse(0); h.chain_pipe(0)
        ref = [t.clone() for t in h.forward_raw(x)]
        names = _names(h, lambda: h.forward_raw(x))
        assert not any(n.startswith(("unit_pipe_kernel", "stage_pipe_kernel")) for n in names), names
        h.chain_pipe(2)
        for rep in range(3):
            for u, v in zip(h.forward_raw(x), ref):
                assert torch.equal(u, v), (tag, "chain_pipe", rep)
        names = _names(h, lambda: h.forward_raw(x))
        assert any(n.startswith("unit_pipe_kernel") for n in names), names
        for publish_early in (True, False):
            h.chain_pipe(1); h.stage_fuse(2, publish_early)
            for rep in range(3):
                for u, v in zip(h.forward_raw(x), ref):
                    assert torch.equal(u, v), (tag, "stage_fuse", publish_early, rep)
            names = _names(h, lambda: h.forward_raw(x))
            for prefix in rc.STAGE_FORMS[(backbone, H, W)]:
                assert any(n.startswith(prefix + ("true" if publish_early else "false")) for n in names), (tag, prefix, names)
        h.stage_fuse(1); h.chain_pipe(1)
        # ---- pw_pipe_kernel against gemm_split_kernel's first configuration
        _, split_fam = h.pw_families()
        h.set_pw_config(split_fam[0])
        refp = [t.clone() for t in h.forward_raw(x)]
        h.set_pw_config(split_fam[-1])
        for rep in range(3):
            for u, v in zip(h.forward_raw(x), refp):
                assert torch.equal(u, v), (tag, "pw_pipe", rep)
        names = _names(h, lambda: h.forward_raw(x))
        assert any(n.startswith("pw_pipe_kernel") for n in names), names
        h.set_pw_config(-1)
        # ---- fused against unfused decode: head_decode*, then head_tail_group_kernel where its rule takes the class count (else its fallback)
        h.tail_fuse(False); h.fuse_decode(False)
        refd = [t.clone() for t in h.infer(x)]
        counts = refd[4].cpu().tolist()
        assert sum(counts) > 0
        names = _names(h, lambda: h.infer(x))
        assert any(n.startswith("decode_kernel") for n in names) and not any(n.startswith(("head_decode", "head_tail")) for n in names), names
        for tail, want in ((False, "head_decode_group_kernel"), (True, "head_tail_group_kernel" if dc.head_tail_ok(C) else "head_decode_group_kernel")):
            h.tail_fuse(tail); h.fuse_decode(2)
            for rep in range(3):
                got = h.infer(x)
                assert got[4].cpu().tolist() == counts, (tag, tail, rep)
                for b in range(B):
                    for r, g_ in zip(refd[:4], got[:4]):
                        assert torch.equal(r[b, :counts[b]], g_[b, :counts[b]]), (tag, tail, rep, b)
            names = _names(h, lambda: h.infer(x))
            assert any(n.startswith(want) for n in names) and not any(n.startswith("decode_kernel") for n in names), (tag, tail, names)
        assert h.range_status() == (False, False)
    finally:
        h.close()


# =====================================================================================================================================
# 3. the decode front ends
# =====================================================================================================================================
def _box_checks(tag, got, r64, r32):
    ratio = bar("box", tag, _t(got), _t(r64["all_bbox"]), _t(r32["all_bbox"]))
    e32 = float(np.abs(r32["all_bbox"].astype(np.float64) - r64["all_bbox"]).max())
    b = 4 * e32 + 4 * float(np.spacing(np.float32(1.0)))
    pre = r64["pre_clamp"]
    assert (got[pre < -b] == 0.0).all() and (got[pre > 1 + b] == 1.0).all(), tag      # a clamped coordinate is exactly the bound
    assert (got >= 0).all() and (got <= 1).all(), tag
    return ratio


def _score_checks(tag, C, conf, scores, cls, r64, r32):
    obj_raw, s64 = r64["obj_raw"], r64["score"]
    nan = np.isnan(obj_raw)
    L = dc.skip_logit(conf)
    must_zero, live = obj_raw < L - 1e-4, (obj_raw > L + 1e-4)
    assert (scores[must_zero] == 0.0).all() and (cls[must_zero] == -1).all(), tag
    assert np.isnan(scores[nan]).all() and (cls[nan] == -1).all(), tag
    z = lambda a: np.where(live, np.nan_to_num(a.astype(np.float64), nan=0.0), 0.0)
    ratio = bar("score", tag, _t(z(scores)), _t(z(s64)), _t(z(r32["score"])))
    sb = dc.score_bar(r64, r32)
    excused = dc.near_tie_mask(r64, r32)
    above, under = live & (s64 >= conf + sb) & ~excused, live & (s64 < conf - sb)
    bad = above & (cls != r64["best"])
    assert not bad.any(), (tag, "class", np.argwhere(bad)[:5], cls[bad][:5], r64["best"][bad][:5])
    assert (cls[under] == -1).all(), tag
    assert ((cls >= -1) & (cls < C)).all(), tag
    return ratio


DECODE_PARAMS = [(C, H, W, win) for C in rc.DECODE_C for H, W in rc.DECODE_GRIDS for win in ("default", "s192", "corner")]
DECODE_PARAMS += [(C, rc.WHOLE_SQUARE, rc.WHOLE_SQUARE, "whole") for C in rc.DECODE_C]


def _window(H, W, win):
    return (H, 0, 0) if win == "whole" else rc.decode_windows(H, W)[win]


@pytest.fixture(scope="module")
def decode_handle(capi):
    cache = {}

    def get(C):
        if C not in cache:
            cache[C] = capi.Handle(64, C, arch.MULTI_ANCHOR_SIZE, max_batch=rc.B)
        return cache[C]
    yield get
    for h in cache.values():
        h.close()


@pytest.mark.parametrize("kind", ["random", "steered"])
@pytest.mark.parametrize("C,H,W,win", DECODE_PARAMS)
def test_decode_vs_float64(decode_handle, C, H, W, win, kind):
    side, left, top = _window(H, W, win)
    h = decode_handle(C)
    if win == "default":
        h.set_grid_rect(H, W)
    else:
        h.set_grid_rect(H, W, side, left, top)
    assert h.shape == (H, W, side, left, top) and h.N == rc.num_pred(H, W) and (h.S == side) == (win == "whole")
    heads = rc.random_heads(C, H, W) if kind == "random" else rc.steered_heads(C, H, W)
    conf = dc.CONF_RANDOM if kind == "random" else dc.CONF_STEERED
    r64, r32 = rc.rect_ref(heads, H, W, side, left, top, C), rc.rect_ref(heads, H, W, side, left, top, C, np.float32)
    hd = [torch.from_numpy(t).cuda() for t in heads]
    tag = "c%d %dx%d %s %s" % (C, H, W, win, kind)
    (bbox, allc), names = _ran(h, lambda: h.score_full(hd))
    assert names == [dc.decode_kernel(C, True)], names
    nan = np.isnan(r64["obj_raw"])
    assert np.isnan(allc[nan]).all() and not np.isnan(allc[~nan]).any(), tag
    z = lambda a: np.where(nan[..., None], 0.0, a.astype(np.float64))
    bar("allcls", tag, _t(z(allc)), _t(z(r64["all_class"])), _t(z(r32["all_class"])))
    _box_checks(tag + " full", bbox, r64, r32)
    (boxes, scores, cls), names = _ran(h, lambda: h.op_decode_cand(hd, conf))
    assert names == [dc.decode_kernel(C, False)], names
    _box_checks(tag + " cand", boxes, r64, r32)
    _score_checks(tag, C, conf, scores, cls, r64, r32)
    _bits_equal(boxes, bbox, tag + " boxes against all_bbox")
    if kind == "steered":                                   # the window's offset meets the clamp on both sides
        assert (r64["pre_clamp"] < -1e-3).any() and (r64["pre_clamp"] > 1 + 1e-3).any(), tag
    else:
        # yn_decode_boxes: canvas pixels, no offset
        t = np.concatenate([x.reshape(rc.B, -1, rc.A, 4) for x in (hh[..., rc.A * (1 + C):] for hh in heads)], 1)
        px = h.decode_boxes(torch.from_numpy(np.ascontiguousarray(t)).cuda()).cpu().numpy()
        bar("pixels", tag, _t(px), _t(r64["pixels"]), _t(r32["pixels"]))
    if win == "whole":                                      # the whole-square window IS the square grid: today's bits
        h.set_grid(H)
        (bbox2, allc2), _ = _ran(h, lambda: h.score_full(hd))
        _bits_equal(bbox2, bbox, tag + " set_grid boxes")
        _bits_equal(allc2, allc, tag + " set_grid scores")
        d = dc.decode_ref(heads, H, C)
        assert np.array_equal(d["all_bbox"], r64["all_bbox"])


@pytest.fixture(scope="module")
def tail_handle(capi):
    cache = {}

    def get(C, kind):
        if (C, kind) not in cache:
            sd, conf = dc.random_state_dict(C), dc.CONF_RANDOM
            if kind == "steered":
                sd, conf = dc.steered_state_dict(sd, C), dc.CONF_STEERED
            h = capi.Handle(64, C, arch.MULTI_ANCHOR_SIZE, conf_thresh=conf, max_batch=rc.B)
            h.autotune(False)
            h.load_state_dict(sd)
            h.fold_bn()
            cache[(C, kind)] = (h, conf)
        return cache[(C, kind)]
    yield get
    for h, _ in cache.values():
        h.close()


@pytest.mark.parametrize("kind", ["random", "steered"])
@pytest.mark.parametrize("C,H,W,win", DECODE_PARAMS)
def test_front_ends_are_bit_identical(tail_handle, C, H, W, win, kind):
    """yn_op_head_tail under every setting of yn_tail_fuse x yn_fuse_decode x yn_group_launch against yn_op_decode_cand on raw heads computed from the
    same activations, layer by layer, with the handle's folded weights: all B * N candidates bit for bit, the kernel the rules name"""
    side, left, top = _window(H, W, win)
    h, conf = tail_handle(C, kind)
    h.set_grid_rect(H, W, side, left, top)
    acts = rc.random_acts(H, W) if kind == "random" else rc.steered_acts(C, H, W)
    xs = [torch.from_numpy(x).cuda() for x in acts]
    tag = "c%d %dx%d %s %s" % (C, H, W, win, kind)
    shapes = ((dc.NECK, 1, 3, 3), (dc.NECK, dc.NECK, 1, 1), (dc.A * (5 + C), dc.NECK, 1, 1))
    raws = []
    for hd, x in enumerate(xs):
        lay = [h.get_folded(conv, shp) for (conv, _), shp in zip(dc.head_keys(hd + 1), shapes)]
        (wd, bd), (wp, bp), (wf, bf) = [(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()) for w, b in lay]
        raws.append(h.op_pwconv(h.op_pwconv(h.op_dwconv3x3(x, wd, bd, 1, 2), wp, bp, 2), wf, bf, 0))
    raw_np = [r.cpu().numpy() for r in raws]
    (rb, rs, rcl), names = _ran(h, lambda: h.op_decode_cand(raws, conf))
    assert names == [dc.decode_kernel(C, False)], names
    try:
        for tail, fuse, group in dc.SWITCHES:
            h.tail_fuse(tail); h.fuse_decode(fuse); h.group_launch(group)
            (boxes, scores, cls), names = _ran(h, lambda: h.op_head_tail(xs))
            ran = [n for n in names if dc.is_decode_kernel(n)]
            assert ran == rc.front_end(C, H, W, tail, fuse, group), (tag, (tail, fuse, group), names)
            what = "%s tail %d fuse %d group %d (%s)" % (tag, tail, fuse, group, ran[0])
            _bits_equal(boxes, rb, what + " boxes")
            _bits_equal(scores, rs, what + " scores")
            assert np.array_equal(cls, rcl), what
    finally:
        h.tail_fuse(True); h.fuse_decode(True); h.group_launch(True)
    r64, r32 = rc.rect_ref(raw_np, H, W, side, left, top, C), rc.rect_ref(raw_np, H, W, side, left, top, C, np.float32)
    _box_checks(tag + " raw", rb, r64, r32)
    _score_checks(tag + " raw", C, conf, rs, rcl, r64, r32)


# =====================================================================================================================================
# 4. end to end
# =====================================================================================================================================
def _infer_vs_oracle(h, x, conf_t, nms_t, diou=False):
    h.set_thresholds(conf_t, nms_t, diou)
    out = h.infer(x)
    heads = h.forward_raw(x)
    bbox, cls = h.score_full(heads)
    counts = out[4].cpu().tolist()
    for b in range(x.shape[0]):
        rb, rs, rcl, ri = orc.postprocess(bbox[b].cpu().numpy(), cls[b].cpu().numpy(), conf_t, nms_t, diou=diou, return_index=True)
        k = counts[b]
        assert k == len(rs), (b, k, len(rs))
        assert np.array_equal(out[3][b, :k].cpu().numpy().astype(np.int64), ri)
        assert np.array_equal(out[0][b, :k].cpu().numpy(), rb)
        assert np.array_equal(out[1][b, :k].cpu().numpy(), rs)
        assert np.array_equal(out[2][b, :k].cpu().numpy().astype(np.int64), rcl)
    return out, counts


@pytest.mark.parametrize("diou", [False, True])
def test_infer_equals_oracle_postprocess(net_handle, diou):
    h = net_handle("1.0x", 20)
    h.set_grid_rect(64, 160, 192, 13, 71)
    x = dev(rc.make_input(3, 64, 160, seed=3))
    try:
        out, counts = _infer_vs_oracle(h, x, 0.001, 0.5, diou)
        assert min(counts) > 0
        b = out[0][0, :counts[0]].cpu().numpy()              # normalised to the 192 square: inside the window's share of it
        assert b[:, [0, 2]].min() >= 0 and b[:, [1, 3]].max() <= 1 and (b[:, 3] > 71 / 192).all() and (b[:, 1] < (71 + 64) / 192).all()
    finally:
        h.set_thresholds(0.001, 0.5, False)


def test_whole_square_window_is_the_square_grid(net_handle):
    h = net_handle("1.0x", 20)
    x = dev(weights.make_input(3, 128, seed=9))
    h.set_grid(128)
    assert h.S == 128 and h.shape == (128, 128, 128, 0, 0)
    ref_raw = [t.clone() for t in h.forward_raw(x)]
    ref = [t.clone() for t in h.infer(x)]
    h.set_grid_rect(128, 128, 128, 0, 0)
    assert h.S == 128 and h.shape == (128, 128, 128, 0, 0)
    for u, v in zip(h.forward_raw(x), ref_raw):
        assert torch.equal(u, v)
    got = h.infer(x)
    assert torch.equal(got[4], ref[4]) and int(ref[4].min()) > 0
    for b in range(3):
        k = int(ref[4][b])
        for r, g_ in zip(ref[:4], got[:4]):
            assert torch.equal(r[b, :k], g_[b, :k])
    h.set_grid_rect(128, 128)                               # side = 0 of a square canvas is the whole square too
    assert h.S == 128


def test_graph_replay_follows_the_window(net_handle):
    """square 128 -> rect (64, 160) -> the same rect in another window -> square 128, one batch size, fixed buffers: every step the eager result"""
    h = net_handle("1.0x", 20)
    B = 2
    xs = {128: dev(weights.make_input(B, 128, seed=4)), 160: dev(rc.make_input(B, 64, 160, seed=5))}
    steps = [("sq", 128, 128, 128, 0, 0), ("rect", 64, 160, 160, 0, 48), ("rect2", 64, 160, 192, 13, 71), ("sq", 128, 128, 128, 0, 0)]

    def run(step, bufs=None):
        _, H, W, side, left, top = step
        h.set_grid_rect(H, W, side, left, top)
        o = h.infer(xs[W], None if bufs is None else bufs[W][0])
        raw = h.forward_raw(xs[W], None if bufs is None else bufs[W][1])
        torch.cuda.synchronize()
        return [t.clone() for t in o], [t.clone() for t in raw]

    h.use_graph(False)
    eager = [run(s) for s in steps]
    assert not torch.equal(eager[1][0][0], eager[2][0][0])    # the two windows give different boxes: a stale graph would show
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            h.set_stream(st)
            h.use_graph(True)
            bufs = {}
            for s in steps[:2]:                                 # fixed buffers per canvas: both windows of the rect share x, outputs and B
                h.set_grid_rect(*s[1:])
                bufs[s[2]] = (h.alloc_outputs(B), [torch.empty(shp, dtype=torch.float32, device="cuda") for shp in h.head_shapes(B)])
            for rnd in range(3):                                # capture, then replays
                for s, (eo, er) in zip(steps, eager):
                    o, raw = run(s, bufs)
                    assert torch.equal(o[4], eo[4]), (rnd, s)
                    for b in range(B):
                        k = int(eo[4][b])
                        for r, g_ in zip(eo[:4], o[:4]):
                            assert torch.equal(r[b, :k], g_[b, :k]), (rnd, s, b)
                    for u, v in zip(raw, er):
                        assert torch.equal(u, v), (rnd, s)
            st.synchronize()
    finally:
        h.use_graph(False)
        h.set_stream(torch.cuda.current_stream())


# =====================================================================================================================================
# 5. the preprocess window
# =====================================================================================================================================
def test_preprocess_window_is_the_slice(capi):
    from yolo_nano_amd import ValTransforms, rect_window
    h = capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x")
    try:
        rng = np.random.RandomState(3)
        side = 160
        tf = ValTransforms(side, handle=h)
        mean, std = tf.mean, tf.std
        frames = [rng.randint(0, 256, size=(h0, w0, 3)).astype(np.uint8) for h0, w0 in rc.FRAMES_16_9 + ((180, 320),)]   # linear, linear, linear, 2:1 ...
        frames.append(rng.randint(0, 256, size=(90, 160, 3)).astype(np.uint8))                                           # ... and a same-size copy
        imgs = [dev(f) for f in frames]
        geoms = [tf.geometry(f.shape[0], f.shape[1])[:4] for f in frames]
        assert geoms[3] == (160, 90, 0, 35) and frames[3].shape[:2] == (180, 320) and geoms[4] == (160, 90, 0, 35)
        full = h.preprocess_batch(imgs, geoms, side, mean, std)
        win = rect_window(geoms, side)
        assert win == (0, 32, 160, 96)
        for left, top, W, H in (win, (0, 0, 160, 160), (0, 32, 160, 128)):
            got = h.preprocess_batch_rect(imgs, geoms, side, (left, top, W, H), mean, std)
            assert tuple(got.shape) == (len(frames), 3, H, W)
            _bits_equal(got.cpu().numpy(), full[:, :, top:top + H, left:left + W].contiguous().cpu().numpy(), "window %r" % ((left, top, W, H),))
        # pad on all four sides: a small picture in the middle of the square
        small = [dev(rng.randint(0, 256, size=(40, 60, 3)).astype(np.uint8)), dev(rng.randint(0, 256, size=(50, 50, 3)).astype(np.uint8))]
        sg = [(60, 40, 50, 60), (32, 32, 64, 64)]
        full = h.preprocess_batch(small, sg, side, mean, std)
        got = h.preprocess_batch_rect(small, sg, side, (32, 32, 96, 96), mean, std)
        _bits_equal(got.cpu().numpy(), full[:, :, 32:128, 32:128].contiguous().cpu().numpy(), "pad on four sides")
        assert (full[:, :, :32] == full[:, :, :1, :1]).all()
        # a window that cuts a frame, and one outside the square
        for bad in ((0, 64, 160, 64), (0, 32, 128, 96), (0, 36, 160, 96)):
            with pytest.raises(capi.YnError, match="cuts image 0"):
                h.preprocess_batch_rect(imgs, geoms, side, bad, mean, std)
        with pytest.raises(capi.YnError, match="outside"):
            h.preprocess_batch_rect(imgs, geoms, side, (0, 96, 160, 96), mean, std)
        # ValTransforms.batch(rect=True) is that call
        x, g7, w = tf.batch(frames[:3], rect=True)
        assert w == win and g7 == [(f.shape[1], f.shape[0], 160, 90, 0, 35, side) for f in frames[:3]]
        _bits_equal(x.cpu().numpy(), h.preprocess_batch(imgs[:3], geoms[:3], side, mean, std)[:, :, 32:128].contiguous().cpu().numpy(), "ValTransforms.batch(rect=True)")
    finally:
        h.close()


# =====================================================================================================================================
# 6. downstream of the packed records: the unchanged 7-field geometry
# =====================================================================================================================================
def _model(S, C=20):
    import yolo_nano_amd
    sd = dict(_state_dict("1.0x", C))
    for hd in (1, 2, 3):                                        # YOLONano.init_bias (models/yolo_nano.py:77-83)
        sd["head_det_%d.4.bias" % hd] = sd["head_det_%d.4.bias" % hd].copy()
        sd["head_det_%d.4.bias" % hd][:3] = -4.595
    m = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, conf_thresh=0.001, nms_thresh=0.5, anchor_size=arch.MULTI_ANCHOR_SIZE)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return m.to("cuda").eval()


def test_records_of_a_rect_run_through_eval_and_painter():
    import json
    import os
    import draw_oracle
    import voc_oracle
    import yolo_nano_amd
    from yolo_nano_amd import ValTransforms, VOCEval, voc_geometry
    S, C = 160, 20
    m = _model(S, C)
    rng = np.random.RandomState(11)
    images = [rng.randint(0, 256, size=(h0, w0, 3)).astype(np.uint8) for h0, w0 in rc.FRAMES_16_9]
    h = m.handle(4)
    x, geoms, (left, top, W, H) = ValTransforms(S, handle=h).batch(images, rect=True)
    assert (left, top, W, H) == (0, 32, 160, 96) and geoms == [voc_geometry(im.shape[0], im.shape[1], S) for im in images]
    m.set_grid((H, W)); m.set_window(S, left, top)
    h = m.handle(4)
    assert h.shape == (96, 160, 160, 0, 32) and h.S is None
    out = h.infer(x)
    rec, off = h.pack_detections(out)
    dets = h.detections_to_host(out)
    assert min(len(d[1]) for d in dets) > 0
    # the model's own forward_batch on the rect tensor is that result
    for (b0, s0, c0), (b1, s1, c1) in zip(m.forward_batch(x), dets):
        assert np.array_equal(b0, b1) and np.array_equal(s0, s1) and np.array_equal(c0, c1)
    assert [tuple(t.shape) for t in m.forward_raw(x)] == [(3, 75, 96 // s, 160 // s) for s in arch.STRIDES]
    # ---- VOCEval
    ev = VOCEval(C, handle=h)
    ev.add(rec, off, geoms, [None] * len(images), handle=h)
    offs = np.cumsum([0] + [len(d[1]) for d in dets])
    want = voc_oracle.ingest(np.concatenate([d[0] for d in dets]), np.concatenate([d[1] for d in dets]), np.concatenate([d[2] for d in dets]), offs, geoms)
    got = ev.records()
    assert got.shape == want.shape and np.array_equal(got, want)
    ev.close()
    # ---- Visualizer
    names = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_names.json")))["voc"]
    thr = float(np.median(np.concatenate([d[1] for d in dets])))
    vis = yolo_nano_amd.Visualizer(names, yolo_nano_amd.class_colors(C), vis_thresh=thr, handle=h)
    frames = [dev(im.copy()) for im in images]
    vis.batch(frames, rec, off, geoms)
    rows = [np.concatenate([d[0], d[1][:, None], d[2][:, None].astype(np.float32)], 1).astype(np.float32) for d in dets]
    wantp = [(b,) + p for b in range(len(images)) for p in draw_oracle.select(rows[b], geoms[b], draw_oracle.LETTERBOX, thr, C)[0]]
    gotp = vis.prims()
    assert len(wantp) >= 1 and gotp.tolist() == [list(p) for p in wantp]
    for b, im in enumerate(images):
        exp = draw_oracle.draw(im, rows[b], geoms[b], draw_oracle.LETTERBOX, thr, vis.colors, vis.labels, vis.font, vis.thickness)[0]
        assert np.array_equal(frames[b].cpu().numpy(), exp), b
    # ---- training entries of the model on a rect grid
    from yolo_nano_amd.capi import YnError
    with pytest.raises(YnError, match="square grid"):
        m.make_targets([[] for _ in images])
    m.trainable = True
    with pytest.raises(YnError, match="square grid"):
        m(x, torch.zeros((3, h.N, 11), device="cuda"))
    m.trainable = False
    m.set_grid(S)
    assert m.handle(4).S == S


def test_mixed_aspect_batch_is_the_square_route():
    from yolo_nano_amd import ValTransforms
    S = 160
    m = _model(S)
    rng = np.random.RandomState(12)
    images = [rng.randint(0, 256, size=(h0, w0, 3)).astype(np.uint8) for h0, w0 in rc.FRAMES_16_9[:2] + ((160, 90),)]
    h = m.handle(4)
    tf = ValTransforms(S, handle=h)
    ref = m.forward_batch(tf.batch(images)[0])
    x, geoms, (left, top, W, H) = tf.batch(images, rect=True)
    assert (left, top, W, H) == (0, 0, S, S)
    m.set_grid((H, W)); m.set_window(S, left, top)
    assert m.handle(4).S == S                               # the whole-square window is the square grid
    got = m.forward_batch(x)
    assert min(len(d[1]) for d in ref) > 0
    for (b0, s0, c0), (b1, s1, c1) in zip(ref, got):
        assert np.array_equal(b0, b1) and np.array_equal(s0, s1) and np.array_equal(c0, c1)


def _pixel_boxes(dets, geoms, n=4):
    """the first n detections of every image in pixels of its frame (the evaluators' unletterbox: (box - offset) / scale * size)"""
    import voc_oracle
    out = []
    for (bb, sc, cl), g in zip(dets, geoms):
        scale, offset, size = voc_oracle.geometry_arrays(g)
        px = (bb[:n].astype(np.float64) - offset) / scale * size
        out.append((np.clip(px, 0, None), cl[:n]))
    return out


def test_evaluators_rect_option():
    """evaluate / evaluate_coco with rect=True: a batch with a portrait frame gets the whole square, which is the square route - the same APs exactly;
    batches of 16:9 frames run on their 160 x 96 window; the model's square grid is back afterwards"""
    from yolo_nano_amd import ValTransforms, evaluate, evaluate_coco, voc_geometry
    S = 160
    m = _model(S)
    rng = np.random.RandomState(13)
    mixed = [rng.randint(0, 256, size=(h0, w0, 3)).astype(np.uint8) for h0, w0 in (rc.FRAMES_16_9[:2] + ((160, 90),)) * 2]
    wide = [rng.randint(0, 256, size=(h0, w0, 3)).astype(np.uint8) for h0, w0 in rc.FRAMES_16_9 * 2]
    for images in (mixed, wide):
        geoms = [voc_geometry(im.shape[0], im.shape[1], S) for im in images]
        dets = m.forward_batch(ValTransforms(S, handle=m.handle(6)).batch(images)[0])
        px = _pixel_boxes(dets, geoms)
        voc_gt = [np.concatenate([np.rint(b), c[:, None], np.zeros((len(c), 1))], 1).astype(np.int32) for b, c in px]
        for g in voc_gt:
            g[:, 2:4] = np.maximum(g[:, 2:4], g[:, 0:2] + 2)
        coco_gt = [np.concatenate([b[:, :2], np.maximum(b[:, 2:] - b[:, :2], 1.0), (np.maximum(b[:, 2:] - b[:, :2], 1.0)).prod(1, keepdims=True), c[:, None],
                                   np.zeros((len(c), 1))], 1).astype(np.float64) for b, c in px]
        ids = list(range(11, 11 + len(images)))
        aps, mAP = evaluate(m, images, voc_gt, batch=3)
        aps_r, mAP_r = evaluate(m, images, voc_gt, batch=3, rect=True)
        assert m.input_size == S and m.handle(3).S == S
        c50, c = evaluate_coco(m, images, ids, coco_gt, batch=3)
        c50_r, c_r = evaluate_coco(m, images, ids, coco_gt, batch=3, rect=True)
        assert m.input_size == S and m.handle(3).S == S
        assert np.nanmax(aps) > 0 and c50 > 0
        assert len(aps_r) == 20 and np.isfinite(mAP_r) and np.isfinite(c50_r) and np.isfinite(c_r)
        if images is mixed:
            assert np.array_equal(np.asarray(aps), np.asarray(aps_r), equal_nan=True) and mAP == mAP_r and (c50, c) == (c50_r, c_r)
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate(m, mixed, [None] * len(mixed), rect=True, test_aug=object())


# =====================================================================================================================================
# 7. refusals
# =====================================================================================================================================
def test_refusals(capi, net_handle):
    h = net_handle("1.0x", 20)
    h.set_grid_rect(64, 160, 192, 13, 71)
    shape = h.shape
    for bad in ((64, 150), (60, 160), (0, 160), (64, -32), (48, 160)):
        with pytest.raises(capi.YnError, match="multiples of 32"):
            h.set_grid_rect(*bad)
        assert h.shape == shape
    for bad in ((64, 160, 128, 0, 0), (64, 160, 192, 33, 0), (64, 160, 192, 0, 129), (64, 160, 192, -1, 0), (64, 160, 192, 0, -1), (64, 160, -192, 0, 0)):
        with pytest.raises(capi.YnError, match="outside"):
            h.set_grid_rect(*bad)
        assert h.shape == shape
    B, N = 2, h.N
    x = dev(rc.make_input(B, 64, 160, seed=1))
    heads = h.forward_raw(x)
    target = torch.zeros((B, N, 11), device="cuda")
    C = 20
    conf, cls, txty = torch.zeros((B, N, 1), device="cuda"), torch.zeros((B, N, C), device="cuda"), torch.zeros((B, N, 4), device="cuda")
    calls = {
        "yn_loss": lambda: h.loss(conf, cls, txty, target),
        "yn_loss_heads": lambda: h.loss_heads(heads, target),
        "yn_make_targets": lambda: h.make_targets([[[0.1, 0.1, 0.5, 0.5, 1]], []], arch.MULTI_ANCHOR_SIZE),
        "yn_train_forward": lambda: h.lib.yn_train_forward(h.h, x.data_ptr(), B, heads[0].data_ptr(), heads[1].data_ptr(), heads[2].data_ptr()),
        "yn_train_step": lambda: h.lib.yn_train_step(h.h, x.data_ptr(), target.data_ptr(), B, 0.0, 0.0, 0.0, 1.0, 0, None),
    }
    for name, fn in calls.items():
        names = []
        h.profile_enable(True)
        try:
            try:
                rc_ = fn()
            except capi.YnError as e:
                msg = str(e)
            else:
                assert rc_ == 1, name
                msg = h.lib.yn_last_error(h.h).decode()
            names = h.profile_records()
        finally:
            h.profile_enable(False)
        assert "square grid" in msg and name in msg, (name, msg)
        assert names == [], (name, names)                   # nothing launched
        assert h.shape == shape, name
    tta = capi.Tta(h, [64, 96], flip=True, max_batch=1)
    try:
        with pytest.raises(capi.YnError, match="yn_tta_infer needs a square grid"):
            tta.infer(dev(weights.make_input(1, 96, seed=2)), 0.5)
        assert h.shape == shape                                 # it leaves the grid it found
    finally:
        tta.close()
    # the same entries are back on a square grid
    h.set_grid(128)
    assert h.make_targets([[[0.1, 0.1, 0.5, 0.5, 1]], []], arch.MULTI_ANCHOR_SIZE).shape == (2, h.N, 11)
