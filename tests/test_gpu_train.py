"""GPU parity of the training step (train.py:212-231): yn_train_step against
  (1) the reference's own recorded step (tests/golden/train.npz, made by tests/golden/gen_golden.py from the reference
      model + tools.loss + torch.optim.SGD), and
  (2) the torch-CPU oracle (oracle/torch_port.TrainNet) for EVERY parameter gradient.
Tolerances: losses 2e-4 relative; the train-mode network amplifies fp32 round-off (the reference's own recorded gradient
is up to 2e-2 * max|g| away from the fp64 oracle's exact one), so every gradient has to be as close to exact as the
reference's fp32 run is (x3) and within 2x that error of the reference's recorded gradient; parameters after SGD to
lr * that bound; BN running statistics 1e-4."""
import numpy as np
import pytest
import torch

from yolo_nano_amd import arch, weights

pytestmark = pytest.mark.gpu


def _handle(S, C, B, bias_value, backbone="1.0x"):
    from yolo_nano_amd import capi
    sd = weights.make_state_dict(backbone, C)
    for hd in (1, 2, 3):                                     # YOLONano.init_bias (models/yolo_nano.py:77-83)
        sd["head_det_%d.4.bias" % hd][:3] = bias_value
    h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, backbone, max_batch=B)
    h.load_state_dict(sd)
    h.train_bind()
    return h, sd


def _grad(h, key, shape):
    return h.flat_grads[h.param_slice(key)].cpu().numpy().reshape(shape)


def _param(h, key, shape):
    return h.flat_params[h.param_slice(key)].cpu().numpy().reshape(shape)


def _close(a, ref, rel, floor):
    atol = max(rel * float(np.abs(ref).max()), floor)
    np.testing.assert_allclose(a, ref, rtol=rel, atol=atol)


def _oracle64(sd, backbone, C, x, target, S, lr):
    """The fp64 oracle step: the round-off-free gradient.  At B=2 the stage-4 BatchNorms see 32 samples and the
    reference's own fp32 gradient is ~2e-2 (relative to max |g|) away from it, so fp32 paths are judged against THIS."""
    from oracle.torch_port import TrainNet
    net = TrainNet(sd, backbone, C, anchors=arch.MULTI_ANCHOR_SIZE, dtype=torch.float64)
    losses, grads = net.train_step(x, target, S, lr=lr)
    return losses, {k: v.numpy() for k, v in grads.items()}, net


def test_train_step_matches_reference_fixture(golden):
    g = golden("train.npz")
    S, C, B, lr = int(g["S"]), int(g["C"]), int(g["B"]), float(g["lr"])
    h, sd = _handle(S, C, B, float(g["init_bias_value"]))
    x0 = weights.make_input(B, S, seed=10)
    t = torch.as_tensor(g["target"]).cuda()
    losses = h.train_step(torch.as_tensor(x0).cuda(), t, lr=lr, momentum=0.9, weight_decay=5e-4)
    np.testing.assert_allclose(losses.cpu().numpy(), g["losses_0"], rtol=2e-4)
    _, g64, _ = _oracle64(sd, "1.0x", C, x0, g["target"], S, lr)
    names = [str(n) for n in g["param_names"]]
    l2 = np.array([float(np.sqrt((_grad(h, n, -1).astype(np.float64) ** 2).sum())) for n in names])
    np.testing.assert_allclose(l2, g["grad_sums_0"][:, 2], rtol=3e-2, atol=1e-4)      # the reference's fp32 round-off (see _oracle64)
    for k in g:
        name = k.split(":", 1)[-1]
        if k.startswith("grad_0:"):
            ref, exact = g[k].astype(np.float64), g64[name]
            scale = float(np.abs(exact).max())
            ref_err = float(np.abs(ref - exact).max())                                  # how far the reference itself is from exact
            got = _grad(h, name, ref.shape)
            if scale < 1e-9:                                                              # mathematically zero gradient: round-off only
                assert float(np.abs(got).max()) < 1e-3
                continue
            assert float(np.abs(got - exact).max()) <= 3 * ref_err + 1e-3 * scale, name # HIP vs exact: as close as the reference's fp32 run
            assert float(np.abs(got - ref).max()) <= 2 * ref_err + 1e-3 * scale, name   # HIP vs reference: within the reference's own error
        if k.startswith("param_0:"):
            exact = g64[name]
            bound = lr * (2 * float(np.abs(g[k.replace("param_0", "grad_0")].astype(np.float64) - exact).max()) + 1e-3 * float(np.abs(exact).max())) + 1e-6
            assert float(np.abs(_param(h, name, g[k].shape) - g[k]).max()) <= bound, name
        if k.startswith("rm_0:"):
            np.testing.assert_allclose(h.read_param(name + ".running_mean", g[k].shape), g[k], rtol=1e-4, atol=1e-6)
        if k.startswith("rv_0:"):
            np.testing.assert_allclose(h.read_param(name + ".running_var", g[k].shape), g[k], rtol=1e-4, atol=1e-6)
    # The fixture's SECOND step (momentum buffer in use, parameters already moved by lr * g with lr * |g| ~ 0.3 on weights of size
    # 0.1): fp32 round-off of step one is amplified, so the bar is DERIVED, per quantity, from how far two legitimate runs of the
    # same two steps lie apart - the fp32 oracle, the fp64 oracle and the reference's recorded run (three realisations of one
    # computation): HIP has to be within 3x the largest pairwise distance among those of the recorded value.
    from oracle.torch_port import TrainNet
    runs = {}
    for dt in (torch.float32, torch.float64):
        net = TrainNet(sd, "1.0x", C, anchors=arch.MULTI_ANCHOR_SIZE, dtype=dt)
        net.train_step(x0, g["target"], S, lr=lr)
        l1, g1 = net.train_step(weights.make_input(B, S, seed=11), g["target"], S, lr=lr)
        runs[dt] = (np.asarray(l1, np.float64), {n: float(np.sqrt((g1[n].double().numpy() ** 2).sum())) for n in names},
                    {k[7:]: g1[k[7:]].double().numpy() for k in g if k.startswith("grad_1:")})
    x1 = torch.as_tensor(weights.make_input(B, S, seed=11)).cuda()
    losses1 = h.train_step(x1, t, lr=lr, momentum=0.9, weight_decay=5e-4)
    assert torch.isfinite(losses1).all() and not torch.equal(losses1, losses)
    got1 = losses1.cpu().numpy().astype(np.float64)
    ref1 = g["losses_1"].astype(np.float64)
    l32, l64 = runs[torch.float32][0], runs[torch.float64][0]
    spread = np.maximum.reduce([np.abs(l32 - l64), np.abs(l32 - ref1), np.abs(l64 - ref1)])
    assert np.all(np.abs(got1 - ref1) <= 3 * spread + 1e-3 * np.abs(ref1)), (got1, ref1, spread)
    l2_1 = np.array([float(np.sqrt((_grad(h, n, -1).astype(np.float64) ** 2).sum())) for n in names])
    ref_l2 = g["grad_sums_1"][:, 2].astype(np.float64)
    n32 = np.array([runs[torch.float32][1][n] for n in names]); n64 = np.array([runs[torch.float64][1][n] for n in names])
    spread_g = np.maximum.reduce([np.abs(n32 - n64), np.abs(n32 - ref_l2), np.abs(n64 - ref_l2)])
    badn = [(names[i], l2_1[i], ref_l2[i], spread_g[i]) for i in range(len(names)) if abs(l2_1[i] - ref_l2[i]) > 3 * spread_g[i] + 1e-2 * ref_l2[i] + 1e-4]
    assert not badn, badn[:8]
    # ... and ELEMENT-WISE on the ten gradients the fixture records for this step (stem, stage 2-4, lateral, smooth, heads): every element
    # within 3x the largest pairwise max-abs distance among the three realisations of that tensor (+ 1e-3 of its scale) of the recorded value
    bade = []
    for k in g:
        if not k.startswith("grad_1:"):
            continue
        name = k[7:]
        ref = g[k].astype(np.float64)
        a32, a64 = runs[torch.float32][2][name], runs[torch.float64][2][name]
        spread_e = max(float(np.abs(a32 - a64).max()), float(np.abs(a32 - ref).max()), float(np.abs(a64 - ref).max()))
        err = float(np.abs(_grad(h, name, ref.shape).astype(np.float64) - ref).max())
        if err > 3 * spread_e + 1e-3 * float(np.abs(ref).max()):
            bade.append((name, err, spread_e, float(np.abs(ref).max())))
    assert not bade, bade
    h.close()


def _targets(S, C, B, seed=5):
    rs = np.random.RandomState(seed)
    N = arch.num_predictions(S)
    target = np.zeros((B, N, 11), np.float32)
    for b in range(B):                                        # a handful of positives / ignored anchors (tools.py:150-215 layout)
        idx = rs.choice(N, 6, replace=False)
        target[b, idx, 0] = 1.0
        target[b, idx, 1] = rs.randint(0, C, 6)
        target[b, idx, 2:4] = rs.uniform(0, 1, (6, 2))
        target[b, idx, 4:6] = rs.standard_normal((6, 2)) * 0.3
        target[b, idx, 6] = rs.uniform(1.0, 2.0, 6)
        c = rs.uniform(0.2, 0.8, (6, 2)); wh = rs.uniform(0.05, 0.4, (6, 2))
        target[b, idx, 7:9], target[b, idx, 9:11] = c - wh / 2, c + wh / 2
        ign = rs.choice(N, 4, replace=False)
        ign = ign[target[b, ign, 0] == 0]
        target[b, ign, 0] = -1.0
        target[b, ign, 6] = -1.0
    return target


@pytest.mark.parametrize("backbone,S,C,B", [("1.0x", 128, 20, 2), ("0.5x", 96, 80, 3), ("1.0x", 160, 80, 4), ("1.0x", 224, 20, 1),
                                            ("1.5x", 96, 20, 2), ("2.0x", 96, 20, 2)])
def test_train_step_every_gradient_vs_oracle(golden, backbone, S, C, B):
    """Every parameter gradient, the SGD update and the BN running statistics against the oracle step.
    The exact gradient is the fp64 oracle's; the fp32 oracle run of the same step measures how much fp32 round-off the
    train-mode network amplifies (1e-2 of max|g| in the backbone is typical): the HIP gradient has to be as close to exact
    as that, per parameter (x4, or half the worst fp32 error, or 2e-3 — whichever is largest)."""
    from oracle.torch_port import TrainNet
    g = golden("train.npz")
    h, sd = _handle(S, C, B, float(g["init_bias_value"]), backbone)
    target = _targets(S, C, B)
    x = weights.make_input(B, S, seed=21)
    ref_losses, g64, net = _oracle64(sd, backbone, C, x, target, S, 1e-3)
    _, g32 = TrainNet(sd, backbone, C, anchors=arch.MULTI_ANCHOR_SIZE).train_step(x, target, S, lr=1e-3)
    before = h.flat_params.clone()
    losses = h.train_step(torch.as_tensor(x).cuda(), torch.as_tensor(target).cuda(), lr=1e-3, momentum=0.9, weight_decay=5e-4, update=True)
    np.testing.assert_allclose(losses.cpu().numpy(), ref_losses, rtol=1e-4)
    gmax = max(float(np.abs(v).max()) for v in g64.values())
    live = [n for n, v in g64.items() if float(np.abs(v).max()) >= 1e-9 * gmax]
    rel = lambda a, exact: float(np.linalg.norm((a - exact).ravel()) / np.linalg.norm(exact.ravel()))   # L2: one flipped ReLU does not dominate
    e32 = {n: rel(g32[n].double().numpy(), g64[n]) for n in live}
    worst32 = max(e32.values())
    bad = []
    for name, exact in g64.items():
        got = _grad(h, name, exact.shape)
        if name not in e32:                                   # mathematically zero (per-channel shift in front of conv + BN): round-off only
            if float(np.abs(got).max()) > 1e-6 * gmax:
                bad.append((name, float(np.abs(got).max()), 0.0))
            continue
        err = rel(got.astype(np.float64), exact)
        if err > max(4 * e32[name], 0.5 * worst32, 2e-3):
            bad.append((name, err, e32[name]))
        # first SGD step: buf = g + wd*p ; p -= lr*buf  (torch.optim.SGD, train.py:167-171) on the gradient just produced
        sl = h.param_slice(name)
        p0 = before[sl].cpu().numpy().astype(np.float64)
        want = p0 - 1e-3 * (got.reshape(-1) + 5e-4 * p0)
        perr = float(np.abs(h.flat_params[sl].cpu().numpy() - want).max())
        if perr > 1e-6 * max(1.0, float(np.abs(want).max())):
            bad.append((name + " (param)", perr, 0.0))
    assert not bad, "mismatch (name, relative err, fp32 oracle err): %s" % bad[:12]
    for spec in arch.conv_specs(backbone, C, 3):
        if spec.bn is not None:
            for stat in (".running_mean", ".running_var"):
                ref = net.p[spec.bn + stat].numpy()
                np.testing.assert_allclose(h.read_param(spec.bn + stat, ref.shape), ref, rtol=1e-4, atol=1e-6, err_msg=spec.bn + stat)
    h.close()


def test_train_then_infer_uses_updated_parameters(golden):
    """After a step, yn_fold_bn folds the UPDATED parameters / running statistics (eval-mode forward changes)."""
    g = golden("train.npz")
    S, C, B = int(g["S"]), int(g["C"]), int(g["B"])
    h, sd = _handle(S, C, B, float(g["init_bias_value"]))
    x = torch.as_tensor(weights.make_input(B, S, seed=10)).cuda()
    h.fold_bn()
    before = torch.cat([o.flatten() for o in h.forward_raw(x)]).clone()
    h.train_step(x, torch.as_tensor(g["target"]).cuda(), lr=float(g["lr"]))
    h.fold_bn()
    after = torch.cat([o.flatten() for o in h.forward_raw(x)])
    assert torch.isfinite(after).all()
    assert (after - before).abs().max().item() > 1e-3
    h.close()


@pytest.mark.parametrize("optimizer", ["torch", "fused"])
def test_shim_runs_the_reference_training_loop(golden, optimizer):
    """train.py:219-231 verbatim on the shim: model(images, target=targets) -> four losses -> total.backward() ->
    optimizer.step() -> optimizer.zero_grad(); torch.optim.SGD and the fused yn_sgd_step optimiser give the reference's
    recorded parameters; the BN statistics come back through state_dict()."""
    import yolo_nano_amd
    g = golden("train.npz")
    S, C, B, lr = int(g["S"]), int(g["C"]), int(g["B"]), float(g["lr"])
    model = yolo_nano_amd.YOLONano("cuda", input_size=S, num_classes=C, trainable=True, anchor_size=arch.MULTI_ANCHOR_SIZE, backbone="1.0x")
    model.load_state_dict({k: torch.as_tensor(v) for k, v in weights.make_state_dict("1.0x", C).items()}, strict=False)
    model.init_bias()
    model = model.to("cuda").train()
    if optimizer == "torch":
        opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=0.9, weight_decay=5e-4)
    else:
        opt = yolo_nano_amd.SGD(model, lr=lr, momentum=0.9, weight_decay=5e-4)
    images = torch.as_tensor(weights.make_input(B, S, seed=10)).cuda()
    targets = torch.as_tensor(g["target"]).cuda()
    conf_loss, cls_loss, bbox_loss, iou_loss = model(images, target=targets)
    total_loss = conf_loss + cls_loss + bbox_loss + iou_loss
    assert not torch.isnan(total_loss)
    total_loss.backward()
    np.testing.assert_allclose([conf_loss.item(), cls_loss.item(), bbox_loss.item(), iou_loss.item()], g["losses_0"], rtol=2e-4)
    named = dict(model.named_parameters())
    for k in g:
        if k.startswith("grad_0:"):
            ref = g[k]
            got = named[k[7:]].grad.cpu().numpy()
            assert np.linalg.norm((got - ref).ravel()) <= 5e-2 * np.linalg.norm(ref.ravel()) + 1e-3, k   # the reference's own fp32 error, see _oracle64
    opt.step()
    opt.zero_grad()
    sd = model.state_dict()
    for k in g:
        name = k.split(":", 1)[-1]
        if k.startswith("param_0:"):
            ref_g = g[k.replace("param_0", "grad_0")]
            bound = lr * 5e-2 * float(np.abs(ref_g).max()) + 1e-5
            assert float(np.abs(sd[name].cpu().numpy() - g[k]).max()) <= bound, name
        if k.startswith("rm_0:"):
            np.testing.assert_allclose(sd[name + ".running_mean"].cpu().numpy(), g[k], rtol=1e-4, atol=1e-6)
        if k.startswith("rv_0:"):
            np.testing.assert_allclose(sd[name + ".running_var"].cpu().numpy(), g[k], rtol=1e-4, atol=1e-6)
    # a second iteration on the updated parameters, then inference with the trained weights (eval.py path)
    losses2 = model(images, target=targets)
    sum(losses2).backward()
    opt.step()
    opt.zero_grad()
    model.trainable = False
    model.eval()
    boxes, scores, cls = model(images)
    assert boxes.shape[1] == 4 and len(scores) == len(cls) == len(boxes) and np.isfinite(boxes).all()


def test_no_gradient_buffer_is_read_before_it_is_written(golden, monkeypatch):
    """The step never memsets the activation gradients: every buffer is fully written by its first producer.  With the
    whole gradient region NaN-filled first (YN_TRAIN_POISON), losses, gradients and the update must come out unchanged."""
    g = golden("train.npz")
    S, C, B = int(g["S"]), int(g["C"]), int(g["B"])
    x = torch.as_tensor(weights.make_input(B, S, seed=10)).cuda()
    t = torch.as_tensor(g["target"]).cuda()
    h, _ = _handle(S, C, B, float(g["init_bias_value"]))
    l0 = h.train_step(x, t, update=False).clone()
    g0 = h.flat_grads.clone()
    monkeypatch.setenv("YN_TRAIN_POISON", "1")
    l1 = h.train_step(x, t, update=False)
    assert torch.isfinite(h.flat_grads).all()
    np.testing.assert_allclose(l1.cpu().numpy(), l0.cpu().numpy(), rtol=1e-6)
    err = (h.flat_grads - g0).abs().max().item()
    assert err <= 1e-3 * g0.abs().max().item()              # atomics / slice order only
    h.close()


def test_full_size_directional_derivative():
    """BASELINE configs[2] shape (1.0x, 608x608, bs=32, COCO head) through a size-independent property: moving the
    parameters by -eps * g must lower the summed loss by eps * |g|^2 to first order (the whole backward pass checked against
    the forward pass at full size, no oracle involved)."""
    from yolo_nano_amd import capi
    S, C, B = 608, 80, 32
    sd = weights.make_state_dict("1.0x", C)
    h = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE_COCO, "1.0x", max_batch=B)
    h.load_state_dict(sd)
    h.train_bind()
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    x = torch.randn((B, 3, S, S), generator=gen, device="cuda")
    rs = np.random.RandomState(3)
    labels = []
    for _ in range(B):
        c = rs.uniform(0.25, 0.75, (8, 2)); wh = rs.uniform(0.05, 0.5, (8, 2))
        box = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32).astype(np.float64)
        labels.append(np.concatenate([box, rs.randint(0, C, (8, 1)).astype(np.float64)], 1).tolist())
    t = h.make_targets(labels, arch.MULTI_ANCHOR_SIZE_COCO)
    l0 = float(h.train_step(x, t, update=False).double().sum())
    g = h.flat_grads.clone()
    assert torch.isfinite(g).all()
    g2 = float((g.double() ** 2).sum())
    p0 = h.flat_params.clone()
    ratios = []
    for frac in (0.01, 0.02):                                   # target loss decrease, as a fraction of the loss
        eps = frac * l0 / g2
        h.flat_params.copy_(p0 - eps * g)
        l1 = float(h.train_step(x, t, update=False).double().sum())
        ratios.append((l0 - l1) / (eps * g2))
    h.flat_params.copy_(p0)
    assert all(0.8 < r < 1.1 for r in ratios), (l0, g2, ratios)     # second-order terms pull the ratio slightly below 1
    assert abs(ratios[0] - 1.0) <= abs(ratios[1] - 1.0) + 0.05       # and it tends to 1 as the step shrinks
    h.close()


def test_nan_skip_leaves_parameters_untouched(golden):
    """train.py:225-226 (`if torch.isnan(total_loss): continue`) on the device: a gradient bucket holding a NaN / Inf — what a NaN
    loss on ANY data-parallel rank turns the all-reduced bucket into — makes yn_sgd_step skip the update as a whole; the next
    clean step applies normally."""
    g = golden("train.npz")
    h, sd = _handle(128, 20, 2, float(g["init_bias_value"]))
    x = torch.as_tensor(weights.make_input(2, 128, seed=3)).cuda()
    t = torch.as_tensor(_targets(128, 20, 2)).cuda()
    h.train_step(x, t, lr=1e-3, update=False)
    p0, m0 = h.flat_params.clone(), h.flat_momentum.clone()
    good = h.flat_grads.clone()
    for poison in (float("nan"), float("inf")):
        h.flat_grads.copy_(good)
        h.flat_grads[12345] = poison
        h.sgd_step(h.flat_params, h.flat_grads, h.flat_momentum, 1e-3)
        assert torch.equal(h.flat_params, p0) and torch.equal(h.flat_momentum, m0)
    assert h.skipped_steps() == 2
    h.flat_grads.copy_(good)
    h.sgd_step(h.flat_params, h.flat_grads, h.flat_momentum, 1e-3)
    assert not torch.equal(h.flat_params, p0) and h.skipped_steps() == 2
    want = p0.double() - 1e-3 * (good.double() + 5e-4 * p0.double())
    assert float((h.flat_params.double() - want).abs().max()) < 1e-6
    # a NaN in the input makes the whole fused step a no-op on the parameters
    p1 = h.flat_params.clone()
    xb = x.clone(); xb[0, 0, 5, 5] = float("nan")
    h.train_step(xb, t, lr=1e-3, update=True)
    assert torch.equal(h.flat_params, p1) and h.skipped_steps() == 3
    h.close()


def _snapshot(h, sd):
    """The handle's CURRENT parameters and BatchNorm running statistics as a numpy state dict (keys / shapes of `sd`)."""
    cur = {}
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            cur[k] = np.asarray(v)
        elif k.endswith(("running_mean", "running_var")):
            cur[k] = h.read_param(k, v.shape)
        else:
            cur[k] = h.flat_params[h.param_slice(k)].cpu().numpy().reshape(v.shape).copy()
    return cur


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_set_grid_steps_without_updates_are_sharp(golden, precision, monkeypatch):
    """The SHARP half of the multi-scale evidence (the steps with real updates below can only be held to chaos-sized bars): the same handle
    walks 128 -> 192 -> 128 through set_grid() with update=False steps on the UNTOUCHED initial weights, and every parameter gradient at
    every size is held to a precision-sized bar.  One obstacle is real and measured (tools/diag_smooth3.py): in ANY fp32 realisation of a
    step - the HIP one and the torch fp32 oracle alike, independently of each other - some pre-activation sits within round-off of zero, its
    LeakyReLU / ReLU slope flips against the float64 run, and where that element carries one of the few large loss gradients of a small map
    the layer's own parameter gradients move by 1e-2 ... 2e-1 (smooth_3 at 4 x 4 x 4 positions: HIP 0.2 / oracle 3e-5 on one seed, HIP 5e-5 /
    oracle 2.4e-3 on the next).  A wrong kernel is wrong on EVERY input, a flip only on the input that has it: each size is therefore run on
    THREE seeds and a tensor passes on its best one - but every step is run TWICE and has to reproduce to the order of the atomic sums - f32: relative L2 error against the float64 gradient <= max(4x the fp32 oracle's best,
    2e-3); f16: <= 2x the fp16-storage emulation's error + 2e-2 on the same seed, median ratio < 1.25 on every seed; losses 1e-4 (f32) on
    every seed.  Returning to 128 must reproduce the first 128 step to the order of the atomic sums (1e-5 of max|g|), and - f16 - the step
    with the BatchNorm sums fused into the GEMM epilogues equals the step with separate reduction launches (YN_TRAIN_FUSE_STATS /
    YN_TRAIN_FUSE_SUMS = 0) to 5e-3 of max|g| (losses 1e-2) at both sizes."""
    from oracle.torch_port import TrainNet
    g = golden("train.npz")
    C, B = 20, 4
    h, sd = _handle(128, C, B, float(g["init_bias_value"]))
    h.train_precision(precision)
    rel = lambda a, e: float(np.linalg.norm((a - e).ravel()) / np.linalg.norm(e.ravel()))
    mk = lambda **kw: TrainNet(sd, "1.0x", C, anchors=arch.MULTI_ANCHOR_SIZE, **kw)
    first = None
    for phase, S in enumerate((128, 192, 128)):
        h.set_grid(S)
        best, best_y = {}, {}
        for si, (xs, ts) in enumerate(((60, 17), (61, 18), (62, 19))):
            x = weights.make_input(B, S, seed=xs)
            target = _targets(S, C, B, seed=ts)
            xd, td = torch.as_tensor(x).cuda(), torch.as_tensor(target).cuda()
            losses = h.train_step(xd, td, lr=1e-4, update=False).cpu().numpy()
            grads = h.flat_grads.clone()
            # the SAME step again on the same handle (advisor, round 4): an activation-sign flip is a property of the data and reproduces to the
            # order of the atomic sums; a race or an uninitialised read in one of the fused kernels does not - and must not be excused as a "flip"
            l_again = h.train_step(xd, td, lr=1e-4, update=False).cpu().numpy()
            np.testing.assert_allclose(l_again, losses, rtol=1e-5, err_msg="S=%d seed %d: the step does not reproduce" % (S, xs))
            assert float((h.flat_grads - grads).abs().max()) <= 1e-5 * float(grads.abs().max()), (S, xs)
            if phase == 0 and si == 0:
                first = (losses, grads)
            if phase == 2:                                         # back at the first size: the first step again, to atomic-sum order
                np.testing.assert_allclose(losses, first[0], rtol=1e-5)
                assert float((grads - first[1]).abs().max()) <= 1e-5 * float(first[1].abs().max())
                break
            l64, g64 = mk(dtype=torch.float64).train_step(x, target, S, lr=1e-4)
            g64 = {k: v.numpy() for k, v in g64.items()}
            gmax = max(float(np.abs(v).max()) for v in g64.values())
            live = [n for n, v in g64.items() if float(np.abs(v).max()) >= 1e-9 * gmax]
            errs = {n: rel(_grad(h, n, g64[n].shape).astype(np.float64), g64[n]) for n in live}
            if precision == "f32":
                _, gy = mk().train_step(x, target, S, lr=1e-4)
                ey = {n: rel(gy[n].double().numpy(), g64[n]) for n in live}
                np.testing.assert_allclose(losses, l64, rtol=1e-4)
                for n in live:
                    best.setdefault(n, []).append(errs[n]); best_y[n] = min(best_y.get(n, 1e9), ey[n])
            else:
                lq, gy = mk(dtype=torch.float64, fp16_storage=True).train_step(x, target, S, lr=1e-4)
                ey = {n: rel(gy[n].numpy(), g64[n]) for n in live}
                for a, e, q in zip(losses, l64, lq):
                    assert abs(a - e) <= 2.0 * abs(q - e) + 2e-2 * abs(e), (S, losses, l64, lq)
                assert np.median([errs[n] / max(ey[n], 1e-6) for n in live]) < 1.25, S
                for n in live:                                     # excess over the same seed's bar
                    best.setdefault(n, []).append(errs[n] - (2.0 * ey[n] + 2e-2))
                if si == 0:                                        # the fused BatchNorm statistics / backward sums against their separate reduction launches
                    monkeypatch.setenv("YN_TRAIN_FUSE_STATS", "0"); monkeypatch.setenv("YN_TRAIN_FUSE_SUMS", "0")
                    l_un = h.train_step(xd, td, lr=1e-4, update=False).cpu().numpy()
                    monkeypatch.delenv("YN_TRAIN_FUSE_STATS"); monkeypatch.delenv("YN_TRAIN_FUSE_SUMS")
                    # (not atomic noise only: the epilogue sums are fp32 partials of 128 rows, the reduction kernel's are double - the statistics
                    #  differ in the 7th digit, a stored fp16 value lands on its neighbour here and there, the conf loss hangs on the IoU of a few
                    #  positives, and the early layers' fp16 gradients are noise-dominated in every realisation (error 0.7-1.0 of the value, the
                    #  emulation's too): the two runs are NOT comparable element by element there.  The unfused step is held to the fused one's
                    #  yardstick instead - the fp64 step, against the emulation's distance from it - and to the fused step where fp16 is exact
                    #  enough to compare: the tensors the emulation gets within 5 %.)
                    np.testing.assert_allclose(l_un, losses, rtol=1e-2)
                    errs_un = {n: rel(_grad(h, n, g64[n].shape).astype(np.float64), g64[n]) for n in live}
                    assert np.median([errs_un[n] / max(ey[n], 1e-6) for n in live]) < 1.25, S
                    for n in live:
                        assert errs_un[n] <= 2.5 * ey[n] + 5e-2, (S, n, errs_un[n], ey[n])
                        if ey[n] < 5e-2:
                            a = _grad(h, n, g64[n].shape).astype(np.float64)
                            b = grads[h.param_slice(n)].cpu().numpy().reshape(g64[n].shape).astype(np.float64)
                            assert rel(a, b) <= 3.0 * ey[n] + 1e-2, (S, n, rel(a, b), ey[n])
        if phase == 2:
            continue
        # a tensor passes on its BEST seed.  (Round 5 tried "two of three": at 128 x 128 two of the three seeds each carry an activation-sign flip
        # that moves every gradient upstream of it - errors 1.2e-2, 6.6e-3 and 3.8e-5 on the three seeds for the same tensors, the fp32 oracle
        # at 2e-5 - so that rule fails a correct step.  What rules out a race or an uninitialised read instead: every step above ran TWICE and
        # reproduced to the order of the atomic sums, which a data-dependent flip does and a race does not.)
        second = {n: sorted(v)[0] for n, v in best.items()}
        if precision == "f32":
            bad = [(n, best[n], best_y[n]) for n in best if second[n] > max(4 * best_y[n], 2e-3)]
            assert not bad, "S=%d (name, errs over the seeds, fp32 oracle's best): %s" % (S, bad[:8])
        else:
            bad = [(n, best[n]) for n in best if second[n] > 0.0]
            assert not bad, "S=%d (name, excess over 2x emulation + 2e-2 per seed): %s" % (S, bad[:8])
    h.close()


def _multi_scale_run(g, precision, sizes, B, C=20, seed_shift=0):
    """The body of test_multi_scale_training_through_set_grid (also tools/soak_multiscale.py): -> list of per-step dicts with the worst
    per-tensor excess over the bar, the offending tensors and the two cosines."""
    from yolo_nano_amd import capi
    from oracle.torch_port import TrainNet
    h, sd = _handle(sizes[0], C, B, float(g["init_bias_value"]))
    h.train_precision(precision)
    rel = lambda a, e: float(np.linalg.norm((a - e).ravel()) / np.linalg.norm(e.ravel()))
    out, seen_N = [], []
    for phase, S in enumerate(sizes):
        h.set_grid(S)
        seen_N.append(h.N)
        assert h.N == arch.num_predictions(S)
        for it in range(2):
            x = weights.make_input(B, S, seed=40 + 2 * phase + it + seed_shift)
            target = _targets(S, C, B, seed=7 + 2 * phase + it + seed_shift)
            cur = _snapshot(h, sd)
            mk = lambda **kw: TrainNet(cur, "1.0x", C, anchors=arch.MULTI_ANCHOR_SIZE, **kw)
            l64, g64 = mk(dtype=torch.float64).train_step(x, target, S, lr=1e-4)
            g64 = {k: v.numpy() for k, v in g64.items()}
            lq = None
            if precision == "f32":
                _, gy = mk().train_step(x, target, S, lr=1e-4)
                gy = {k: v.double().numpy() for k, v in gy.items()}
            else:
                lq, gy = mk(dtype=torch.float64, fp16_storage=True).train_step(x, target, S, lr=1e-4)
                gy = {k: v.numpy() for k, v in gy.items()}
            if it == 0 and phase > 0:                           # set_grid against a handle that has never seen another size
                hf = capi.Handle(S, C, arch.MULTI_ANCHOR_SIZE, "1.0x", max_batch=B)
                hf.load_state_dict(cur); hf.train_bind(); hf.train_precision(precision)
                lf = hf.train_step(torch.as_tensor(x).cuda(), torch.as_tensor(target).cuda(), lr=1e-4, update=False).cpu().numpy()
                la = h.train_step(torch.as_tensor(x).cuda(), torch.as_tensor(target).cuda(), lr=1e-4, update=False).cpu().numpy()
                np.testing.assert_allclose(la, lf, rtol=1e-5)
                assert float((h.flat_grads - hf.flat_grads).abs().max()) <= 1e-5 * float(hf.flat_grads.abs().max())
                hf.close()
            before = h.flat_params.clone()
            # the step once WITHOUT its update: the updating step below has to reproduce these gradients to the order of the atomic sums - a tensor
            # over its bar that is excused on another data draw has then at least been the same wrong number twice (a flip), not a race
            h.train_step(torch.as_tensor(x).cuda(), torch.as_tensor(target).cuda(), lr=1e-4, update=False)
            g_dry = h.flat_grads.clone()
            losses = h.train_step(torch.as_tensor(x).cuda(), torch.as_tensor(target).cuda(), lr=1e-4, momentum=0.9, weight_decay=5e-4, update=True).cpu().numpy()
            assert float((h.flat_grads - g_dry).abs().max()) <= 1e-5 * float(g_dry.abs().max()), ("step does not reproduce", phase, it)
            assert np.isfinite(losses).all() and h.skipped_steps() == 0, (phase, it, losses)
            assert not torch.equal(h.flat_params, before)                        # the update was applied
            gmax = max(float(np.abs(v).max()) for v in g64.values())
            live = [n for n, v in g64.items() if float(np.abs(v).max()) >= 1e-9 * gmax]
            ey = {n: rel(gy[n], g64[n]) for n in live}
            errs = {}
            for n in live:
                got = _grad(h, n, g64[n].shape).astype(np.float64)
                assert np.isfinite(got).all(), n
                errs[n] = rel(got, g64[n])
            va = np.concatenate([_grad(h, n, g64[n].shape).astype(np.float64).ravel() for n in live])
            ve = np.concatenate([g64[n].ravel() for n in live])
            vy = np.concatenate([gy[n].ravel() for n in live])
            cos = lambda u, w: float(u @ w / (np.linalg.norm(u) * np.linalg.norm(w)))
            out.append({"phase": phase, "S": S, "it": it, "losses": losses, "l64": np.asarray(l64), "lq": None if lq is None else np.asarray(lq),
                        "errs": errs, "ey": ey, "cos": cos(va, ve), "cos_y": cos(vy, ve)})
    assert seen_N[0] == seen_N[2] != seen_N[1]
    # and the eval path after the size changes: fold the trained weights, infer at a third size
    h.set_grid(160)
    h.fold_bn()
    o = h.infer(torch.as_tensor(weights.make_input(2, 160, seed=1)).cuda())
    assert int(o[4].sum().item()) > 0
    h.close()
    return out


# per-tensor bar of the steps WITH updates: (multiple of the yardstick's own error, absolute floor)
MS_SIZES, MS_B = (256, 320, 256), 4
MS_BAR = {"f32": (8.0, 0.2), "f16": (3.0, 0.2)}


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_multi_scale_training_through_set_grid(golden, precision):
    """train.py:202-208: every 10 iterations the SAME model gets a new input size through set_grid() and keeps training.
    Two steps at 256, set_grid(320), two steps, set_grid(256) again, two steps - REAL updates in between; every step's losses and gradients
    are checked against the float64 oracle started from the handle's own current parameters and running statistics (each comparison stands
    alone), and the arena re-carving in both directions is exercised.  Sharp statements: at every size change a FRESH handle built at the new
    size from the same snapshot gives the same losses and gradients (1e-5 of max|g|: only the order of atomic sums differs; measured 2e-7),
    losses to 1e-4 (f32), and the update-free walk of test_set_grid_steps_without_updates_are_sharp.  Against the oracle the per-tensor bar
    can only be flip-sized (see that test's docstring: single activation-sign flips move a layer's gradients by up to 2e-1 in the HIP step
    and in the fp32 torch oracle alike).  Round 3 ran this walk at 128 / 192 with four images - 64 positions per BatchNorm channel at stride
    32 - with a 0.25 floor AND up to three tensors per step allowed outside it at up to 300 %.  Round 4 runs it at 256 / 320 (256 / 400
    positions: a flip weighs a quarter as much) and holds EVERY tensor to max(8x the fp32 oracle's own error, 0.2) (f32) / 3x the
    fp16-storage emulation's error + 0.2 (f16; the emulation itself sits at 0.3-0.55 on the backbone tensors) - NO exemptions - plus a
    cosine >= 0.98 between the whole flat gradient and the oracle's (f16: no more than 0.1 below the emulation's own).
    Soaks (tools/soak_multiscale.py; profiles/r04_soak_multiscale.txt): 20 + 20 runs in the middle of the round had every tensor inside these
    bars (worst 0.74 / 0.87 of them); a second soak on the round's final sources (20 f32 + 14 f16 runs) had ONE f32 run with one head conv of
    the 8 x 8 level at 0.44 (a flip in a 96-channel layer seeing 256 positions) and the suite itself one f16 run with one 96-element bias at
    0.339 against a bar of 0.333.  A flip is an event of ONE data draw; a wrong kernel is wrong on every draw.  So the rule is: the walk runs
    once; if any tensor is over its bar the walk runs a second time on other data (input and target seeds shifted) and NO tensor may be over its
    bar in both.  Losses and cosines are held on every walk that runs."""
    g = golden("train.npz")
    k_mul, k_abs = MS_BAR[precision]
    bar = (lambda y: max(k_mul * y, k_abs)) if precision == "f32" else (lambda y: k_mul * y + k_abs)

    def walk(shift):
        over = {}
        for st in _multi_scale_run(g, precision, MS_SIZES, MS_B, seed_shift=shift):
            tag = "phase %d (S=%d) step %d" % (st["phase"], st["S"], st["it"])
            if precision == "f32":
                np.testing.assert_allclose(st["losses"], st["l64"], rtol=1e-4, err_msg=tag)
            else:
                for a, e, q in zip(st["losses"], st["l64"], st["lq"]):
                    assert abs(a - e) <= 3.0 * abs(q - e) + 4e-2 * abs(e) + 2e-2, (tag, st["losses"], st["l64"], st["lq"])
            for n, e in st["errs"].items():
                if e > bar(st["ey"][n]):
                    over.setdefault(n, []).append((tag, e, st["ey"][n]))
            assert st["cos"] >= (0.98 if precision == "f32" else min(0.98, st["cos_y"] - 0.1)), (tag, st["cos"], st["cos_y"])
        return over

    first = walk(0)
    if first:
        assert len(first) <= 3, "more than three tensors over their bar in one walk: %s" % first
        second = walk(100)
        both = {n: (first[n], second[n]) for n in first if n in second}
        assert not both, "over the bar on two independent data draws (name: (step, err, yardstick) per walk): %s" % both


def test_allreduce_grads_over_rccl_without_torch_distributed(golden):
    """yn_allreduce_grads(h, ncclComm_t) — SURVEY 8(b) — on the hardware: a communicator built straight from librccl (no
    torch.distributed anywhere), world size 1 on the one-GPU box: the flat gradient bucket goes through ncclAllReduce on the handle's
    stream (sum over one rank = itself, bit for bit), ordered between the backward pass and yn_sgd_step; a null communicator and an
    unbound handle are errors."""
    import ctypes
    import os
    from yolo_nano_amd import capi
    g = golden("train.npz")
    cand = [os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so"), "librccl.so.1", "/opt/rocm/lib/librccl.so.1"]
    rccl = None
    for c in cand:
        try:
            rccl = ctypes.CDLL(c, mode=ctypes.RTLD_GLOBAL)
            break
        except OSError:
            continue
    assert rccl is not None, "no librccl found"

    class UID(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_char * 128)]
    uid, comm = UID(), ctypes.c_void_p()
    rccl.ncclGetUniqueId.argtypes = [ctypes.POINTER(UID)]
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UID, ctypes.c_int]
    rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
    torch.cuda.set_device(0)
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    h, sd = _handle(128, 20, 2, float(g["init_bias_value"]))
    try:
        x = torch.as_tensor(weights.make_input(2, 128, seed=3)).cuda()
        t = torch.as_tensor(_targets(128, 20, 2)).cuda()
        for prec in ("f32", "f16"):
            h.train_precision(prec)
            h.train_step(x, t, lr=1e-3, update=False)
            g0 = h.flat_grads.clone()
            p0 = h.flat_params.clone()
            h.allreduce_grads(comm)                                   # RCCL, on the handle's stream
            h.sgd_step(h.flat_params, h.flat_grads, h.flat_momentum, 1e-3, grad_scale=1.0, first_step=(prec == "f32"))
            h.synchronize()
            assert torch.equal(h.flat_grads, g0) and torch.isfinite(g0).all()
            assert not torch.equal(h.flat_params, p0)
        with pytest.raises(capi.YnError):
            h.allreduce_grads(0)
        h2 = capi.Handle(128, 20, arch.MULTI_ANCHOR_SIZE, "1.0x")
        with pytest.raises(capi.YnError):
            h2.allreduce_grads(comm)                                  # nothing bound
        h2.close()
    finally:
        h.close()
        rccl.ncclCommDestroy(comm)
