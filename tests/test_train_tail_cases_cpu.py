"""tests/train_tail_cases.py without a device: loss64 reproduces the reference's recorded losses and autograd gradients and agrees with
oracle/loss.py on every case; every loss case has the property it claims; the exact SGD data is exact in fp32; the tables hold what
tests/test_gpu_train_tail_ops.py says they reach."""
import numpy as np
import pytest
import torch

import train_tail_cases as tc
from oracle import loss as oloss
from yolo_nano_amd import arch

GRADS = ("g_conf", "g_cls", "g_t")


def test_loss64_reproduces_the_reference_fixture(golden):
    g = golden("loss.npz")
    S = int(g["S"])
    r = tc.loss64(g["pred_conf"][..., 0], g["pred_cls"], g["pred_txtytwth"], g["target"], S, arch.MULTI_ANCHOR_SIZE)
    np.testing.assert_allclose(r["losses"].numpy(), g["losses"], rtol=1e-4)
    np.testing.assert_allclose(r["g_conf"].numpy(), g["g_conf"][..., 0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(r["g_cls"].numpy(), g["g_cls"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(r["g_t"].numpy(), g["g_txtytwth"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("fp16_inputs", [False, True])
@pytest.mark.parametrize("cid", tc.LOSS_IDS)
def test_references_are_finite_and_agree_with_the_oracle(cid, fp16_inputs):
    """oracle/loss.py decodes and takes the IoU in float32: it may be as far from float64 as torch's float32 is (4 * e32 + 4 ulp)"""
    c = tc.loss_case(cid, fp16_inputs)
    for r in (c["ref64"], c["ref32"]):
        assert all(bool(torch.isfinite(r[k]).all()) for k in ("losses", "iou") + GRADS)
        assert all(bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0 for v in r["terms"])
    losses, iou, g_conf, g_cls, g_t = oloss.loss_and_grads(c["conf"], c["cls"], c["t"], c["target"], c["S"], c["anchors"])
    for name, got in zip(GRADS, (g_conf, g_cls, g_t)):
        ref64, ref32 = c["ref64"][name], c["ref32"][name].double()
        e32 = float((ref32 - ref64).abs().max())
        ulp = float(np.spacing(np.float32(float(ref64.abs().max()))))
        assert float((torch.from_numpy(got).double() - ref64).abs().max()) <= 4 * e32 + 4 * ulp, name
    bars = tc.loss_value_bar(c["ref64"], c["ref32"])
    for k in range(4):
        assert abs(float(losses[k]) - float(c["ref64"]["losses"][k])) <= bars[k] + 4 * float(np.spacing(np.float32(losses[k])))


def test_max_and_min_split_the_gradient_on_ties():
    for dtype in (torch.float32, torch.float64):
        a = torch.tensor([0.25, 0.5], dtype=dtype, requires_grad=True)
        b = torch.tensor([0.25, 0.75], dtype=dtype, requires_grad=True)
        (torch.max(a, b).sum() + 2 * torch.min(a, b).sum()).backward()
        assert a.grad.tolist() == [1.5, 2.0] and b.grad.tolist() == [1.5, 1.0]


def test_block_counts():
    for cid, S, C, B, *_ in tc.LOSS_CASES:
        if cid in tc.LOSS_BLOCKS:
            assert tc.loss_blocks(S, B) == tc.LOSS_BLOCKS[cid], cid
    assert tc.LOSS_BLOCKS == {"s32-b1-c1": 1, "s64-b3-c20": 3, "s64-b64-c20": 63, "s128-b66-c20": 260}
    assert arch.num_predictions(32) == 63 and 3 * arch.num_predictions(64) == 756 and 756 % 256 != 0        # one block, not a full last wave; a ragged last block
    assert 64 * arch.num_predictions(64) == 63 * 256 and 66 * arch.num_predictions(128) == 66528          # no ragged block; more than 256 partials
    assert tc.head_row(20) == (75, 80) and tc.head_row(80) == (255, 256) and tc.head_row(1) == (18, 24)
    N = arch.num_predictions(64)
    assert any(0 < (b * N) % 256 for b in (1, 2))            # image boundaries inside blocks
    c = tc.loss_case("s64-b2-c80")
    assert tc.to_heads(c["conf"], c["cls"], c["t"], 64)[0].shape[-1] == 255


def test_heads_layout_round_trip():
    c = tc.loss_case("s64-b3-c20")
    back = tc.from_heads(tc.to_heads(c["conf"], c["cls"], c["t"], c["S"]), c["C"])
    for a, b in zip(back, (c["conf"], c["cls"], c["t"])):
        assert torch.equal(a, torch.from_numpy(np.array(b)))


def test_ties_case():
    c = tc.loss_case("ties")
    slots = tc.tie_slots(c["target"], c["t"])
    assert 40 <= int(slots.sum()) <= 50
    b32 = tc.decode(c["t"], c["S"], c["anchors"], torch.float32)[torch.from_numpy(slots)]
    b64 = tc.decode(c["t"], c["S"], c["anchors"], torch.float64)[torch.from_numpy(slots)]
    assert torch.equal(b32.double(), b64) and torch.equal(b64 * 64, (b64 * 64).round())            # exact in both, k / 64
    gt = torch.from_numpy(c["target"][slots][:, 7:11]).double()
    assert torch.equal(gt * 64, (gt * 64).round())
    shared = (gt == b64).sum(-1)
    for k in tc.TIE_SHARED:
        assert int((shared == k).sum()) >= 5, "%d shared edges" % k
    moved = (gt - b64)[gt != b64] * 64
    assert bool((moved > 0).any()) and bool((moved < 0).any()) and float(moved.abs().max()) <= 3
    iou = c["ref64"]["iou"][torch.from_numpy(slots)]
    assert bool((iou[shared == 4] == 1.0).all()) and bool((iou[shared < 4] < 1.0).all()) and bool((iou > 0).all())
    assert bool((c["ref32"]["iou"][torch.from_numpy(slots)][shared == 4] == 1.0).all())
    # the tie weights matter: a reference that gave a tied edge the whole gradient would differ on these slots
    k = torch.from_numpy(slots)
    part = c["ref64"]["g_t"][k][(shared > 0) & (shared < 4)]
    assert float(part.abs().max()) > 1e-3


def test_ignored_box_case():
    for cid in ("ignored-box", "s64-b3-c20", "saturated"):
        c = tc.loss_case(cid)
        k = tc.groups(c["target"])["ign"] & (c["target"][..., 7:11] != 0).any(-1)
        assert int(k.sum()) >= 10
        k = torch.from_numpy(k)
        assert bool((c["ref64"]["iou"][k] > 0).all()), "an ignored slot's box does not overlap its prediction"
        assert bool((c["target"][k.numpy()][:, 6] == -1).all())
        r = c["ref64"]
        assert not r["g_conf"][k].any() and not r["g_cls"][k].any() and bool((r["g_t"][k].abs().sum(-1) > 0).all())


def test_miss_case():
    c = tc.loss_case("miss")
    k = torch.from_numpy(tc.miss_slots(c["target"], c["t"]))
    assert int(k.sum()) == 4 * c["B"]
    for r in (c["ref64"], c["ref32"]):
        assert not r["en"][k].any() and not r["iou"][k].any()
        assert bool((r["terms"][3][k] == 0.5 / c["B"]).all())                                # |d| == 1: the linear branch of SmoothL1
    # the IoU path carries no gradient there: g_t is the box regression's alone
    t = torch.from_numpy(np.array(c["t"])).double()[k]
    tg = torch.from_numpy(np.array(c["target"])).double()[k]
    w = tg[:, 6:7] / c["B"]
    want = torch.cat([(torch.sigmoid(t[:, :2]) - tg[:, 2:4]) * w, 2 * (t[:, 2:] - tg[:, 4:6]) * w], -1)
    assert float((c["ref64"]["g_t"][k] - want).abs().max()) < 1e-14


def test_none_and_dense_cases():
    c = tc.loss_case("none")
    assert not tc.groups(c["target"])["pos"].any() and float(c["ref64"]["losses"][1]) == 0.0 and float(c["ref64"]["losses"][2]) == 0.0
    c = tc.loss_case("none-one")
    pos = tc.groups(c["target"])["pos"]
    assert not pos[1].any() and pos[0].any() and pos[2].any()
    c = tc.loss_case("dense")
    assert tc.groups(c["target"])["pos"][1].all()
    c = tc.loss_case("s32-b1-c1")
    assert float(c["ref64"]["losses"][1]) == 0.0 and not c["ref64"]["g_cls"].any()


def test_saturated_case():
    c = tc.loss_case("saturated")
    assert set(np.unique(np.abs(c["conf"]))) == {20.0, 50.0, 100.0}
    pos, neg = tc.groups(c["target"])["pos"], tc.groups(c["target"])["neg"]
    sat = (np.abs(c["t"][..., :2]) == 60).any(-1)
    assert (sat & pos).any() and (sat & neg).any()
    assert float(np.abs(c["t"][..., 2:]).max()) <= 8.0 and float(np.abs(c["t"][..., 2:]).max()) > 7.0
    assert float(np.abs(c["cls"][pos]).max()) > 80.0
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(100.0)))           # expf(-v) overflows in a sigmoid written 1 / (1 + exp(-v))


def test_exact_sgd_data_is_exact_in_fp32():
    """the float64 run on absolute values (every sign taken the worse way): at step k, g / 2 + p / 16, the momentum and p - buf / 8 are multiples of
    2**(-7 k), so a step is exact while those magnitudes * 2**(7 k) stay below 2**24; and on random data of the table every intermediate is an
    fp32 number"""
    lr, mom, wd, gs = (tc.SGD_EXACT[k] for k in ("lr", "momentum", "weight_decay", "grad_scale"))
    assert (lr, mom, wd, gs) == (2.0 ** -3, 0.5, 2.0 ** -4, 0.5)
    for first in (False, True):
        p = buf = 3.0
        for step in range(3):
            d = 3.0 * gs + wd * p
            buf = d if first and step == 0 else mom * buf + d
            p = p + lr * buf
            assert max(p, buf, d) * 2.0 ** (7 * (step + 1)) < 2.0 ** 24, (first, step, p, buf, d)
        rs = np.random.RandomState(5)
        p, buf = (torch.from_numpy(rs.randint(-3, 4, 4096).astype(np.float64)) for _ in range(2))
        for step in range(3):
            g = torch.from_numpy(rs.randint(-3, 4, 4096).astype(np.float64))
            d = g * tc.SGD_EXACT["grad_scale"] + tc.SGD_EXACT["weight_decay"] * p
            p, buf = tc.sgd64(p, g, buf, first=first and step == 0, **tc.SGD_EXACT)
            for v in (d, p, buf, tc.SGD_EXACT["lr"] * buf):
                assert torch.equal(v.float().double(), v)


def test_sgd_scan_and_ema_tables():
    assert tc.SGD_LENGTHS == [0, 1, 2, 3, 4, 5, 7, 1023, 1025, 5003, 2097152 + 3075]
    assert sorted({n % 4 for n in tc.SGD_LENGTHS}) == [0, 1, 2, 3]
    assert [tc.sgd_trips(n) for n in tc.SGD_LENGTHS[-3:]] == [1, 1, 2] and tc.SGD_LENGTHS[-1] % 4 == 3
    assert tc.sgd_blocks(2097152) == tc.SGD_GRID_CAP and tc.sgd_trips(2097152) == 1
    for n in tc.SCAN_LENGTHS:
        pl = tc.scan_placements(n)
        assert pl["first"] == 0 and pl["last"] == n - 1 and pl["tail"] == n - n % 4 and n % 4 and all(0 <= v < n for v in pl.values())
        assert pl["late-stride"] // tc.scan_stride(n) >= 3     # the scan's fourth trip or later
    assert tc.scan_stride(600001) == 512 * 256                # the scan's grid is capped below the update's
    assert tc.EMA_LENGTHS == [1, 257, 524288 + 257] and tc.EMA_LENGTHS[-1] > 2048 * 256
    assert tc.EMA_DECAYS["zero"] == 0.0 and tc.EMA_DECAYS["late"] == 0.9999 and 0 < tc.EMA_DECAYS["ramp-first"] < 1e-3
    assert np.float32(tc.FLT_MAX) == np.finfo(np.float32).max and 3.0e38 < tc.FLT_MAX
    v, m = np.float32([1.5, -2.0]), np.float32([0.25, 4.0])
    assert np.array_equal(tc.ema32(v, m, 0.0), m) and tc.ema32(v, m, 0.5).tolist() == [0.875, 1.0]
