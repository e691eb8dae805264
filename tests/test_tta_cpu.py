"""Batched test-time augmentation without a GPU: the host restatement (tests/tta_oracle.py) against live torch and against what the
reference's TestTimeAugmentation recorded (tests/golden/tta.npz), and the C-ABI boundary of yn_tta_* / yn_resize_batch.

Relation of the pinned resize to F.interpolate(mode='bilinear', align_corners=False).  Both evaluate the same bilinear form over taps of
magnitude <= M; they differ in (1) the order and fusing of the value operations - each side rounds at most four times at magnitude
<= M, 2^-24 relative each: 8 * 2^-24 * M together - and (2) the source coordinate, which torch computes with two roundings where the
pinned form fuses: at most one ulp u = np.spacing(float32(S0)) of a coordinate < S0.  Bilinear interpolation is continuous and
piecewise linear with slope <= D (the largest difference between adjacent taps), so a coordinate that moves by u moves the value by at
most u * D, across a cell boundary (a flipped floor) included.  Hence per element |oracle - torch| <= 8 * 2^-24 * M + u * D."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_oracle as to  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(160, 128), (160, 192), (96, 224), (64, 100), (128, 64), (128, 32)]


@pytest.mark.parametrize("S0,s", SHAPES)
def test_oracle_resize_is_within_the_derived_bound_of_torch(S0, s):
    """Measured worst |oracle - torch| / bound (N(0,1) data, B = 2, torch 2.10 CPU): 160 -> 128 0.042, 160 -> 192 0.196,
    96 -> 224 0.178, 64 -> 100 0.129, 128 -> 64 0.027, 128 -> 32 0.010; the worst absolute difference is 4.8e-7 (160 -> 192)."""
    x = np.random.default_rng(1000 * S0 + s).standard_normal((2, 3, S0, S0)).astype(np.float32)
    mine = to.resize(x, s)
    ref = torch.nn.functional.interpolate(input=torch.from_numpy(x), size=(s, s), mode="bilinear", align_corners=False).numpy()
    (a, b, c, d), _ = to.taps(x, s)
    M = np.max(np.abs(np.stack([a, b, c, d])), axis=0).astype(np.float64)
    D = np.max(np.abs(np.stack([a.astype(np.float64) - b, c.astype(np.float64) - d, a.astype(np.float64) - c, b.astype(np.float64) - d])), axis=0)
    u = float(np.spacing(np.float32(S0)))
    bound = 8.0 * 2.0 ** -24 * M + u * D
    diff = np.abs(mine.astype(np.float64) - ref.astype(np.float64))
    ratio = float(np.max(diff / np.maximum(bound, 1e-300)))
    print("tta resize %d -> %d: worst |oracle - torch| %.3g, worst ratio to the bound %.3f" % (S0, s, float(diff.max()), ratio))
    assert np.all(diff <= bound), "worst ratio %.3f" % ratio


def test_oracle_resize_identity_and_exact_reductions():
    x = np.random.default_rng(7).standard_normal((2, 3, 128, 128)).astype(np.float32)
    x[0, 0, 0, 0] = -0.0
    same = to.resize(x, 128)
    assert same is not x and np.array_equal(same.view(np.uint32), x.view(np.uint32))          # s == S0: the bits, -0 included
    # 2:1: src = 2 d + 1/2, all four weights 1/2, and a multiplication by 1/2 is exact: the pinned form is the 2 x 2 mean with the
    # row sums first, ((a + b) + (c + d)) / 4, two roundings in all
    quarter = np.float32(0.25)
    want = ((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])) * quarter
    assert np.array_equal(to.resize(x, 64), want)


def test_oracle_flip_and_unmirror():
    r = np.arange(2 * 3 * 4 * 4, dtype=np.float32).reshape(2, 3, 4, 4)
    p = to.flip_pairs(r)
    assert p.shape == (4, 3, 4, 4)
    assert np.array_equal(p[0], r[0]) and np.array_equal(p[2], r[1])
    assert np.array_equal(p[1], torch.flip(torch.from_numpy(r[0]), [-1]).numpy()) and np.array_equal(p[3][..., 0], r[1][..., 3])
    b = np.array([[0.1, 0.2, 0.4, 0.9], [0.0, 0.5, 1.0, 0.75]], dtype=np.float32)
    m = to.unmirror(b)
    assert np.array_equal(m[:, 0], np.float32(1.0) - b[:, 2]) and np.array_equal(m[:, 2], np.float32(1.0) - b[:, 0])
    assert np.array_equal(m[:, 1::2], b[:, 1::2]) and np.array_equal(b[0], np.array([0.1, 0.2, 0.4, 0.9], dtype=np.float32))


def test_list_building_and_merge_reproduce_the_reference_fixture(golden):
    """tta.npz: six forwards the reference's TestTimeAugmentation made (three scales x flip) and its merged result."""
    g = golden("tta.npz")
    C = int(g["C"])
    per = [(g["f%d_boxes" % i], g["f%d_scores" % i], g["f%d_labels" % i]) for i in range(int(g["n_forwards"]))]
    bb, sc, lb, start = to.build_list(per)
    assert list(start) == list(np.cumsum([0] + [len(p[1]) for p in per[:-1]]))
    assert len(bb) == len(sc) == len(lb) == sum(len(p[1]) for p in per)
    ob, osc, ol, keep = orc.tta_merge([(bb, sc, lb)], C, 0.4)                 # one un-flipped "forward": the list as built
    np.testing.assert_array_equal(ob, g["boxes"])
    np.testing.assert_array_equal(osc, g["scores"])
    np.testing.assert_array_equal(ol, g["labels"])
    eb, es, el, ekeep = orc.tta_merge(per, C, 0.4)                            # the existing route un-mirrors by itself: the same rows
    np.testing.assert_array_equal(keep, ekeep)
    np.testing.assert_array_equal(ob, eb)


NEW_ENTRIES = ["yn_resize_batch", "yn_tta_create", "yn_tta_destroy", "yn_tta_infer", "yn_tta_result", "yn_tta_forwards"]


def test_header_and_ctypes_table_name_the_new_entries():
    from yolo_nano_amd import capi
    header = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(yn_[a-z0-9_]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared, "%s is not declared in include/yolonano_hip.h" % name
        assert name in capi.SIGNATURES, "%s is missing from capi.SIGNATURES" % name
    assert {k for k in capi.SIGNATURES if k.startswith("yn_tta_")} == {n for n in NEW_ENTRIES if n.startswith("yn_tta_")}
    assert "typedef struct yn_tta yn_tta;" in header
    # argument counts of the table against the header's declarations
    for name in NEW_ENTRIES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(capi.SIGNATURES[name][1]), name
    import yolo_nano_amd
    assert callable(yolo_nano_amd.resize_batch)
    assert callable(yolo_nano_amd.TestTimeAugmentation.batch) and callable(yolo_nano_amd.TestTimeAugmentation.records)
