"""Anchor k-means on the device (yn_kmeans_*, yolo_nano_amd.anchors) against the exact-sum host restatement tests/kmeans_oracle.py, BIT FOR
BIT (centroids, loss, counts, groups, picks, iterations), and against the reference's own run (tests/golden/kmeans.npz) with the
tolerance of tests/test_kmeans_cpu.py: equal picks, groups and iteration counts, centroids and loss within 4 * N * 2^-53 relative."""
import math
import os
import random
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_oracle as ko  # noqa: E402

pytestmark = pytest.mark.gpu

SETS = ["ln300", "ln5000", "int257", "same5", "four"]
SMALL_N = [1, 63, 64, 65, 257, 300, 5000]
# The pass runs min(ceil(N / 1024), 256) workgroups of 1024 threads; copy-in and assign min(ceil(N / 256), 1024) of 256.
BIG_N = 200003                                   # 196 workgroups; with K = 32 their 196 * 162 slab words take two rounds of the fold
STRIDE_N = 600011                                # more than 256 * 1024: every grid-stride loop runs up to three times per thread


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def close(a, b, n):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= 4.0 * n * 2.0 ** -53 * np.abs(b)))


def lognormal(n, seed):
    r = np.random.RandomState(seed)
    return np.clip(np.exp(r.normal(4.0, 0.9, size=(n, 2))), 1.0, 416.0)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans.npz")


@pytest.fixture(scope="module")
def handle():
    from yolo_nano_amd import arch, capi
    return capi.Handle(32, 1, arch.MULTI_ANCHOR_SIZE, "1.0x")


def make(boxes, handle):
    from yolo_nano_amd import AnchorKMeans
    return AnchorKMeans(boxes, handle=handle)


def check_passes(km, boxes, cent, passes):
    """device step by step against the oracle, bit for bit; -> the oracle's trajectory"""
    trail = []
    for p in range(passes):
        groups = km.assign().cpu().numpy()
        new, group, counts, loss = ko.do_kmeans(boxes, cent)
        got_c, got_n, got_l = km.step()
        assert np.array_equal(groups, group), "pass %d groups" % p
        assert same(got_c, new) and same(got_l, loss) and np.array_equal(got_n, counts), "pass %d" % p
        trail.append((new, group, loss))
        cent = new
    return trail


@pytest.mark.parametrize("name", SETS)
def test_fixture_set_pass_by_pass(fx, handle, name):
    boxes, K = fx[name + "_boxes"], int(fx[name + "_k"])
    n = len(boxes)
    km = make(boxes, handle)
    cent = km.seed(K, rng=np.random.RandomState(int(fx[name + "_seed"])))
    want_c, want_p, _, _ = ko.init_centroids(boxes, K, int(fx[name + "_first"]), fx[name + "_draws"])
    assert np.array_equal(km.picked, want_p) and same(cent, want_c)
    assert np.array_equal(km.picked, fx[name + "_picked"]) and same(cent, fx[name + "_seeds"])
    trail = check_passes(km, boxes, cent, len(fx[name + "_losses"]))
    for p, (c, g, loss) in enumerate(trail):                            # and the reference itself
        assert np.array_equal(g, fx[name + "_groups"][p])
        assert close(c, fx[name + "_cents"][p], n) and close(loss, fx[name + "_losses"][p], n)
    km.close()


@pytest.mark.parametrize("name", SETS)
def test_fixture_set_full_loop(fx, handle, name):
    from yolo_nano_amd import anchor_box_kmeans
    boxes, K = fx[name + "_boxes"], int(fx[name + "_k"])
    n = len(boxes)
    cent, info = anchor_box_kmeans(boxes, K, rng=np.random.RandomState(int(fx[name + "_seed"])), handle=handle, return_info=True)
    want_c, want_n, want_l, want_it = ko.run(boxes, fx[name + "_seeds"], 1e-6, 1000)
    assert info["iterations"] == want_it == int(fx[name + "_iterations"])
    assert same(cent, want_c) and same(info["loss"], want_l) and np.array_equal(info["counts"], want_n)
    assert np.array_equal(info["picked"], fx[name + "_picked"])
    assert close(cent, fx[name + "_final"], n) and close(info["loss"], fx[name + "_final_loss"], n)
    # the same loop driven from the host, one yn_kmeans_pass at a time
    km = make(boxes, handle)
    km.set_centroids(fx[name + "_seeds"])
    c, cnt, old = km.step()
    it = 1
    while True:
        c, cnt, loss = km.step()
        it += 1
        if abs(old - loss) < 1e-6 or it > 1000:
            break
        old = loss
    assert it == want_it and same(c, cent) and same(loss, info["loss"]) and np.array_equal(cnt, info["counts"])
    km.close()


@pytest.fixture(scope="module")
def sized():
    """boxes per size, made once; the oracle's seeding and passes are cached per (N, K)"""
    return {n: lognormal(n, 100 + n) for n in SMALL_N + [BIG_N, STRIDE_N]}


@pytest.mark.parametrize("N, K", [(n, k) for n in SMALL_N for k in (1, 2, 9, 32)] + [(BIG_N, 9), (BIG_N, 32), (STRIDE_N, 9)])
def test_sizes_bit_for_bit(handle, sized, N, K):
    boxes = sized[N]
    if N >= BIG_N:                                # the exact column sum is not a double: the final rounding is exercised
        assert sum(Fraction(float(v)) for v in boxes[:4096, 0]) != Fraction(math.fsum(boxes[:4096, 0]))
    first, draws = ko.draws_from(np.random.RandomState(7 * N + K), N, K)
    km = make(boxes, handle)
    cent = km.seed_draws(K, first, draws)
    want_c, want_p, _, _ = ko.init_centroids(boxes, K, first, draws)
    assert np.array_equal(km.picked, want_p) and same(cent, want_c)
    if N < K:
        assert (km.picked[N:] == -1).all() and not cent[N:].any()
    check_passes(km, boxes, cent, 3)
    km.close()


def test_order_independence_and_repeatability(fx, handle):
    boxes, seeds = fx["ln5000_boxes"], fx["ln5000_seeds"]
    results = []
    r = np.random.RandomState(42)
    for order in [np.arange(len(boxes)), r.permutation(len(boxes)), r.permutation(len(boxes)), r.permutation(len(boxes)), np.arange(len(boxes))]:
        km = make(boxes[order], handle)
        km.set_centroids(seeds)
        first = km.step()
        km.set_centroids(seeds)
        results.append((first, km.run(1e-6, 1000)))
        km.close()
    (c0, n0, l0), (fc0, fn0, fl0, it0) = results[0]
    assert it0 == int(fx["ln5000_iterations"])
    for (c, n, l), (fc, fn, fl, it) in results[1:]:
        assert same(c, c0) and same(l, l0) and np.array_equal(n, n0)
        assert same(fc, fc0) and same(fl, fl0) and np.array_equal(fn, fn0) and it == it0


def test_run_reads_once_per_batch(fx, handle):
    km = make(fx["ln5000_boxes"], handle)
    km.set_centroids(fx["ln5000_seeds"])
    _, _, _, it = km.run(1e-6, 1000)
    passes, reads = km.stats()
    assert passes == it == int(fx["ln5000_iterations"]) and reads == -(-it // 32) and reads < it
    km.close()


def test_duplicate_centroids_and_empty_group(handle):
    boxes = lognormal(300, 9)
    cent = np.array([[40.0, 40.0], [40.0, 40.0], [120.0, 90.0], [0.0, 0.0]])
    km = make(boxes, handle)
    km.set_centroids(cent)
    trail = check_passes(km, boxes, cent, 3)
    new, group, _ = trail[0]
    assert not (group == 1).any() and not (group == 3).any()           # the tie went to the lower index; (0, 0) never wins
    for c, g, _ in trail:
        assert not c[1].any() and not c[3].any() and (g != 1).all() and (g != 3).all()   # an empty group stays (0, 0)
    km.close()


def test_iters_one_means_two_passes(fx, handle):
    boxes, seeds = fx["ln300_boxes"], fx["ln300_seeds"]
    km = make(boxes, handle)
    km.set_centroids(seeds)
    c, n, l, it = km.run(1e-6, 1)
    want = ko.run(boxes, seeds, 1e-6, 1)
    assert it == 2 == want[3] and same(c, want[0]) and same(l, want[2]) and np.array_equal(n, want[1])
    km.set_centroids(seeds)
    c, n, l, it = km.run(0.0, 5)                                        # loss_convergence = 0 never stops early: iters + 1 passes
    want = ko.run(boxes, seeds, 0.0, 5)
    assert it == 6 == want[3] and same(c, want[0]) and same(l, want[2])
    km.close()


def test_halfway_sums_round_to_even(handle):
    for boxes, sums in ko.halfway_sets():
        km = make(boxes, handle)
        km.set_centroids([[2.0, 2.0]])
        c, n, l = km.step()
        want = ko.do_kmeans(boxes, np.array([[2.0, 2.0]]))
        assert n.tolist() == [len(boxes)] and same(c, want[0]) and same(l, want[3])
        assert same(c[0], [sums[0] / len(boxes), sums[1] / len(boxes)])
        km.close()


def test_out_of_domain_boxes_are_refused_with_their_number(handle):
    from yolo_nano_amd import AnchorKMeans, capi
    good = lognormal(700, 4)
    bad = good.copy()
    bad[3, 0] = 0.5
    bad[650, 1] = float("nan")
    bad[699, 0] = 65536.0
    with pytest.raises(capi.YnError, match="3 of 700 boxes"):           # a device tensor: counted by yn_kmeans_set_boxes
        AnchorKMeans(torch.from_numpy(bad).cuda(), handle=handle)
    with pytest.raises(ValueError, match="3 of 700 boxes"):             # a host array: refused before anything is uploaded
        AnchorKMeans(bad, handle=handle)
    km = AnchorKMeans(torch.from_numpy(good).cuda(), handle=handle)     # and the device path accepts what is inside
    km.set_centroids([[50.0, 50.0]])
    assert km.step()[1].tolist() == [700]
    km.close()


def test_plain_sampling_branch(fx, handle):
    from yolo_nano_amd import anchor_box_kmeans
    boxes = fx["ln300_boxes"]
    idx = random.Random(5).sample(range(len(boxes)), 4)
    cent, info = anchor_box_kmeans(boxes, 4, plus=False, rng=random.Random(5), handle=handle, return_info=True)
    want = ko.run(boxes, boxes[idx], 1e-6, 1000)
    assert info["picked"].tolist() == idx and info["iterations"] == want[3] and same(cent, want[0]) and same(info["loss"], want[2])


def test_anchor_table_feeds_the_model(fx, handle):
    from yolo_nano_amd import YOLONano, anchor_box_kmeans, as_anchor_table
    table = as_anchor_table(anchor_box_kmeans(fx["ln300_boxes"], 9, rng=np.random.RandomState(3), handle=handle))
    areas = [w * h for w, h in table]
    assert len(table) == 9 and areas == sorted(areas)
    m = YOLONano(torch.device("cuda"), input_size=320, num_classes=20, anchor_size=table)
    assert m.num_anchors == 3
