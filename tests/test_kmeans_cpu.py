"""Anchor k-means without a GPU: the exact-sum host restatement (tests/kmeans_oracle.py) against what the reference's kmeans_anchor.py
produced (tests/golden/kmeans.npz, written by tests/golden/gen_kmeans.py), the pure-python helpers of yolo_nano_amd.anchors, and the
C-ABI boundary of yn_kmeans_*.

Tolerance of oracle against reference: picks, groups and iteration counts are equal (the generator asserts that no decision hangs on
the last bits); once the groups agree a pass's centroids and loss depend on the groups alone, and the reference adds at most N
positive terms one after the other, each addition within 2^-53 relative of the running sum, so the difference is at most
N * 2^-53 relative, and it does not compound over passes.  The bound used is 4 * N * 2^-53."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_oracle as ko  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ["ln300", "ln5000", "int257", "same5", "four"]


def rel_tol(n):
    return 4.0 * n * 2.0 ** -53


def close(a, b, n):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= rel_tol(n) * np.abs(b)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("kmeans.npz")


def test_fixture_comes_from_the_reference(fx):
    assert "kmeans_anchor.py of the reference" in str(fx["source"])
    assert list(fx["names"]) == SETS
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kmeans.npz")) < 300 * 1024


@pytest.mark.parametrize("name", SETS)
def test_oracle_seeding_picks_what_the_reference_picked(fx, name):
    boxes, K = fx[name + "_boxes"], int(fx[name + "_k"])
    rng = np.random.RandomState(int(fx[name + "_seed"]))
    first, draws = ko.draws_from(rng, len(boxes), K)
    assert first == int(fx[name + "_first"]) and np.array_equal(draws, fx[name + "_draws"])
    cent, picked, _, _ = ko.init_centroids(boxes, K, first, draws)
    assert np.array_equal(picked, fx[name + "_picked"])
    assert np.array_equal(cent, fx[name + "_seeds"])


@pytest.mark.parametrize("name", SETS)
def test_oracle_passes_match_the_reference(fx, name):
    boxes = fx[name + "_boxes"]
    n = len(boxes)
    cent = fx[name + "_seeds"]
    for p in range(len(fx[name + "_losses"])):
        cent, group, counts, loss = ko.do_kmeans(boxes, cent)
        assert np.array_equal(group, fx[name + "_groups"][p]), "pass %d" % p
        assert np.array_equal(counts, np.bincount(group, minlength=len(cent)))
        assert close(cent, fx[name + "_cents"][p], n), "pass %d" % p
        assert close(loss, fx[name + "_losses"][p], n), "pass %d" % p


@pytest.mark.parametrize("name", SETS)
def test_oracle_loop_stops_where_the_reference_stopped(fx, name):
    boxes = fx[name + "_boxes"]
    cent, counts, loss, it = ko.run(boxes, fx[name + "_seeds"], 1e-6, 1000)
    assert it == int(fx[name + "_iterations"])
    assert close(cent, fx[name + "_final"], len(boxes)) and close(loss, fx[name + "_final_loss"], len(boxes))
    assert int(counts.sum()) == len(boxes)


def test_all_duplicate_boxes_give_the_shorter_list(fx):
    assert np.array_equal(fx["same5_seeds"], [[10, 20], [0, 0], [0, 0]])
    _, group, counts, loss = ko.do_kmeans(fx["same5_boxes"], fx["same5_seeds"])
    assert counts.tolist() == [5, 0, 0] and loss == 0.0 and not group.any()


def test_oracle_sum_is_round_to_even_on_a_tie():
    from fractions import Fraction
    for boxes, sums in ko.halfway_sets():
        for c in range(2):
            exact = sum(Fraction(float(v)) for v in boxes[:, c])
            lo, hi = np.nextafter(sums[c], 0.0), np.nextafter(sums[c], np.inf)
            assert abs(Fraction(float(sums[c])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
        cent, _, counts, _ = ko.do_kmeans(boxes, np.array([[2.0, 2.0]]))
        assert counts.tolist() == [len(boxes)]
        assert cent[0, 0] == sums[0] / len(boxes) and cent[0, 1] == sums[1] / len(boxes)
    small = ko.halfway_sets()[0][0]
    assert Fraction(float(small[0, 0])) + Fraction(float(small[1, 0])) == Fraction(2) + Fraction(1, 2 ** 52)       # exactly halfway
    assert ko.do_kmeans(small, np.array([[2.0, 2.0]]))[0][0].tolist() == [1.0, 1.0 + 2.0 ** -51]                   # down to even, up to even


def test_oracle_prefix_comparison_in_limbs_is_the_plain_integer_one():
    r = np.random.RandomState(0)
    v = r.randint(0, 1 << 53, size=3000, dtype=np.int64)
    v[::7] = 1 << 53
    total = int(sum(int(x) for x in v))
    for t in [0, 1, int(v[0]) - 1, int(v[0]), total // 3, total - 1, total, total + 5, 1 << 76]:
        assert np.array_equal(ko.prefix_exceeds(v, t), ko.prefix_exceeds_plain(v, t)), t


def test_dataset_boxes_restates_the_loader():
    from yolo_nano_amd import dataset_boxes
    ann = [np.array([[10, 20, 110, 70, 3], [0, 0, 0.5, 300, 1]], dtype=np.float64),     # the second is thinner than 1 pixel at 416
           np.zeros((0, 5)),
           np.array([[5, 5, 6, 7, 0]], dtype=np.float64)]
    sizes = [(500, 375), (640, 480), (100, 200)]
    got = dataset_boxes(ann, sizes, 416)
    want = []
    for a, (w, h) in zip(ann, sizes):                         # the reference's loop, box by box
        for xmin, ymin, xmax, ymax, _ in a:
            bw = (xmax - xmin) / max(w, h) * 416
            bh = (ymax - ymin) / max(w, h) * 416
            if bw < 1.0 or bh < 1.0:
                continue
            want.append([bw, bh])
    assert got.dtype == np.float64 and np.array_equal(got, np.array(want)) and len(want) == 2
    assert dataset_boxes([], [], 416).shape == (0, 2)
    with pytest.raises(ValueError):
        dataset_boxes(ann, sizes[:2], 416)


def test_as_anchor_table_sorts_by_area_and_rounds():
    from yolo_nano_amd import arch, as_anchor_table
    c = np.array([[100.456, 50.0], [10.005, 12.994], [30.0, 300.0], [3.14159, 2.71828]])
    t = as_anchor_table(c)
    assert t == [[round(3.14159, 2), round(2.71828, 2)], [round(10.005, 2), round(12.994, 2)], [round(100.456, 2), 50.0], [30.0, 300.0]]
    nine = as_anchor_table(np.array(arch.MULTI_ANCHOR_SIZE)[::-1])
    assert nine == sorted([list(map(float, r)) for r in arch.MULTI_ANCHOR_SIZE], key=lambda r: r[0] * r[1])
    assert len(nine) == 9 and all(isinstance(v, float) for r in nine for v in r)


@pytest.mark.parametrize("bad, count", [([[0.5, 3.0]], 1), ([[3.0, 65536.0]], 1), ([[float("nan"), 2.0], [2.0, float("inf")]], 2),
                                        ([[-1.0, 2.0]], 1)])
def test_out_of_domain_boxes_are_refused_with_their_number(bad, count):
    from yolo_nano_amd import anchors
    boxes = np.array([[2.0, 3.0]] * 4 + bad)
    with pytest.raises(ValueError, match=r"^%d of %d boxes" % (count, len(boxes))):
        anchors.check_boxes(boxes)
    with pytest.raises(ValueError):
        anchors.check_boxes(np.zeros((0, 2)))
    with pytest.raises(ValueError):
        anchors.check_boxes(np.ones((3, 3)))
    assert anchors.check_boxes([[1.0, 65535.999]]).shape == (1, 2)


def test_kmeans_symbols_in_header_table_and_library():
    from yolo_nano_amd import build, capi
    build.build()
    want = {"yn_kmeans_create", "yn_kmeans_destroy", "yn_kmeans_set_boxes", "yn_kmeans_seed", "yn_kmeans_set_centroids", "yn_kmeans_run",
            "yn_kmeans_pass", "yn_kmeans_assign"}
    header = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(yn_kmeans_[a-z0-9_]+)\s*\(", header))
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (yn_kmeans_[a-z0-9_]+)", exported))
    table = {k for k in capi.SIGNATURES if k.startswith("yn_kmeans_")}
    assert want <= declared and declared == exported == table
    src = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "kernels_kmeans.hip")).read()
    assert "getenv" not in src
    flags = dict(build.SOURCES)["kernels_kmeans.hip"]
    assert "-ffp-contract=off" in flags


def test_host_reads_once_per_batch_of_passes():
    """the structural requirement: inside the run loop the only host read is ONE read of the state record per batch, and the launch
    function neither allocates nor synchronises (the GPU suite checks the counts through yn_kmeans_stats)"""
    src = open(os.path.join(ROOT, "yolo-nano_amd", "csrc", "kernels_kmeans.hip")).read()
    body = src[src.index("int kmeans_run("):src.index("int kmeans_assign(")]
    loop = body[body.index("for ("):]
    assert loop.count("read_state(") == 1 and "Synchronize" not in loop and "hipMemcpy" not in loop
    launch = src[src.index("void launch_pass("):src.index("int read_state(")]
    assert "Malloc" not in launch and "Synchronize" not in launch


def test_package_does_not_import_the_oracle():
    text = open(os.path.join(ROOT, "yolo-nano_amd", "anchors.py")).read()
    assert "import kmeans_oracle" not in text and "from kmeans_oracle" not in text and "import tests" not in text and "from tests" not in text
