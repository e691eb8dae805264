"""CPU checks of the VOC metric restatement that yn_eval runs on the device: the host oracle (tests/voc_oracle.py, stable tie rule)
equals the reference's own voc_eval on tests/golden/voc_eval.npz bit for bit, and numpy's pairwise summation order (the area AP's
np.sum, restated in kernels_eval.hip) is pinned against np.sum."""
import numpy as np
import pytest

import voc_oracle

C = 20


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("use07", [True, False])
def test_oracle_equals_reference_voc_eval(golden, use07):
    g = golden("voc_eval.npz")
    recs = voc_oracle.ingest(g["boxes"], g["scores"], g["classes"], g["offsets"], g["geoms"])
    aps, curves, npos = voc_oracle.voc_metric(recs, g["gt"], g["gt_off"], C, 0.5, use07)
    tag = "07" if use07 else "area"
    assert _same(aps, g["ap_" + tag])
    assert _same(np.mean(aps), g["map_" + tag])
    off = g["curve_off"]
    for c in range(C):
        if off[c + 1] == off[c]:
            assert curves[c] == (-1., -1.) and aps[c] == -1.
            continue
        assert _same(curves[c][0], g["rec_" + tag][off[c]:off[c + 1]])
        assert _same(curves[c][1], g["prec_" + tag][off[c]:off[c + 1]])
    # the workload covers what the issue asks of it
    assert aps[18] == -1. and npos[19] == 0 and (np.diff(g["gt_off"]) == 0).any()
    assert 0 < np.sum((aps > 0) & (aps < 1))


def test_fixture_scores_are_distinct_per_class(golden):
    g = golden("voc_eval.npz")
    recs = voc_oracle.ingest(g["boxes"], g["scores"], g["classes"], g["offsets"], g["geoms"])
    for c in range(C):
        k = recs[recs[:, 1] == c, 2]
        assert len(np.unique(k)) == len(k)


def test_pairwise_sum_restatement_equals_np_sum():
    rng = np.random.default_rng(7)
    lengths = list(range(0, 300)) + list(rng.integers(0, 5001, 2700)) + [8191, 8192, 8193, 16384 + 17]
    for n in lengths:
        kind = int(rng.integers(0, 3))
        a = rng.standard_normal(n) * (10.0 ** rng.integers(-8, 9, n)) if kind == 0 else rng.random(n) * rng.random(n)
        if kind == 2:
            a[rng.random(n) < 0.5] = 0.0
        assert np.float64(voc_oracle.numpy_sum(a)).tobytes() == np.sum(a).tobytes(), n


def test_eleven_point_thresholds():
    assert [float(t) for t in np.arange(0., 1.1, 0.1)] == [i * 0.1 for i in range(11)]
