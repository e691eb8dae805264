"""The two pieces every records route shares, on stub objects (no device): YOLONano's retry under exact f32 and capi.records_to_host."""
import warnings

import numpy as np
import pytest
import torch

from yolo_nano_amd.capi import YnRangeError, records_to_host
from yolo_nano_amd.model import YOLONano


class _Handle:
    def __init__(self):
        self.calls = []

    def range_status(self):
        self.calls.append("range_status")
        return False, True

    def exact_f32(self, on=True):
        self.calls.append(("exact_f32", on))


class _Model:
    _switch_to_exact = YOLONano._switch_to_exact
    _retry_exact = YOLONano._retry_exact

    def __init__(self, exact):
        self._exact_f32 = exact


def _call(fail_first):
    attempts = []

    def call():
        attempts.append(len(attempts))
        if len(attempts) <= fail_first:
            raise YnRangeError("yn_tta_infer: a forward split an activation >= 65504")
        return "attempt %d" % len(attempts)
    return call, attempts


def test_retry_switches_once_and_returns_the_second_attempt():
    m, h = _Model(False), _Handle()
    call, attempts = _call(1)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = m._retry_exact(h, call)
    assert got == "attempt 2" and len(attempts) == 2
    assert len(rec) == 1 and issubclass(rec[0].category, UserWarning) and "split-f16 range" in str(rec[0].message)
    assert h.calls.count("range_status") == 1 and h.calls.count(("exact_f32", True)) == 1 and len(h.calls) == 2
    assert m._exact_f32 is True


def test_retry_reraises_when_the_model_is_exact_already():
    m, h = _Model(True), _Handle()
    call, attempts = _call(1)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(YnRangeError):
            m._retry_exact(h, call)
    assert len(attempts) == 1 and not rec and not h.calls


def test_records_to_host():
    rng = np.random.default_rng(3)
    rows = rng.random((9, 6)).astype(np.float32)
    rows[:, 5] = [3, 0, 19, 7, 7, 1, 2, 2, 5]
    rec = torch.from_numpy(np.concatenate([rows, np.full((4, 6), np.nan, np.float32)]))      # rows past offsets[B] are not read
    offsets = torch.tensor([0, 4, 4, 9], dtype=torch.int32)                                     # image 1 is empty
    got = records_to_host(rec, offsets)
    assert len(got) == 3
    for b, (lo, hi) in enumerate(((0, 4), (4, 4), (4, 9))):
        bboxes, scores, cls = got[b]
        assert (bboxes.dtype, scores.dtype, cls.dtype) == (np.float32, np.float32, np.int64)
        assert bboxes.shape == (hi - lo, 4) and scores.shape == (hi - lo,) and cls.shape == (hi - lo,)
        assert np.array_equal(bboxes.view(np.uint32), rows[lo:hi, :4].view(np.uint32))
        assert np.array_equal(scores.view(np.uint32), rows[lo:hi, 4].copy().view(np.uint32))
        assert np.array_equal(cls, rows[lo:hi, 5].astype(np.int64))
        for a in (bboxes, scores, cls):
            assert a.flags.writeable and a.flags.owndata
            a[...] = 0                                           # fresh: writing one does not reach the others or the source
    assert np.array_equal(rec[:9].numpy(), rows)
