"""CPU: the host half of mosaic samples (yolo_nano_amd.augment.Mosaic) against the reference's own load_mosaic + ColorTransforms
(tests/golden/mosaic.npz, made by tests/golden/gen_mosaic.py), bit for bit, and the canvas composition of the numpy pixel oracle
(tests/mosaic_oracle.py) that the GPU tests hold the device to.

Every test in this module fails at the parent commit: `Mosaic` (or `use_mosaic` / `sample_item`) cannot be imported from the package;
test_fixture_covers_the_branches alone reads only the fixture."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mosaic_oracle as mo                                   # noqa: E402

FN = {0: "randint", 1: "uniform"}


class DrawLog(object):
    """np.random.randint / uniform and Python's random.uniform / random.sample, logged."""

    def __init__(self):
        self.rows, self.py_uniform, self.py_sample = [], [], []

    def __enter__(self):
        self._np = {k: getattr(np.random, k) for k in FN.values()}
        self._py = {k: getattr(random, k) for k in ("uniform", "sample")}
        for code, k in FN.items():
            setattr(np.random, k, self._wrap(code, self._np[k]))
        random.uniform = self._uniform
        random.sample = self._sample
        return self

    def __exit__(self, *exc):
        for k, f in self._np.items():
            setattr(np.random, k, f)
        for k, f in self._py.items():
            setattr(random, k, f)

    def _wrap(self, code, f):
        def g(*args):
            v = f(*args)
            a = list(args) + [np.nan] * (2 - len(args))
            self.rows.append((code, float(a[0]), float(a[1]), float(v)))
            return v
        return g

    def _uniform(self, a, b):
        v = self._py["uniform"](a, b)
        self.py_uniform.append((float(a), float(b), float(v)))
        return v

    def _sample(self, population, k):
        v = self._py["sample"](population, k)
        self.py_sample.append((len(population), k, list(v)))
        return v


def _cases(g):
    for i in range(len(g["m_size"])):
        t = [g["m_target"][g["m_target_off"][4 * i + k]:g["m_target_off"][4 * i + k + 1]] for k in range(4)]
        yield dict(i=i, size=int(g["m_size"][i]), index=int(g["m_index"][i]), py_seed=int(g["m_py_seed"][i]), np_seed=int(g["m_np_seed"][i]),
                   ids=[int(v) for v in g["m_ids"][i]], shapes=[tuple(int(v) for v in s) for s in g["m_shapes"][i]], targets=t,
                   uniform=g["m_uniform"][i], ext=g["m_ext"][i], rect_a=g["m_rect_a"][i], rect_b=g["m_rect_b"][i],
                   mosaic_tg=g["m_mosaic_tg"][g["m_mosaic_tg_off"][i]:g["m_mosaic_tg_off"][i + 1]],
                   draws=g["m_draws"][g["m_draws_off"][i]:g["m_draws_off"][i + 1]],
                   boxes=g["m_boxes"][g["m_out_off"][i]:g["m_out_off"][i + 1]], labels=g["m_labels"][g["m_out_off"][i]:g["m_out_off"][i + 1]],
                   py_probe=float(g["m_py_probe"][i]), np_probe=float(g["m_np_probe"][i]), canvas_id=int(g["m_canvas_id"][i]))


def _as_lists(targets):
    """What load_img_targets hands over: a list of [x1, y1, x2, y2, class] rows, possibly empty."""
    return [[list(r) for r in t] for t in targets]


def test_sampler_equals_the_reference_load_mosaic_and_color_pass(golden):
    from yolo_nano_amd import ColorTransforms, Mosaic, MosaicParams
    g = golden("mosaic.npz")
    n_ids = int(g["m_n_ids"])
    mean = tuple(float(v) for v in g["m_mean"])
    n = 0
    for c in _cases(g):
        s = c["size"]
        mz = Mosaic(s, ColorTransforms(s, mean=mean))
        targets = _as_lists(c["targets"])
        random.seed(c["py_seed"])
        np.random.seed(c["np_seed"])
        with DrawLog() as log:
            ids = mz.sample_ids(c["index"], n_ids)
            assert len(log.py_sample) == 1 and len(log.rows) == 0 and not log.py_uniform
            frames, (yc, xc), mosaic_tg = mz.compose(c["shapes"], targets)
            assert len(log.py_uniform) == 2 and len(log.py_sample) == 1 and len(log.rows) == 0       # load_mosaic draws from `random` only
        msg = "case %d (S %d)" % (c["i"], s)
        assert ids == c["ids"], msg
        np.testing.assert_array_equal(np.array(log.py_uniform), c["uniform"], err_msg=msg)          # arguments and values, yc first
        assert (yc, xc) == (int(c["uniform"][0, 2]), int(c["uniform"][1, 2])), msg
        assert [tuple(f[:2]) for f in frames] == c["shapes"], msg
        np.testing.assert_array_equal(frames[:, 2:4], c["ext"], err_msg=msg + ": resized extents")
        np.testing.assert_array_equal(frames[:, 4:8], c["rect_a"], err_msg=msg + ": canvas rectangles")
        np.testing.assert_array_equal(frames[:, 8:12], c["rect_b"], err_msg=msg + ": source rectangles")
        assert mosaic_tg.dtype == np.float64
        np.testing.assert_array_equal(mosaic_tg, c["mosaic_tg"], err_msg=msg + ": mosaic targets")
        # the whole sample from the same seeds: the draws of both generators, the boxes, the record
        random.seed(c["py_seed"])
        np.random.seed(c["np_seed"])
        with DrawLog() as log:
            assert mz.sample_ids(c["index"], n_ids) == c["ids"]
            rec, boxes, labels, scale, offset = mz.sample(c["shapes"], targets)
        assert random.uniform(0.0, 1.0) == c["py_probe"], msg + ": draws consumed from random"
        assert np.random.uniform(0.0, 1.0) == c["np_probe"], msg + ": draws consumed from np.random"
        np.testing.assert_array_equal(np.array(log.rows, np.float64).reshape(-1, 4), c["draws"], err_msg=msg + ": np.random draws")
        assert len(log.py_uniform) == 2 and len(log.py_sample) == 1
        np.testing.assert_array_equal(boxes, c["boxes"] * 1. + np.zeros([1, 4]), err_msg=msg + ": boxes")      # Resize, square: scale 1., offset 0
        np.testing.assert_array_equal(np.asarray(labels, np.float64), c["labels"], err_msg=msg + ": labels")
        assert scale == 1. and np.array_equal(offset, np.zeros([1, 4]))
        assert isinstance(rec, MosaicParams) and rec.geom.dtype == np.int32 and rec.geom.shape == (50,)
        assert rec.photo.dtype == np.float32 and rec.photo.shape == (7,)
        np.testing.assert_array_equal(rec.geom[:48].reshape(4, 12), frames)
        assert int(rec.geom[48]) == int(c["draws"][-1, 3]), msg + ": mirror"                     # RandomMirror draws last
        np.testing.assert_array_equal(rec.photo[4:], np.array([v * 255 for v in mean]).astype(np.float32))
        for t, t0 in zip(targets, _as_lists(c["targets"])):
            assert t == t0, msg + ": the caller's targets changed"
        n += 1
    assert n >= 100


def test_fixture_covers_the_branches(golden):
    g = golden("mosaic.npz")
    cases = list(_cases(g))
    assert {c["size"] for c in cases} >= {64, 416, 500, 608}
    assert {c["index"] for c in cases} >= {0, int(g["m_n_ids"]) - 1}
    unresized = area = up = down = clipped = empty = thin = 0
    for c in cases:
        for (h0, w0), (rw, rh), a, b in zip(c["shapes"], c["ext"], c["rect_a"], c["rect_b"]):
            unresized += (rw, rh) == (w0, h0)
            area += (2 * rw, 2 * rh) == (w0, h0)
            up += rw > w0
            down += rw < w0 and (2 * rw, 2 * rh) != (w0, h0)
            clipped += (b[2] - b[0], b[3] - b[1]) != (rw, rh)           # only part of the frame fits its quadrant
            thin += min(rw, rh) <= 2
        empty += all(len(t) == 0 for t in c["targets"])
    assert min(unresized, area, up, down, clipped, empty, thin) > 0
    assert {int(c["draws"][-1, 3]) for c in cases} == {0, 1}


def test_sample_ids_equals_the_list_form():
    from yolo_nano_amd import ColorTransforms, Mosaic
    mz = Mosaic(416, ColorTransforms(416))
    for n_ids in (4, 5, 23, 1000):
        ids = [("root", "%06d" % k) for k in range(n_ids)]
        for index in (0, n_ids // 2, n_ids - 1):
            for seed in range(25):
                random.seed(seed)
                ref = [ids[index]] + random.sample(ids[:index] + ids[index + 1:], 3)                 # data/voc.py:141-145
                ref_next = random.random()
                random.seed(seed)
                got = mz.sample_ids(index, n_ids)
                assert random.random() == ref_next
                assert [ids[j] for j in got] == ref and got[0] == index and index not in got[1:]


def test_center_argument_and_range():
    from yolo_nano_amd import ColorTransforms, Mosaic
    for s in (64, 416, 608, 65):
        mz = Mosaic(s, ColorTransforms(s))
        shapes, targets = [(375, 500)] * 4, [[], [], [], []]
        lo, hi = -((-s) // 2), 2 * s + (-s) // 2                       # random.uniform(-x, 2 * S + x), x = (-S) // 2
        for yc, xc in ((lo, lo), (hi, hi), (lo, hi)):
            frames, c, tg = mz.compose(shapes, targets, center=(yc, xc))
            assert c == (yc, xc)
            assert frames[0, 6] == xc and frames[0, 7] == yc and frames[3, 4] == xc and frames[3, 5] == yc
            np.testing.assert_array_equal(tg, np.zeros([1, 5]))            # no target at all
        random.seed(s)
        for _ in range(200):
            _, (yc, xc), _ = mz.compose(shapes, targets)
            assert lo <= yc <= hi and lo <= xc <= hi


def test_degenerate_frame_is_refused():
    from yolo_nano_amd import ColorTransforms, Mosaic
    mz = Mosaic(64, ColorTransforms(64))
    random.seed(0)
    np.random.seed(0)
    with pytest.raises(ValueError):
        mz.sample([(375, 500), (4, 300), (375, 500), (375, 500)], [[], [], [], []])                   # int(4 * 64 / 300) == 0
    with pytest.raises(ValueError):
        mz.sample([(375, 500), (375, 500), (375, 500), (700, 3)], [[], [], [], []])
    mz.sample([(375, 500), (64, 1), (375, 500), (375, 500)], [[], [], [], []])                        # r == 1: pasted as it is


def test_oracle_canvas_equals_the_reference_canvas(golden):
    from yolo_nano_amd import ColorTransforms, Mosaic
    g = golden("mosaic.npz")
    mean = tuple(float(v) for v in g["m_mean"])
    seen = 0
    for c in _cases(g):
        if c["canvas_id"] < 0:
            assert "canvas_%d" % c["i"] not in g
            continue
        s = c["size"]
        frames = [mo.frame(c["canvas_id"] + j, h0, w0) for j, (h0, w0) in zip(c["ids"], c["shapes"])]
        random.seed(c["py_seed"])
        np.random.seed(c["np_seed"])
        mz = Mosaic(s, ColorTransforms(s, mean=mean))
        mz.sample_ids(c["index"], int(g["m_n_ids"]))
        rec = mz.sample(c["shapes"], _as_lists(c["targets"]))[0]
        got = mo.canvas(frames, rec.geom, s, mean)
        assert got.dtype == np.float64 and got.shape == (2 * s, 2 * s, 3)
        ref = g["canvas_%d" % c["i"]]
        assert ref.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.float32), ref, err_msg="case %d (S %d)" % (c["i"], s))
        fill = np.array([v * 255 for v in mean])
        covered = np.zeros((2 * s, 2 * s), bool)
        for a in c["rect_a"]:
            covered[a[1]:a[3], a[0]:a[2]] = True
        assert (got[~covered] == fill).all() and (~covered).any()          # the fractional float64 fill, outside every rectangle
        seen += 1
    assert seen >= 15


def test_use_mosaic_draws_only_when_on():
    from yolo_nano_amd.augment import use_mosaic
    np.random.seed(3)
    state = np.random.get_state()[1].copy()
    assert use_mosaic(False) is False
    assert np.array_equal(np.random.get_state()[1], state)              # `self.mosaic and np.random.randint(2)`: short-circuit
    np.random.seed(3)
    ref = [int(np.random.randint(2)) for _ in range(32)]
    np.random.seed(3)
    assert [int(use_mosaic(True)) for _ in range(32)] == ref and set(ref) == {0, 1}


def test_sample_item_follows_pull_item():
    from yolo_nano_amd import AugParams, ColorTransforms, Mosaic, MosaicParams, TrainTransforms
    from yolo_nano_amd.augment import sample_item
    s, n_ids = 64, 9
    rs = np.random.RandomState(1)
    shapes = [(37, 53), (53, 37), (64, 48), (128, 128), (129, 95), (61, 200), (9, 4), (100, 64), (40, 40)]
    frames = [mo.frame(50 + j, *shapes[j]) for j in range(n_ids)]
    targets = [[[0.1, 0.2, 0.5, 0.6, float(j)]] if j % 3 else [] for j in range(n_ids)]
    tf, mz = TrainTransforms(s), Mosaic(s, ColorTransforms(s))
    kinds = set()
    for index in range(n_ids):
        random.seed(index)
        np.random.seed(100 + index)
        fr, rec, target = sample_item(index, n_ids, lambda j: (frames[j], targets[j]), tf, mz)
        random.seed(index)
        np.random.seed(100 + index)
        if np.random.randint(2):                                          # data/voc.py:216-220
            ids = mz.sample_ids(index, n_ids)
            r2, boxes, labels, _, _ = mz.sample([shapes[j] for j in ids], [targets[j] for j in ids])
            assert isinstance(rec, MosaicParams) and len(fr) == 4 and all(a is frames[j] for a, j in zip(fr, ids))
        else:                                                             # :224-231
            t = np.zeros([1, 5]) if not targets[index] else np.array(targets[index])
            r2, boxes, labels, _, _ = tf.sample(shapes[index], t[:, :4], t[:, 4])
            assert isinstance(rec, AugParams) and fr is frames[index]
        kinds.add(type(rec).__name__)
        np.testing.assert_array_equal(rec.geom, r2.geom)
        np.testing.assert_array_equal(rec.photo, r2.photo)
        np.testing.assert_array_equal(target, np.hstack((boxes, np.expand_dims(labels, axis=1))))
        np.random.seed(100 + index)                                        # mosaic off: no branch draw, the plain transform
        fr, rec, _ = sample_item(index, n_ids, lambda j: (frames[j], targets[j]), tf, None)
        np.random.seed(100 + index)
        t = np.zeros([1, 5]) if not targets[index] else np.array(targets[index])
        np.testing.assert_array_equal(rec.geom, tf.sample(shapes[index], t[:, :4], t[:, 4])[0].geom)
    assert kinds == {"AugParams", "MosaicParams"}


def test_mosaic_sampler_is_numpy_only():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, random, numpy as np; from yolo_nano_amd import ColorTransforms, Mosaic; random.seed(0); np.random.seed(0); "
            "m = Mosaic(416, ColorTransforms(416)); m.sample_ids(3, 10); "
            "m.sample([(375, 500)] * 4, [[[0.1, 0.1, 0.5, 0.5, 3.0]], [], [], []]); "
            "assert 'torch' not in sys.modules, 'the sampler imported torch'")
    subprocess.check_call([sys.executable, "-c", code], cwd=root)
