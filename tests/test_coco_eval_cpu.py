"""tests/coco_oracle.py (the host restatement of pycocotools' COCOeval for 'bbox') against cases worked by hand, one per rule, and
against the committed fixture tests/golden/coco_eval.npz.  pycocotools is not needed; where it is installed,
tests/golden/gen_coco_eval.py asserts the restatement against it."""
import numpy as np

import coco_oracle

EPS = np.spacing(1)
ONE = 1.0 / (1.0 + EPS)                                     # a lone true positive: just under 1


def _img(image_id, gts, dts):
    """gts rows x, y, w, h, area, category, iscrowd; dts rows x, y, w, h, score, category (results-list order)"""
    g = np.asarray(gts, dtype=np.float64).reshape(-1, 7)
    d = np.asarray(dts, dtype=np.float64).reshape(-1, 6)
    return {"id": image_id, "gt": g[:, :5], "gt_cat": g[:, 5].astype(int), "gt_crowd": g[:, 6].astype(int),
            "dt": d[:, :4], "dt_score": d[:, 4], "dt_cat": d[:, 5].astype(int)}


def test_default_parameters():
    p = coco_oracle.default_params()
    assert len(p["iouThrs"]) == 10 and len(p["recThrs"]) == 101 and p["maxDets"] == [1, 10, 100]
    assert p["areaRng"] == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
    assert p["iouThrs"][0] == 0.5 and p["recThrs"][0] == 0.0 and p["recThrs"][-1] == 1.0


def test_hand_case():
    """two ground truths, three detections that are [match, miss, match] by score at every threshold"""
    im = _img(1, [[0, 0, 10, 10, 100, 0, 0], [100, 100, 10, 10, 100, 0, 0]],
              [[0, 0, 10, 10, .9, 0], [50, 50, 10, 10, .8, 0], [100, 100, 10, 10, .7, 0]])
    stats, precision, recall, ev = coco_oracle.coco_eval([im], 1)
    e = ev[0][0][0]
    assert e["matched"].tolist() == [[True, False, True]] * 10 and not e["dt_ig"].any()
    first, second = 1.0 / (1.0 + EPS), 2.0 / (3.0 + EPS)
    assert first == 0.9999999999999998 and second == 0.6666666666666666
    want = np.array([first] * 51 + [second] * 50)
    for t in range(10):
        assert np.array_equal(precision[t, :, 0, 0, 2], want)
        assert np.array_equal(precision[t, :, 0, 1, 2], want)            # both boxes are small
        assert (precision[t, :, 0, 2, 2] == -1).all() and (precision[t, :, 0, 3, 2] == -1).all()
        assert np.array_equal(precision[t, :, 0, 0, 0], [first] * 51 + [0.0] * 50)   # maxDets 1: the first detection alone
    assert (recall[:, 0, 0, 2] == 1.0).all() and (recall[:, 0, 0, 0] == 0.5).all() and (recall[:, 0, 2, 2] == -1).all()
    assert abs(stats[0] - np.mean(want)) <= 1e-12 and abs(stats[0] - 0.8349834983498) < 1e-12
    assert np.all(np.abs(stats[1:4] - stats[0]) <= 1e-12) and stats[4] == -1 and stats[5] == -1   # the summation order moves the last bit
    assert stats[6] == 0.5 and stats[7] == 1.0 and stats[8] == 1.0 and stats[9] == 1.0 and stats[10] == -1


def test_perfect_detections():
    rng = np.random.default_rng(1)
    images = []
    sizes = [12, 50, 150]                                    # small, medium, large
    for i in range(9):
        gts, dts = [], []
        for k in range(4):                                   # one box per (image, category), so one detection per image recalls all
            w = h = sizes[(i + k) % 3]
            x, y = int(rng.integers(0, 400)), int(rng.integers(0, 400))
            gts.append([x, y, w, h, w * h, k, 0])
            dts.append([x, y, w, h, float(rng.uniform(0.1, 1.0)), k])
        images.append(_img(100 - i, gts, dts))
    stats = coco_oracle.coco_eval(images, 5)[0]              # category 4 is empty
    assert (stats > -1).all()
    assert np.all(np.abs(stats - 1.0) <= 1e-12)
    assert np.all(stats[6:] == 1.0)                          # recall is exact; precision is n / (n + eps), under 1 only for n = 1


def test_crowd_absorbs_detections():
    im = _img(1, [[0, 0, 100, 100, 5000, 0, 1], [200, 200, 20, 20, 400, 0, 0], [0, 0, 100, 100, 5000, 1, 1]],
              [[10, 10, 20, 20, .9, 0], [40, 40, 20, 20, .8, 0], [10, 10, 20, 20, .7, 0], [200, 200, 20, 20, .6, 0], [10, 10, 20, 20, .9, 1]])
    stats, precision, recall, ev = coco_oracle.coco_eval([im], 2)
    e = ev[0][0][0]
    assert e["gt_ig"].tolist() == [True, False]
    assert e["matched"].all() and e["match_gt"][0].tolist() == [0, 0, 0, 1]        # IoU with a crowd box = intersection / detection area = 1
    assert e["dt_ig"][0].tolist() == [True, True, True, False]
    assert (precision[:, :, 0, 0, 2] == ONE).all() and (recall[:, 0, 0, 2] == 1.0).all()
    assert (precision[:, :, 1, :, :] == -1).all() and (recall[:, 1] == -1).all()    # crowd only: no non-ignored ground truth


def test_area_ignore_uses_the_annotation_area():
    im = _img(1, [[0, 0, 40, 40, 900, 0, 0]], [[0, 0, 40, 40, .9, 0], [500, 500, 40, 40, .8, 0]])
    stats, precision, recall, ev = coco_oracle.coco_eval([im], 1)
    small, medium = ev[0][1][0], ev[0][2][0]
    assert small["gt_ig"].tolist() == [False] and medium["gt_ig"].tolist() == [True]   # area 900, though w * h = 1600
    assert small["dt_ig"][0].tolist() == [False, True]       # matched: takes the ground truth's flag; unmatched: w * h = 1600 is outside
    assert medium["dt_ig"][0].tolist() == [True, False]
    assert (precision[:, :, 0, 1, 2] == ONE).all() and (precision[:, :, 0, 0, 2] == ONE).all()
    assert (precision[:, :, 0, 2, 2] == -1).all() and (recall[:, 0, 2, 2] == -1).all()
    assert stats[3] == ONE and stats[4] == -1


def test_max_dets_cut():
    dts = [[1000 + 20 * j, 0, 10, 10, .9, 0] for j in range(100)] + [[0, 0, 10, 10, .5, 0]]
    im = _img(1, [[0, 0, 10, 10, 100, 0, 0]], dts)
    stats, precision, recall, ev = coco_oracle.coco_eval([im], 1)
    assert len(ev[0][0][0]["order"]) == 100 and ev[0][0][0]["order"] == list(range(100))
    assert (precision[:, :, 0, 0, :] == 0).all() and (recall[:, 0, 0, :] == 0).all()
    im2 = _img(1, [[0, 0, 10, 10, 100, 0, 0]], dts[1:])       # 100 in all: the match is the last one kept
    stats, precision, recall, ev = coco_oracle.coco_eval([im2], 1)
    assert (recall[:, 0, 0, 2] == 1).all() and (recall[:, 0, 0, 1] == 0).all()
    assert (precision[:, :, 0, 0, 2] == 1.0 / (99.0 + 1.0 + EPS)).all()


def test_tie_orders():
    # equal IoU (0.6) against two boxes: the later one wins, the next detection gets the earlier one
    im = _img(1, [[100, 100, 40, 40, 1600, 0, 0], [120, 100, 40, 40, 1600, 0, 0]],
              [[110, 100, 40, 40, .9, 0], [110, 100, 40, 40, .8, 0], [110, 100, 40, 40, .7, 0]])
    e = coco_oracle.coco_eval([im], 1)[3][0][0][0]
    assert e["match_gt"][0].tolist() == [1, 0, -1] and e["match_gt"][2].tolist() == [1, 0, -1] and e["match_gt"][3].tolist() == [-1] * 3
    # equal scores inside an image: results-list order
    gt = [[0, 0, 10, 10, 100, 0, 0]]
    hit, miss = [0, 0, 10, 10, .8, 0], [50, 50, 10, 10, .8, 0]
    p1 = coco_oracle.coco_eval([_img(1, gt, [hit, miss])], 1)[1]
    p2 = coco_oracle.coco_eval([_img(1, gt, [miss, hit])], 1)[1]
    assert (p1[:, :, 0, 0, 2] == ONE).all() and (p2[:, :, 0, 0, 2] == 1.0 / (2.0 + EPS)).all()
    # equal scores across images: ascending image id, not add order
    a = _img(7, gt, [miss])
    b = _img(3, gt, [hit])
    for images in ([a, b], [b, a]):
        p = coco_oracle.coco_eval(images, 1)[1]
        assert np.array_equal(p[0, :, 0, 0, 2], [ONE] * 51 + [0.0] * 50)


def test_empty_category_and_no_ground_truth():
    im = _img(1, [[0, 0, 10, 10, 100, 0, 0]], [[0, 0, 10, 10, .9, 0], [0, 0, 10, 10, .9, 2]])
    stats, precision, recall, ev = coco_oracle.coco_eval([im, _img(2, [], [])], 3)
    assert ev[1][0] == [None, None] and ev[0][0][1] is None
    assert (precision[:, :, 1] == -1).all() and (precision[:, :, 2] == -1).all() and (recall[:, 1:] == -1).all()
    assert stats[0] == ONE
    stats = coco_oracle.coco_eval([_img(1, [], [[0, 0, 10, 10, .9, 0]])], 1)[0]
    assert (stats == -1).all()


def _fixture_images(g):
    images = []
    for i in range(len(g["image_ids"])):
        s, e = g["offsets"][i], g["offsets"][i + 1]
        images.append(coco_oracle.image_from_arrays(g["image_ids"][i], g["gt"][g["gt_off"][i]:g["gt_off"][i + 1]],
                                                    (g["boxes"][s:e], g["scores"][s:e], g["classes"][s:e]), g["geoms"][i]))
    return images


def test_fixture(golden):
    g = golden("coco_eval.npz")
    assert str(g["source"]) in ("oracle", "pycocotools")
    images = _fixture_images(g)
    stats, precision, recall, ev = coco_oracle.coco_eval(images, 80)
    assert np.array_equal(precision, g["precision"]) and np.array_equal(recall, g["recall"]) and np.array_equal(stats, g["stats"])
    # what the fixture is there to cover
    ids = g["image_ids"].tolist()
    assert ids != sorted(ids) and len(set(ids)) == len(ids)
    gt = g["gt"]
    assert (gt[:, 6] == 1).any() and (gt[:, 4] != gt[:, 2] * gt[:, 3]).any()
    for lo, hi in coco_oracle.default_params()["areaRng"][1:]:
        assert ((gt[:, 4] >= lo) & (gt[:, 4] <= hi) & (gt[:, 6] == 0)).any()
    assert ((gt[:, 2] * gt[:, 3] > 1024) & (gt[:, 4] < 1024)).any()                  # w * h and the area in different ranges
    gcat, dcat = set(gt[:, 5].astype(int).tolist()), set(g["classes"].tolist())
    assert (dcat - gcat) and (gcat - dcat) and (set(range(80)) - gcat - dcat)
    n_gt, n_dt = np.diff(g["gt_off"]), np.diff(g["offsets"])
    assert ((n_gt == 0) & (n_dt > 0)).any() and ((n_gt > 0) & (n_dt == 0)).any() and ((n_gt == 0) & (n_dt == 0)).any()
    assert max(np.bincount(g["classes"][g["offsets"][i]:g["offsets"][i + 1]], minlength=80).max() for i in range(len(ids))) > 100
    assert len(np.unique(g["scores"])) < len(g["scores"]) // 4
    crowd_hits = sum(int((e["matched"][0] & e["dt_ig"][0]).sum()) for k in range(80) for e in ev[k][0] if e is not None)
    assert crowd_hits >= 4
    im2 = images[2]                                           # the two boxes of category 8 with IoU 0.6 each: the later one first
    e = coco_oracle.evaluate_img(im2["dt"][im2["dt_cat"] == 8], im2["dt_score"][im2["dt_cat"] == 8], im2["gt"][im2["gt_cat"] == 8],
                                 im2["gt_crowd"][im2["gt_cat"] == 8], [0, 1e10], [0.5], 100)
    assert sorted(e["match_gt"][0].tolist(), reverse=True)[:2] == [1, 0]
    assert -1 < stats[0] < 1 and (stats > -1).all()
