"""The tracker without a GPU: the C ABI carries the yn_track_* symbols, a bad configuration is refused with its reason, the restatement
(tests/track_oracle.py) behaves as a tracker should, its float32 filter stays close to the float64 one, and matching in rounds (what the
kernel does) equals taking the best pair one at a time (what the specification says)."""
import os
import re
import subprocess

import numpy as np
import pytest

import track_cases as cases
import track_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["yn_track_create", "yn_track_destroy", "yn_track_reset", "yn_track_state", "yn_track_status", "yn_track_update"]


def test_symbols_in_header_ctypes_table_and_library():
    from yolo_nano_amd import build, capi
    build.build()
    header = open(os.path.join(ROOT, "include", "yolonano_hip.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (yn_track_[a-z_]+)", exported))
    assert sorted(exported) == SYMBOLS
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in capi.SIGNATURES, s
    assert "yn_track_params" in header
    lib = capi.load_library()
    assert lib.yn_abi_version() == 2
    import yolo_nano_amd
    from yolo_nano_amd import track
    assert yolo_nano_amd.Tracker is track.Tracker
    assert ctypes_size(track.TrackParams) == 44
    for k, v in orc.DEFAULTS.items():                           # the package's defaults are the oracle's
        assert track.DEFAULTS[k] == v, k
    assert np.float32(track.DEFAULTS["w_pos"]) == np.float32(1) / np.float32(20)
    assert np.float32(track.DEFAULTS["w_vel"]) == np.float32(1) / np.float32(160)


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


@pytest.mark.parametrize("kw, reason", [
    (dict(track_high=float("nan")), "yn_track_create: track_high is not finite"),
    (dict(w_vel=float("inf")), "yn_track_create: w_vel is not finite"),
    (dict(track_low=0.6, track_high=0.5), "yn_track_create: track_low is above track_high"),
    (dict(iou_high=0.0), "yn_track_create: iou_high outside (0, 1]"),
    (dict(iou_low=1.5), "yn_track_create: iou_low outside (0, 1]"),
    (dict(iou_new=-0.25), "yn_track_create: iou_new outside (0, 1]"),
    (dict(max_lost=-1), "yn_track_create: max_lost is negative"),
    (dict(min_hits=0), "yn_track_create: min_hits is below 1"),
    (dict(streams=0), "yn_track_create: streams 0 outside 1..4096"),
    (dict(max_tracks=129), "yn_track_create: max_tracks 129 outside 1..128"),
    (dict(max_dets=0), "yn_track_create: max_dets 0 outside 1..128"),
])
def test_a_bad_configuration_is_refused_with_its_reason(kw, reason):
    """The checks of yn_track_create, made by the package before it asks for a device (tests/test_gpu_track.py holds the library to the
    same text)."""
    from yolo_nano_amd import capi, track
    kw = dict(kw)
    args = [kw.pop(k, d) for k, d in (("streams", 1), ("max_tracks", 128), ("max_dets", 128))]
    assert track.refusal(*args, track.make_params(**kw)) == reason
    with pytest.raises(capi.YnError) as e:
        track.Tracker(*args, **kw)
    assert str(e.value) == reason
    assert track.refusal(1, 128, 128, track.make_params()) is None
    assert track.refusal(1, 1, 1, track.make_params(iou_high=1.0, max_lost=0, min_hits=1, track_low=0.5, track_high=0.5)) is None
    with pytest.raises(TypeError):
        track.make_params(iou=0.5)


# ---- the oracle as a tracker -------------------------------------------------------------------------------------------------------

def run(frames, **kw):
    t = orc.Tracker(1, **kw)
    return t, [t.update([f]) for f in frames]


def test_two_objects_that_cross_keep_their_ids():
    frames = cases.crossing()
    t, outs = run(frames)
    for k, (rec, ids, off) in enumerate(outs[1:], 1):
        assert list(ids) == [1, 2], (k, ids)
        # id 1 is still the object that moves to the right, id 2 the one that moves to the left
        assert abs(0.5 * (rec[0, 0] + rec[0, 2]) - (40 + 6 * k)) < 3 and abs(0.5 * (rec[1, 0] + rec[1, 2]) - (220 - 6 * k)) < 3, k
    x0 = [0.5 * (r[0][0, 0] + r[0][0, 2]) for r in outs[1:]]
    x1 = [0.5 * (r[0][1, 0] + r[0][1, 2]) for r in outs[1:]]
    assert x0[0] < x1[0] and x0[-1] > x1[-1], "the case has no crossing"
    assert t.streams[0].next_id == 3


@pytest.mark.parametrize("extra, same", [(0, True), (1, False)])
def test_a_gap_of_max_lost_frames_gives_the_id_back_and_one_more_a_new_one(extra, same):
    max_lost = 6
    t, outs = run(cases.gap(3, max_lost + extra, 3), max_lost=max_lost)
    assert list(outs[2][1]) == [1]
    for k in range(3, 3 + max_lost + extra):
        assert len(outs[k][1]) == 0
    ids = [list(o[1]) for o in outs[3 + max_lost + extra:]]
    assert ids == ([[1], [1], [1]] if same else [[], [2], [2]]), ids


def test_a_tentative_track_that_misses_its_second_frame_never_appears():
    f = cases.frame(cases.box(100, 100, 40, 40))
    t, outs = run([f, cases.frame(), f, cases.frame(), f, f])
    assert [list(o[1]) for o in outs] == [[], [], [], [], [], [3]]
    assert t.counters["births"] == 3 and (t.streams[0].meta[:, 0] != orc.FREE).sum() == 1


def test_a_low_score_detection_keeps_a_confirmed_track_alive_but_starts_none():
    hi, lo = cases.frame(cases.box(100, 100, 40, 40, 0.9)), cases.frame(cases.box(100, 100, 40, 40, 0.3))
    t, outs = run([hi, hi] + [lo] * 40)
    assert all(list(o[1]) == [1] for o in outs[1:]), "stage B did not keep the track"
    assert outs[-1][0][0, 4] == np.float32(0.3)
    t, outs = run([lo] * 10)
    assert all(len(o[1]) == 0 for o in outs) and t.counters["births"] == 0 and t.streams[0].next_id == 1
    # between track_high and new_thresh: matched by an existing track, but no birth
    t, outs = run([cases.frame(cases.box(100, 100, 40, 40, 0.55))] * 5)
    assert t.counters["births"] == 0


def test_the_scripted_scene_does_what_its_description_says():
    frames, kw = cases.scripted_scene()
    t, outs = run(frames, **kw)
    ids = [list(o[1]) for o in outs]
    assert ids[0] == [] and ids[1] == [1, 2, 3, 4, 5]
    assert all(i[:2] == [1, 2] for i in ids[1:]), "A and B lost their ids in the crossing"
    assert 3 not in ids[9] and 3 in ids[11] and 3 in ids[29], "C did not come back"
    assert 4 not in ids[12] and all(4 not in i for i in ids[10:])
    assert all(5 in i for i in ids[1:]), "E died at a low score"
    born_f = [k for k, i in enumerate(ids) if 7 in i]
    assert born_f and born_f[0] == 21, ids                      # G took id 6 in frame 5 and never showed
    assert all(6 not in i for i in ids)
    slot_d = 3
    assert t.streams[0].meta[slot_d, 1] == 7, "F did not take the lowest free slot (D's)"


# ---- float32 against float64 -----------------------------------------------------------------------------------------------------------

def test_float32_filter_stays_within_a_derived_bound_of_float64():
    """One track followed for 200 steps by the oracle (float32) and by the same recursion in float64, fed the same float32 measurements.

    The bound.  Let x = (p, v, P00, P01, P11) be one coordinate's filter and f_t its exact one-step map (predict, then update with z_t).
    The float32 run computes x'_{t+1} = f_t(x'_t) + l_t, where l_t is the rounding committed inside the step: each of the at most 8
    operations on the path to a component rounds a quantity no larger than the sum m_i of the absolute values of the terms that enter
    it, so |l_t,i| <= 8 u m_i with u = 2^-24.  The measurement noise term (w_pos s)^2 uses the track's own w or h, so its relative
    perturbation is that of p_w, p_h, covered by the same count.  To first order the difference e_t = x'_t - x_t obeys
    e_{t+1} = J_t e_t + l_t with J_t the Jacobian of f_t, hence |e_T| <= sum_k |J_{T-1} ... J_{k+1}| |l_k|.  The test evaluates exactly
    this sum in float64 from the float64 run: J_t by central differences of the float64 step, m_i from its terms, and doubles it for the
    second-order remainder.  Nothing in the bound comes from the float32 run."""
    p = orc.params()
    rng = np.random.RandomState(7)
    T = 200
    wp, wv = float(p["w_pos"]), float(p["w_vel"])
    t = orc.Tracker(1, 4, 4, min_hits=1)
    # the truth moves at constant velocity and breathes; the measurements carry noise of about the size the filter assumes
    zs = []
    for k in range(T + 1):
        cx, cy, w, h = 200 + 3.0 * k, 150 - 1.5 * k, 60 + 10 * np.sin(k / 15.0), 90 + 8 * np.cos(k / 11.0)
        n = rng.normal(0, 1.5, size=4)
        zs.append(cases.frame(cases.box(cx + n[0], cy + n[1], w + n[2], h + n[3], 0.9, 0)))
    z64 = [orc.measurement(f)[0].astype(np.float64) for f in zs]          # the float32 measurement, widened: both runs see the same z

    def init64(z, s):
        return np.array([z, 0.0, (2.0 * wp * s) ** 2, 0.0, (10.0 * wv * s) ** 2])

    def step64(x, z, s):
        pp, v, P00, P01, P11 = x
        q, qv = wp * s, wv * s
        pp, P00, P01, P11 = pp + v, ((P00 + 2.0 * P01) + P11) + q * q, P01 + P11, P11 + qv * qv
        return pp, v, P00, P01, P11

    def upd64(x, z, s):
        pp, v, P00, P01, P11 = x
        q = wp * s
        S = P00 + q * q
        K0, K1 = P00 / S, P01 / S
        r = z - pp
        return np.array([pp + K0 * r, v + K1 * r, P00 - K0 * K0 * S, P01 - K0 * K1 * S, P11 - K1 * K1 * S])

    def full64(X, z):
        """X [4][5] -> X after predict and update; the scales are read from X before each half, as the rules say."""
        s = (X[2][0], X[3][0], X[2][0], X[3][0])
        Y = np.array([step64(X[k], z[k], s[k]) for k in range(4)])
        s = (Y[2][0], Y[3][0], Y[2][0], Y[3][0])
        return np.array([upd64(Y[k], z[k], s[k]) for k in range(4)])

    def magnitudes(X, z):
        """m: per component, the sum of the absolute values of the terms that enter it in one step."""
        s = (X[2][0], X[3][0], X[2][0], X[3][0])
        Y = np.array([step64(X[k], z[k], s[k]) for k in range(4)])
        m = np.zeros((4, 5))
        for k in range(4):
            pp, v, P00, P01, P11 = Y[k]
            q = wp * (Y[2][0] if k in (0, 2) else Y[3][0])
            S = P00 + q * q
            K0, K1 = P00 / S, P01 / S
            r = abs(z[k]) + abs(pp)
            m[k] = [abs(X[k][0]) + abs(X[k][1]) + K0 * r + abs(pp), abs(v) + abs(K1) * r, 2 * P00 + K0 * K0 * S, 2 * abs(P01) + abs(K0 * K1) * S,
                    2 * P11 + K1 * K1 * S]
        return m

    u = 2.0 ** -24
    X = np.array([init64(z64[0][k], z64[0][2 + k % 2]) for k in range(4)])
    t.update([zs[0]])
    bound = np.zeros(20)
    worst = 0.0
    for k in range(1, T + 1):
        # Jacobian of the whole 20-variable step by central differences, in float64
        x0 = X.reshape(-1)
        J = np.zeros((20, 20))
        for i in range(20):
            d = max(abs(x0[i]), 1e-3) * 1e-6
            a, b = x0.copy(), x0.copy()
            a[i] += d
            b[i] -= d
            J[:, i] = (full64(a.reshape(4, 5), z64[k]).reshape(-1) - full64(b.reshape(4, 5), z64[k]).reshape(-1)) / (2 * d)
        bound = np.abs(J) @ bound + 8 * u * magnitudes(X, z64[k]).reshape(-1)
        X = full64(X, z64[k])
        rec, ids, off = t.update([zs[k]])
        assert list(ids) == [1], k
        got = t.streams[0].filt[0, 2:].astype(np.float64)
        err = np.abs(got - X.reshape(-1))
        assert (err <= 2 * bound).all(), (k, err, 2 * bound)
        worst = max(worst, float((err / np.maximum(2 * bound, 1e-300)).max()))
    # the bound is not vacuous: positions stay within a few thousandths of a pixel over 200 steps
    assert (2 * bound.reshape(4, 5)[:, 0]).max() < 0.05, bound.reshape(4, 5)[:, 0]
    print("largest error / bound over 200 steps: %.3f; position bound %.2e px" % (worst, (2 * bound.reshape(4, 5)[:, 0]).max()))


# ---- matching in rounds ---------------------------------------------------------------------------------------------------------------

def test_matching_in_rounds_equals_the_sequential_greedy_matching():
    """400 random matrices up to 13 x 13 whose entries come from a handful of values (ties everywhere), with random open rows and
    columns, and a few 128 x 128 ones: the kernel's rounds and the specification's one-pair-at-a-time loop take the same pairs."""
    rng = np.random.RandomState(11)
    most = 0
    for k in range(404):
        T, D = (rng.randint(1, 14), rng.randint(1, 14)) if k < 400 else (128, 128)
        levels = rng.randint(2, 6) if k < 400 else 40
        iou = (rng.randint(-1, levels, size=(T, D)) / np.float32(levels)).astype(np.float32)
        rows, cols = rng.uniform(size=T) < 0.8, rng.uniform(size=D) < 0.8
        thr = np.float32(rng.choice([0.25, 0.5]))
        seq = orc.greedy_sequential(iou, rows, cols, thr)
        rnd, rounds = orc.greedy_rounds(iou, rows, cols, thr)
        assert sorted(seq) == sorted(rnd), k
        most = max(most, rounds)
        for r, c in seq:
            assert rows[r] and cols[c] and iou[r, c] >= thr
    # a chain: every pair is the best of its row only after the one before it has gone, so the rounds degenerate to one pair each
    n = 9
    iou = np.full((n, n), -1, np.float32)
    for i in range(n):
        iou[i, i] = 0.9 - 0.05 * i
        if i + 1 < n:
            iou[i + 1, i] = 0.9 - 0.05 * i - 0.02
    seq = orc.greedy_sequential(iou, np.ones(n, bool), np.ones(n, bool), np.float32(0.25))
    rnd, rounds = orc.greedy_rounds(iou, np.ones(n, bool), np.ones(n, bool), np.float32(0.25))
    assert sorted(seq) == sorted(rnd) == [(i, i) for i in range(n)] and rounds >= 1
