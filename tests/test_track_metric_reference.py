"""CPU: tests/track_metric_reference.py -- the float64 restatement of the tracking metric that the GPU tests
compare the kernels with -- pinned on hand-built scenes with the expected numbers written out."""
import math

import numpy as np

import track_metric_cases as H
import track_metric_reference as R

CNT = {n: i for i, n in enumerate(R.COUNTS)}
RK = R.recall_thresholds()


def _car(out):
    """The car slot (class 0 is the first tracked class)."""
    return out["counts"][0], out["dist_sum"][0], out["valid"][0], out["thresholds"][0]


def _summary(out):
    tracked, _ = R.default_config()
    names = [n for n, t in zip(R.CLASS_NAMES, tracked) if t]
    return R.summarize_reference(out, names, RK)


def test_perfect_track():
    out = H.run(H.PERFECT)
    counts, dist, valid, theta = _car(out)
    assert out["status"] == 0 and valid.tolist() == [1] * 41 and np.all(theta == 0.9)
    for p in range(41):
        c = counts[p]
        assert (c[CNT["matches"]], c[CNT["switches"]], c[CNT["fp"]], c[CNT["miss"]], c[CNT["frames"]], c[CNT["objects"]]) == \
               (6, 0, 0, 0, 6, 6)
        assert abs(dist[p] / 6 - H.OFFSET) < 1e-12
    s = _summary(out)
    lm = s["label_metrics"]
    assert lm["amota"]["car"] == 1.0 and abs(lm["amotp"]["car"] - H.OFFSET) < 1e-12 and lm["motar"]["car"] == 1.0
    assert lm["tp"]["car"] == 6 and lm["mt"]["car"] == 1 and lm["ml"]["car"] == 0 and lm["tid"]["car"] == 0.0
    # the other six classes have no ground truth: the worst values, NaN where the worst value is -1
    assert lm["amota"]["bus"] == 0.0 and lm["amotp"]["bus"] == 2.0 and math.isnan(lm["ids"]["bus"]) and lm["faf"]["bus"] == 500
    assert abs(s["amota"] - 1.0 / 7) < 1e-12 and s["tp"] == 6.0 and s["ids"] == 0.0


def test_reachable_thresholds_set_amota():
    """A second object that is never detected: P = 12, n = 6, so only r_k <= 0.5 is reached (18 of the 40)."""
    frames = [(o + [(2, 30.0, 0.0)], h) for o, h in H.PERFECT]
    out = H.run(frames)
    counts, dist, valid, theta = _car(out)
    assert valid[1:].sum() == 18 and np.all(np.isnan(theta[18:])) and np.all(theta[:18] == 0.9) and RK[17] <= 0.5 < RK[18]
    assert counts[1, CNT["miss"]] == 6 and counts[1, CNT["matches"]] == 6 and counts[20].tolist() == [0] * 12
    lm = _summary(out)["label_metrics"]
    assert abs(lm["amota"]["car"] - 18 / 40) < 1e-12          # motar 1 at the 18 reached thresholds: fn = (1 - recall) P, no fp / ids
    assert abs(lm["amotp"]["car"] - (18 * H.OFFSET + 22 * 2.0) / 40) < 1e-12
    assert lm["ml"]["car"] == 1 and lm["mt"]["car"] == 1 and lm["recall"]["car"] == 0.5


def test_id_swap_and_refound():
    counts = _car(H.run(H.ID_SWAP))[0]
    assert counts[0, CNT["switches"]] == 2 and counts[0, CNT["matches"]] == 10 and counts[1, CNT["switches"]] == 2
    out = H.run(H.MISSED_SAME_ID)
    c = _car(out)[0][0]
    assert (c[CNT["switches"]], c[CNT["matches"]], c[CNT["miss"]], c[CNT["frag"]], c[CNT["lgd"]], c[CNT["tid"]], c[CNT["inst"]]) == \
           (0, 4, 2, 1, 2, 0, 1)
    assert c[CNT["frames"]] == 6 and c[CNT["mt"]] == 0 and c[CNT["ml"]] == 0          # 4 / 6 tracked
    assert _summary(out)["label_metrics"]["lgd"]["car"] == 1.0                        # 2 frames of 0.5 s
    c = _car(H.run(H.MISSED_NEW_ID))[0][0]
    assert (c[CNT["switches"]], c[CNT["matches"]], c[CNT["miss"]], c[CNT["frag"]]) == (1, 3, 2, 1)


def test_assignment_and_reestablish_cases():
    out = H.run(H.REESTABLISH)
    assert out["events_type"].tolist() == [1, 1] and out["events_row"].tolist() == [0, 2]
    assert _car(out)[0][0, CNT["fp"]] == 1 and abs(_car(out)[1][0] - (0.3 + 1.5)) < 1e-12
    out = H.run(H.CARDINALITY)
    assert out["events_type"].tolist() == [1, 1] and out["events_row"].tolist() == [1, 0]
    assert abs(_car(out)[1][0] - 3.8) < 1e-12
    assert math.sqrt(H.BELOW_2 * H.BELOW_2) < 2.0
    out = H.run(H.AT_THRESHOLD)
    assert out["events_type"].tolist() == [0, 1] and out["events_row"].tolist() == [-1, 1]
    out = H.run(H.CLAIMED)
    assert out["events_type"].tolist() == [1, 1, 1, 0] and out["events_row"].tolist() == [0, 1, 2, -1]
    assert _car(out)[0][0, CNT["switches"]] == 0


def test_filters_and_empty_frames():
    frames = [([(1, 0.0, 0.0), (2, 60.0, 0.0), (3, 5.0, 0.0), (4, 7.0, 0.0), (5, 9.0, 0.0, 5)],
               [(1, 0.1, 0.0, 0.9), (2, 60.1, 0.0, 0.9), (0, 5.0, 0.0, 0.9), (6, 9.0, 0.0, 0.9, 5)]),
              ([], []),
              ([(1, 0.0, 0.0)], [(1, 0.1, 0.0, 0.7)])]
    out = H.run(frames, num_pts=[5, 5, 0, 5, 5, 5], keep=[1, 1, 1, 0, 1, 1])
    c = _car(out)[0][0]
    # object 2 and its detection are beyond 50 m, object 3 has no points, object 4 is filtered, class 5 is not tracked, id 0 is no track
    assert (c[CNT["frames"]], c[CNT["objects"]], c[CNT["matches"]], c[CNT["fp"]], c[CNT["miss"]]) == (2, 2, 2, 0, 0)
    assert out["events_type"].tolist() == [1, -1, -1, -1, -1, 1] and out["status"] == 0
    ts = out["track_score"]
    assert ts[0] == ts[4] == (0.9 + 0.7) / 2 and np.isnan(ts[[1, 2, 3]]).all()              # the track's mean score
    bad = H.build(frames)
    bad["rec"][0, 0] = np.nan
    pos = [bad.pop(k) for k in ("rec", "cls", "track_id", "row_start", "row_count", "gt_xyz", "gt_cls", "gt_instance",
                                "gt_num_pts", "gt_keep", "gt_off", "ego", "scene", "timestamp_us")]
    assert R.evaluate_reference(*pos, **bad)["status"] == R.ST_NONFINITE


def test_no_objects_and_no_match():
    out = H.run([([], [(1, 0.0, 0.0, 0.9)])])                                              # P = 0
    assert np.isnan(_car(out)[3]).all() and _car(out)[0][0, CNT["fp"]] == 1 and _car(out)[2][1:].sum() == 0
    out = H.run([([(1, 0.0, 0.0)], [(1, 9.0, 0.0, 0.9)])])                                 # no match at all
    assert np.isnan(_car(out)[3]).all() and _car(out)[0][0, CNT["miss"]] == 1
    lm = _summary(out)["label_metrics"]
    assert lm["amota"]["car"] == 0.0 and lm["amotp"]["car"] == 2.0 and math.isnan(lm["gt"]["car"]) and lm["tid"]["car"] == 20


def test_thresholds_against_numpy_interp():
    rng = np.random.default_rng(3)
    for n, P in ((1, 1), (4, 4), (7, 10), (13, 40), (40, 40), (5, 0), (0, 6)):
        s = np.sort(rng.uniform(0.1, 1.0, n))[::-1]
        got = R.interp_thresholds(s, P, RK)
        if n == 0 or P == 0:
            assert np.isnan(got).all()
            continue
        rec = np.arange(1, n + 1, dtype=np.float64) / np.float64(P)
        want = np.interp(RK, rec, s)
        want[RK > np.float64(n) / np.float64(P)] = np.nan
        assert np.array_equal(got, want, equal_nan=True), (n, P)
    s = np.array([0.9, 0.7, 0.5, 0.3])
    got = R.interp_thresholds(s, 4, np.array([0.1, 0.25, 0.5, 0.625, 1.0]))
    assert got.tolist() == [0.9, 0.9, 0.7, 0.7 + ((0.5 - 0.7) / (0.75 - 0.5)) * (0.625 - 0.5), 0.3]


def test_mt_ml_tid_by_hand():
    """Object 1: tracked 4 of 5 (mt), first tracked one frame late; object 2: tracked 0 of 5 (ml); object 3: 1 of 2."""
    frames = []
    for f in range(5):
        objs = [(1, 0.0, 0.0), (2, 20.0, 0.0)] + ([(3, 40.0, 0.0)] if f >= 3 else [])
        hyps = ([(1, 0.1, 0.0, 0.9)] if f >= 1 else []) + ([(3, 40.1, 0.0, 0.8)] if f == 4 else [])
        frames.append((objs, hyps))
    c = _car(H.run(frames))[0][0]
    assert (c[CNT["mt"]], c[CNT["ml"]], c[CNT["tid"]], c[CNT["lgd"]], c[CNT["inst"]], c[CNT["frag"]]) == (1, 1, 1 + 1, 1 + 1, 2, 0)


def test_assignment_against_brute_force():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n, m = rng.integers(1, 7, 2)
        D = rng.uniform(0.0, 4.0, (n, m))
        pairs = R.assign(D, 2.0)
        k, cost = R.brute_force_assign(D, 2.0)
        assert len(pairs) == k and abs(sum(D[i, j] for i, j in pairs) - cost) < 1e-12
        assert len({i for i, _ in pairs}) == len({j for _, j in pairs}) == k and all(D[i, j] < 2.0 for i, j in pairs)
