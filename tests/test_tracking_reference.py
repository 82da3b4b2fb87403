"""CPU: tests/tracking_reference.py, the numpy restatement of the tracker, pinned on hand-built scenes; the host
grouping `ops.tracking.scene_frames`; and the generators of test_tracking_gpu.py held inside the kernel's caps."""
import numpy as np
import pytest

import tracking_reference as R

CAR, TRUCK, BARRIER, PED = 0, 1, 5, 8
TC, MD = R.default_config()


def _scene(frames, dts=None):
    """frames: a list of lists of (x, y, vx, vy, score, cls) -> the reference's arguments for one scene, 0.5 s apart."""
    rec, cls, start, count = [], [], [], []
    for f in frames:
        start.append(len(rec))
        count.append(len(f))
        for x, y, vx, vy, score, c in f:
            rec.append([x, y, 0.0, 1.0, 1.0, 1.0, 0.0, vx, vy, score])
            cls.append(c)
    n = len(frames)
    dt = np.array([0.0] + [0.5] * (n - 1)) if dts is None else np.asarray(dts, np.float64)
    return (np.array(rec, np.float64).reshape(-1, 10), np.array(cls, np.int32), np.array(start), np.array(count),
            np.arange(n), np.array([0, n]), dt)


def _run(frames, **kw):
    ids, hits, status = R.track_reference(*_scene(frames, kw.pop("dts", None)), TC, MD, **kw)
    assert status == 0
    return ids.tolist(), hits.tolist()


def test_straight_line_keeps_its_id():
    frames = [[(10.0 + 2.0 * 0.5 * k, 5.0 - 1.0 * 0.5 * k, 2.0, -1.0, 0.9, CAR)] for k in range(6)]
    ids, hits = _run(frames)
    assert ids == [1] * 6 and hits == [1, 2, 3, 4, 5, 6]


def test_crossing_objects_need_the_velocity():
    # two pedestrians 1.2 m apart swap places within one 0.5 s frame; max_dist for pedestrians is 1 m
    a = lambda k: (0.0 + 2.4 * 0.5 * k, 0.0, 2.4, 0.0, 0.9, PED)
    b = lambda k: (1.2 - 2.4 * 0.5 * k, 0.0, -2.4, 0.0, 0.8, PED)
    ids, hits = _run([[a(0), b(0)], [a(1), b(1)]])
    assert ids == [1, 2, 1, 2] and hits == [1, 1, 2, 2]
    still = lambda t: t[:2] + (0.0, 0.0) + t[4:]
    ids, _ = _run([[still(a(0)), still(b(0))], [still(a(1)), still(b(1))]])
    assert ids == [1, 2, 2, 1]                       # without the compensation each detection lands on the other's track


@pytest.mark.parametrize("max_age", [2, 3, 4])
def test_missing_object_gets_its_id_back_until_max_age(max_age):
    det = lambda k: [(1.0 * 0.5 * k, 0.0, 1.0, 0.0, 0.9, CAR)]
    for gap, same in ((max_age - 1, True), (max_age, False)):
        frames = [det(0), det(1)] + [[] for _ in range(gap)] + [det(2 + gap)]
        ids, hits = _run(frames, max_age=max_age)
        assert ids == ([1, 1, 1] if same else [1, 1, 2]), (gap, ids)
        assert hits == [1, 2, 1]                      # a rematch after a miss restarts at 1, as a new track does


def test_other_class_never_takes_a_track():
    ids, hits = _run([[(0.0, 0.0, 0.0, 0.0, 0.9, CAR)], [(0.0, 0.0, 0.0, 0.0, 0.9, TRUCK)], [(0.0, 0.0, 0.0, 0.0, 0.5, CAR)]])
    assert ids == [1, 2, 1] and hits == [1, 1, 1]


def test_max_dist_is_inclusive_to_the_last_bit():
    md = MD[CAR]                                      # 4 m; d2 = 4 * 4 exactly
    ids, _ = _run([[(0.0, 0.0, 0.0, 0.0, 0.9, CAR)], [(md, 0.0, 0.0, 0.0, 0.9, CAR)]])
    assert ids == [1, 1]
    ids, _ = _run([[(0.0, 0.0, 0.0, 0.0, 0.9, CAR)], [(np.nextafter(md, np.inf), 0.0, 0.0, 0.0, 0.9, CAR)]])
    assert ids == [1, 2]


def test_untracked_classes_and_low_scores_get_no_id():
    frames = [[(0.0, 0.0, 0.0, 0.0, 0.9, BARRIER), (1.0, 0.0, 0.0, 0.0, 0.1, CAR), (2.0, 0.0, 0.0, 0.0, 0.3, CAR),
               (3.0, 0.0, 0.0, 0.0, 0.9, 2), (4.0, 0.0, 0.0, 0.0, 0.9, -1), (5.0, 0.0, 0.0, 0.0, 0.9, 10)]]
    ids, hits = _run(frames, score_threshold=0.3)
    assert ids == [0, 0, 1, 0, 0, 0] and hits == [0, 0, 1, 0, 0, 0]


def test_ties_in_score_and_in_distance():
    # equal scores: the lower row is the first candidate and takes id 1
    ids, _ = _run([[(0.0, 0.0, 0.0, 0.0, 0.5, CAR), (9.0, 0.0, 0.0, 0.0, 0.5, CAR), (20.0, 0.0, 0.0, 0.0, 0.7, CAR)]])
    assert ids == [2, 3, 1]
    # one detection exactly between two tracks: the lower slot (the higher-scored track of the frame before) wins
    ids, _ = _run([[(-1.0, 0.0, 0.0, 0.0, 0.6, CAR), (1.0, 0.0, 0.0, 0.0, 0.8, CAR)], [(0.0, 0.0, 0.0, 0.0, 0.9, CAR)]])
    assert ids == [2, 1, 1]
    ids, _ = _run([[(-1.0, 0.0, 0.0, 0.0, 0.8, CAR), (1.0, 0.0, 0.0, 0.0, 0.6, CAR)], [(0.0, 0.0, 0.0, 0.0, 0.9, CAR)]])
    assert ids == [1, 2, 1]


def test_coast_uses_the_current_dt_and_nonfinite_rows_are_reported():
    # the track was seen 0.5 s after its predecessor, the next frame comes 1 s later: it coasts 3 m, not 1.5 m
    frames = [[(0.0, 0.0, 3.0, 0.0, 0.9, PED)], [(1.5, 0.0, 3.0, 0.0, 0.9, PED)], [(4.5, 0.0, 3.0, 0.0, 0.9, PED)]]
    ids, _ = _run(frames, dts=[0.0, 0.5, 1.0])
    assert ids == [1, 1, 1]
    args = _scene([[(0.0, 0.0, np.nan, 0.0, 0.9, CAR), (1.0, 0.0, 0.0, 0.0, 0.9, CAR), (2.0, 0.0, np.nan, 0.0, 0.9, BARRIER)]])
    ids, hits, status = R.track_reference(*args, TC, MD)
    assert status == R.ST_NONFINITE and ids.tolist() == [0, 1, 0]


def test_scene_frames_orders_shuffled_samples():
    from unidistill_amd.ops.tracking import scene_frames
    scene = [7, 3, 7, 3, 7, 3, 3]
    ts = [3_000_000, 500_000, 1_000_000, 2_500_000, 1_000_000, 500_000, 1_000_001]
    fs, off, dt = scene_frames(scene, ts)
    assert fs.tolist() == [1, 5, 6, 3, 2, 4, 0]      # duplicate timestamps by sample index
    assert off.tolist() == [0, 4, 7]
    assert dt.tolist() == [0.0, 0.0, 500_001 * 1e-6, 1_499_999 * 1e-6, 0.0, 0.0, 2_000_000 * 1e-6]
    rfs, roff, rdt = R.scene_frames_reference(scene, ts)
    assert rfs.tolist() == fs.tolist() and roff.tolist() == off.tolist() and rdt.tobytes() == dt.tobytes()
    rng = np.random.default_rng(5)
    scene, ts = rng.integers(0, 9, 200), rng.integers(0, 50, 200) * 500_000 + 1_533_000_000_000_000
    fs, off, dt = scene_frames(scene, ts)
    rfs, roff, rdt = R.scene_frames_reference(scene, ts)
    assert rfs.tolist() == fs.tolist() and roff.tolist() == off.tolist() and rdt.tobytes() == dt.tobytes()
    assert fs.dtype == off.dtype == np.int64 and dt.dtype == np.float64


def test_generators_stay_inside_the_caps():
    import test_tracking_gpu as G
    from unidistill_amd.ops import tracking as T
    seen = set()
    for name in G.CASES:
        d, (fs, off, dt), (ids, hits, status), max_age = G._case(name)
        assert status == 0 and (ids > 0).any()
        peak_c, peak_t = R.live_tracks_peak(d["rec"], d["cls"], d["row_start"], d["row_count"], fs, off, dt, TC, MD, max_age)
        assert d["row_count"].max() <= T.MAX_BOXES and peak_c <= T.MAX_BOXES and peak_t <= max_age * T.MAX_BOXES, name
        assert 1 <= max_age <= T.MAX_AGE
        seen.add(name)
        if name == "cap_1024":
            assert peak_c == T.MAX_BOXES
        if name == "live_over_1024":
            stats = {}
            R.track_reference(d["rec"], d["cls"], d["row_start"], d["row_count"], fs, off, dt, TC, MD, max_age, stats=stats)
            assert T.MAX_BOXES < stats["peak_live"] <= peak_t                  # the reference's own list, not the bound
            assert (hits > 1).sum() == 0 and ids.max() < (ids > 0).sum()       # ids come back across a frame
        if name.startswith("tied_scores"):
            ties = cross = 0
            for s, n in zip(d["row_start"], d["row_count"]):
                sc, cl = d["rec"][s:s + n, 9], d["cls"][s:s + n]
                keep = np.isin(cl, G.TRACKED)
                same = (sc[keep][:, None] == sc[keep][None, :]) & ~np.eye(int(keep.sum()), dtype=bool)
                ties += int(same.sum())
                cross += int((same & (cl[keep][:, None] != cl[keep][None, :])).sum())
            assert ties > 0 and cross > 0, name
    assert {"one", "empty_frames", "wave_65", "wide_300", "cap_1024", "live_over_1024", "many_scenes", "age_1", "age_8",
            "shuffled", "tied_scores_4", "tied_scores_16"} <= seen
