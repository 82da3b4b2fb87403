"""GPU: `ops.tracking.track_scenes` (csrc/track.hip) against tests/tracking_reference.py.  track_id and
track_hits are compared as integers with no tolerance: both sides do the same float64 operations in the same order with
contraction off, and d2 is compared without a square root, so any difference is a bug.  The cases are the smallest shapes that
cross each internal boundary of the kernel (a wave, the workgroup's width, the per-frame cap, one generation of tracks, the CU
count, both ends of max_age, a non-monotonic row_start)."""
import functools

import numpy as np
import pytest
import torch

import tracking_reference as R

TRACKED = [0, 1, 3, 4, 6, 7, 8]
TC, MD = R.default_config()

# name -> (make_scenes arguments, max_age)
CASES = {
    "one": (dict(seed=1, num_scenes=1, num_frames=1, num_objects=1, classes=[0]), 3),
    "empty_frames": (dict(seed=2, num_scenes=1, num_frames=7, num_objects=12, classes=TRACKED, empty_frames=(0, 3)), 3),
    "wave_65": (dict(seed=3, num_scenes=1, num_frames=2, num_objects=65, classes=[8], spread=12.0), 3),
    "wide_300": (dict(seed=4, num_scenes=2, num_frames=6, num_objects=300, classes=TRACKED, extra_classes=(2, 5, 9)), 3),
    "cap_1024": (dict(seed=5, num_scenes=1, num_frames=2, num_objects=1024, classes=TRACKED, spread=90.0), 3),
    "live_over_1024": (dict(seed=6, num_scenes=1, num_frames=5, num_objects=600, classes=TRACKED, alternate=True), 3),
    "many_scenes": (dict(seed=7, num_scenes=300, num_frames=2, num_objects=3, classes=TRACKED, spread=5.0), 3),
    "age_1": (dict(seed=8, num_scenes=2, num_frames=8, num_objects=40, classes=TRACKED, spread=25.0), 1),
    "age_8": (dict(seed=9, num_scenes=2, num_frames=12, num_objects=40, classes=TRACKED, spread=25.0), 8),
    "shuffled": (dict(seed=10, num_scenes=3, num_frames=6, num_objects=30, classes=TRACKED, spread=20.0,
                      shuffle_samples=True, extra_classes=(5,)), 3),
    # scores quantised to 4 / 16 values: equal scores within a class and across classes, ordered by row alone
    "tied_scores_4": (dict(seed=11, num_scenes=2, num_frames=6, num_objects=90, classes=TRACKED, spread=30.0, score_levels=4,
                          extra_classes=(5,)), 3),
    "tied_scores_16": (dict(seed=12, num_scenes=1, num_frames=5, num_objects=300, classes=TRACKED, score_levels=16), 3),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's arrays, its frame plan and the reference's answer, computed once and shared."""
    gen, max_age = CASES[name]
    d = R.make_scenes(**gen)
    fs, off, dt = R.scene_frames_reference(d["scene"], d["timestamp_us"])
    ids, hits, status = R.track_reference(d["rec"], d["cls"], d["row_start"], d["row_count"], fs, off, dt, TC, MD, max_age)
    for a in (ids, hits, fs, off, dt, *d.values()):
        a.setflags(write=False)
    return d, (fs, off, dt), (ids, hits, status), max_age


def _device_run(d, plan, max_age, out=None, **kw):
    from unidistill_amd.ops import tracking as T
    dev = torch.device("cuda", 0)
    rec = torch.from_numpy(np.array(d["rec"])).to(dev)
    cls = torch.from_numpy(np.array(d["cls"])).to(dev)
    ids, hits, status = T.track_scenes(rec, cls, d["row_start"], d["row_count"], *plan, track_class=TC, max_dist=MD,
                                       max_age=max_age, out=out, **kw)
    return ids.cpu().numpy(), hits.cpu().numpy(), int(status.item())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_matches_reference(name):
    from unidistill_amd.ops import tracking as T
    d, plan, (rid, rhits, rstatus), max_age = _case(name)
    fs, off, dt = T.scene_frames(d["scene"], d["timestamp_us"])
    assert all(np.array_equal(a, b) for a, b in zip((fs, off), plan[:2])) and dt.tobytes() == plan[2].tobytes()
    ids, hits, status = _device_run(d, (fs, off, dt), max_age)
    print(name, "rows", len(rid), "tracked", int((rid > 0).sum()), "ids", int(rid.max(initial=0)), "id mismatches",
          int((ids != rid).sum()), "hits mismatches", int((hits != rhits).sum()))
    assert status == rstatus == 0
    assert np.array_equal(ids, rid) and np.array_equal(hits, rhits)
    assert (rid > 0).any()


def _hand_scene(frames):
    """frames: lists of (x, y, vx, vy, score, cls) -> (d, plan) of one scene with frames 0.5 s apart."""
    rows = [r for f in frames for r in f]
    rec = np.array([[x, y, 0.0, 1.0, 1.0, 1.0, 0.0, vx, vy, s] for x, y, vx, vy, s, _ in rows], np.float64).reshape(-1, 10)
    count = np.array([len(f) for f in frames], np.int64)
    d = {"rec": rec, "cls": np.array([r[5] for r in rows], np.int32), "row_start": np.cumsum(count) - count, "row_count": count}
    n = len(frames)
    return d, (np.arange(n, dtype=np.int64), np.array([0, n], np.int64), np.array([0.0] + [0.5] * (n - 1)))


@pytest.mark.gpu
def test_ties_in_score_and_in_distance_on_the_device():
    """The tie rules on hand-built scenes, with the expected ids written out and the reference agreeing: equal scores order by
    row whatever the classes (a pedestrian in row 0 before a car in row 1), and a detection exactly between two tracks of its
    class takes the lower slot, in the newest generation and across generations."""
    CAR, PED = 0, 8
    cases = [
        # equal scores across classes and within one: candidate order is row order, so ids count up with the rows
        ([[(0.0, 0.0, 0.0, 0.0, 0.5, PED), (9.0, 0.0, 0.0, 0.0, 0.5, CAR), (20.0, 0.0, 0.0, 0.0, 0.5, PED),
           (30.0, 0.0, 0.0, 0.0, 0.5, CAR), (40.0, 0.0, 0.0, 0.0, 0.75, CAR)]], [2, 3, 4, 5, 1]),
        # equidistant (d2 = 1 = 1 exactly): the lower slot is the higher-scored track of the frame before
        ([[(-1.0, 0.0, 0.0, 0.0, 0.6, CAR), (1.0, 0.0, 0.0, 0.0, 0.8, CAR)], [(0.0, 0.0, 0.0, 0.0, 0.9, CAR)]], [2, 1, 1]),
        ([[(-1.0, 0.0, 0.0, 0.0, 0.8, CAR), (1.0, 0.0, 0.0, 0.0, 0.6, CAR)], [(0.0, 0.0, 0.0, 0.0, 0.9, CAR)]], [1, 2, 1]),
        # equal scores decide the slots (row order), then the equidistant detection takes the lower row's track
        ([[(1.0, 0.0, 0.0, 0.0, 0.5, CAR), (5.0, 5.0, 0.0, 0.0, 0.5, PED), (-1.0, 0.0, 0.0, 0.0, 0.5, CAR)],
          [(0.0, 0.0, 0.0, 0.0, 0.9, CAR)]], [1, 2, 3, 1]),
        # across generations (pedestrians, max_dist 1 m): the track of frame 0 at -1 is missed in frame 1, where a new one appears
        # at +1; the detection at 0 is 1 m from both and takes the younger track, which comes first in the list
        ([[(-1.0, 0.0, 0.0, 0.0, 0.9, PED)], [(1.0, 0.0, 0.0, 0.0, 0.9, PED)], [(0.0, 0.0, 0.0, 0.0, 0.9, PED)]], [1, 2, 2]),
    ]
    for frames, expected in cases:
        d, plan = _hand_scene(frames)
        rid, rhits, _ = R.track_reference(d["rec"], d["cls"], d["row_start"], d["row_count"], *plan, TC, MD, 3)
        ids, hits, status = _device_run(d, plan, 3)
        assert status == 0 and rid.tolist() == expected, (rid.tolist(), expected)
        assert ids.tolist() == expected and np.array_equal(hits, rhits), (ids.tolist(), expected)


@pytest.mark.gpu
def test_runs_are_bitwise_identical_and_overwrite_a_sentinel():
    d, plan, (rid, rhits, _), max_age = _case("wide_300")
    dev = torch.device("cuda", 0)
    outs = []
    for fill in (-7, 0x5A5A5A5A):
        out = (torch.full((len(rid),), fill, dtype=torch.int32, device=dev),
               torch.full((len(rid),), fill, dtype=torch.int32, device=dev))
        outs.append(_device_run(d, plan, max_age, out=out))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    assert np.array_equal(outs[0][0], rid) and np.array_equal(outs[0][1], rhits)
    untracked = ~np.isin(d["cls"], TRACKED)
    assert untracked.any() and (outs[0][0][untracked] == 0).all() and (outs[0][1][untracked] == 0).all()


@pytest.mark.gpu
def test_device_layout_tensors_and_score_threshold():
    """The layout given as device tensors (the kernel's own checks) and a threshold that drops rows."""
    from unidistill_amd.ops import tracking as T
    d, plan, _, max_age = _case("shuffled")
    rid, rhits, _ = R.track_reference(d["rec"], d["cls"], d["row_start"], d["row_count"], *plan, TC, MD, max_age, 0.4)
    dev = torch.device("cuda", 0)
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (d["row_start"], d["row_count"], *plan)]
    ids, hits, status = T.track_scenes(torch.from_numpy(np.array(d["rec"])).to(dev), torch.from_numpy(np.array(d["cls"])).to(dev),
                                       *on_dev, track_class=TC, max_dist=MD, max_age=max_age, score_threshold=0.4)
    assert int(status.item()) == 0
    assert np.array_equal(ids.cpu().numpy(), rid) and np.array_equal(hits.cpu().numpy(), rhits)
    assert ((d["rec"][:, 9] < 0.4) & (rid == 0) & np.isin(d["cls"], TRACKED)).any()
    # a count above the cap in a device tensor: reported by the kernel, the frame treated as empty
    on_dev[1] = on_dev[1].clone()
    on_dev[1][0] = T.MAX_BOXES + 1
    _, _, status = T.track_scenes(torch.from_numpy(np.array(d["rec"])).to(dev), torch.from_numpy(np.array(d["cls"])).to(dev),
                                  *on_dev, track_class=TC, max_dist=MD, max_age=max_age)
    assert int(status.item()) & T.ST_COUNT and "more than" in T.status_text(int(status.item()))


@pytest.mark.gpu
def test_nan_velocity_sets_the_status_bit():
    from unidistill_amd.ops import tracking as T
    d, plan, _, max_age = _case("empty_frames")
    d = dict(d, rec=np.array(d["rec"]))
    tracked_rows = np.nonzero(np.isin(d["cls"], TRACKED))[0]
    d["rec"][tracked_rows[3], 7] = np.nan
    d["rec"][tracked_rows[5], 9] = np.inf
    rid, rhits, rstatus = R.track_reference(d["rec"], d["cls"], d["row_start"], d["row_count"], *plan, TC, MD, max_age)
    ids, hits, status = _device_run(d, plan, max_age)
    assert status == rstatus == T.ST_NONFINITE and "non-finite" in T.status_text(status)
    assert np.array_equal(ids, rid) and np.array_equal(hits, rhits) and ids[tracked_rows[3]] == 0 == ids[tracked_rows[5]]


@pytest.mark.gpu
def test_over_cap_sizes_are_rejected_on_the_host():
    from unidistill_amd import _lib
    from unidistill_amd.ops import tracking as T
    d, plan, _, _ = _case("one")
    dev = torch.device("cuda", 0)
    rec = torch.zeros((T.MAX_BOXES + 1, 10), dtype=torch.float64, device=dev)
    cls = torch.zeros((T.MAX_BOXES + 1,), dtype=torch.int32, device=dev)
    kw = dict(track_class=TC, max_dist=MD)
    with pytest.raises(ValueError, match="more than 1024"):
        T.track_scenes(rec, cls, [0], [T.MAX_BOXES + 1], *plan, **kw)
    for bad_age in (0, T.MAX_AGE + 1):
        with pytest.raises(ValueError, match="max_age"):
            T.track_scenes(rec, cls, [0], [1], *plan, max_age=bad_age, **kw)
    with pytest.raises(ValueError, match="outside"):
        T.track_scenes(rec, cls, [T.MAX_BOXES], [2], *plan, **kw)
    with pytest.raises(ValueError, match="frame_sample"):
        T.track_scenes(rec, cls, [0], [1], [1], plan[1], plan[2], **kw)
    with pytest.raises(ValueError, match="classes"):
        T.track_scenes(rec, cls, [0], [1], *plan, track_class=[True] * 16, max_dist=[1.0] * 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        T.track_scenes(rec.cpu(), cls, [0], [1], *plan, **kw)
    lib = _lib.load()
    assert lib.ud_track_workspace_bytes(1, 0) == 0 == lib.ud_track_workspace_bytes(1, T.MAX_AGE + 1)
    assert lib.ud_track_workspace_bytes(0, 3) == 0 and lib.ud_track_workspace_bytes(150, 3) == 150 * 3 * 1024 * 24
