"""GPU: ops.track_metric.evaluate_tracks (csrc/track_metric.hip) against tests/track_metric_reference.py on seeded
scenes -- objects that move, appear and vanish, noisy detections with misses, id changes and false positives, continuous
coordinates and scores -- at the smallest shapes that cross each internal boundary.  Integers are equal as integers, thresholds
and dist_sum as bits; the events of a chosen pass give the same pairs per frame."""
import numpy as np
import pytest
import torch

import track_metric_cases as H
import track_metric_reference as R

KEYS = ("rec", "cls", "track_id", "row_start", "row_count", "gt_xyz", "gt_cls", "gt_instance", "gt_num_pts", "gt_keep", "gt_off",
        "ego", "scene", "timestamp_us")
TRACKED = [c for c, on in enumerate(R.default_config()[0]) if on]


def _device(d, recall, events_pass=None, **kw):
    from unidistill_amd.ops import track_metric as M
    dev = torch.device("cuda", 0)
    tracked, rng = R.default_config()
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)
    args = dict(track_class=tracked, class_range=rng, recall=recall, events_pass=events_pass)
    args.update(kw)
    return M.evaluate_tracks(up(d["rec"], np.float64), up(d["cls"], np.int32), up(d["track_id"], np.int32), d["row_start"],
                             d["row_count"], up(d["gt_xyz"], np.float64).reshape(-1, 3), up(d["gt_cls"], np.int32),
                             up(d["gt_num_pts"], np.int32), up(d["gt_keep"], np.uint8), d["gt_instance"], d["gt_off"],
                             up(d["ego"], np.float64), d["scene"], d["timestamp_us"], **args)


def _reference(d, recall, events_pass=None, max_boxes=500):
    tracked, rng = R.default_config()
    return R.evaluate_reference(*[d[k] for k in KEYS], tracked=tracked, class_range=rng, recall=recall, events_pass=events_pass,
                                max_boxes_per_sample=max_boxes)


def _compare(d, recall=None, events_pass=None, status=0, max_boxes=500):
    recall = R.recall_thresholds() if recall is None else recall
    out = _device(d, recall, events_pass, max_boxes_per_sample=max_boxes)
    ref = _reference(d, recall, events_pass, max_boxes)
    got = {k: out[k].cpu().numpy() for k in ("counts", "dist_sum", "valid", "thresholds", "num_scores")}
    assert int(out["status"].item()) == ref["status"] == status
    assert np.array_equal(got["num_scores"], ref["num_scores"])
    assert got["thresholds"].tobytes() == ref["thresholds"].tobytes()                  # equal as bits, NaN included
    assert np.array_equal(got["valid"], ref["valid"])
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], ref["counts"])
    err = np.abs(got["dist_sum"] - ref["dist_sum"]) / np.maximum(np.abs(ref["dist_sum"]), 1e-300)
    print("dist_sum max relative error", float(err.max()))
    assert float(err.max()) <= 1e-12
    assert got["dist_sum"].tobytes() == ref["dist_sum"].tobytes()      # the device's float64 square root rounds as the host's does
    if events_pass is not None:
        et, er = out["events_type"].cpu().numpy(), out["events_row"].cpu().numpy()
        _compare_events(d, et, er, ref["events_type"], ref["events_row"])
    return out, ref


def _compare_events(d, et, er, ret, rer):
    """Per frame and class: the same number of pairs and the same cost within 1e-9 (the optimum, not the identity of the pairs)."""
    assert np.array_equal(et < 0, ret < 0)
    for s in range(len(d["row_start"])):
        g = np.arange(d["gt_off"][s], d["gt_off"][s + 1])
        for c in TRACKED:
            rows = g[d["gt_cls"][g] == c]
            cost = []
            for typ, row in ((et, er), (ret, rer)):
                m = rows[typ[rows] > 0]
                assert (row[m] >= 0).all() and len(set(row[m].tolist())) == len(m)
                dxy = d["gt_xyz"][m, :2] - d["rec"][row[m], :2]
                cost.append((len(m), float(np.sqrt((dxy * dxy).sum(1)).sum())))
            assert cost[0][0] == cost[1][0] and abs(cost[0][1] - cost[1][1]) <= 1e-9, (s, c, cost)
    assert np.array_equal(et, ret) and np.array_equal(er, rer)          # continuous data: the optimum is unique


@pytest.mark.gpu
def test_one_pair_one_frame():
    d = H.build([([(1, 3.0, 4.0)], [(1, 3.5, 4.0, 0.7)])])
    out, ref = _compare(d, events_pass="none")
    assert ref["counts"][0, 0, 2] == 1 and out["classes"] == TRACKED


@pytest.mark.gpu
def test_scene_with_empty_frames_and_all_classes():
    """300 rows a frame over the 7 tracked classes and 3 untracked ones; frames 0 and 3 are empty; samples and rows shuffled."""
    d = R.make_case(1, num_scenes=2, num_frames=7, num_objects=140, classes=TRACKED, extra_classes=(2, 5, 9) * 8,
                    empty_frames=(0, 3), shuffle_samples=True, false_pos=20)
    assert d["row_count"].max() >= 150
    out, ref = _compare(d, events_pass=3)
    assert ref["counts"][:, 0, 3].sum() > 0 and ref["counts"][:, 0, 8].sum() > 0 and (ref["valid"][:, 1:].sum(1) > 5).all()


@pytest.mark.gpu
def test_more_than_a_wave_of_one_class():
    d = R.make_case(2, num_scenes=1, num_frames=5, num_objects=65, classes=[0], spread=12.0, false_pos=6)
    assert np.diff(d["gt_off"]).max() >= 65 - 25
    d2 = R.make_case(2, num_scenes=1, num_frames=3, num_objects=90, classes=[0], spread=10.0, false_pos=10)
    d2["gt_num_pts"][:] = 5
    _compare(d, events_pass="none")
    _compare(d2, events_pass=0)


@pytest.mark.gpu
def test_frame_cap_512_by_512():
    """512 objects and 512 hypotheses of one class in every frame, dense enough for long augmenting paths."""
    rng = np.random.default_rng(4)
    frames = []
    p = rng.uniform(-18, 18, (512, 2))
    for f in range(3):
        q = p + rng.normal(0, 0.6, p.shape)
        ids = rng.permutation(512) + 1 if f == 2 else np.arange(512) + 1
        frames.append(([(i + 1, p[i, 0], p[i, 1]) for i in range(512)],
                       [(int(ids[i]), q[i, 0], q[i, 1], float(rng.uniform(0.2, 1.0))) for i in rng.permutation(512)]))
        p = p + rng.normal(0, 0.3, p.shape)
    d = H.build(frames)
    out, ref = _compare(d, recall=np.array([0.3, 0.8]), events_pass="none", max_boxes=512)
    assert ref["counts"][0, 0, 1] == 3 * 512 and ref["counts"][0, 0, 3] > 50


@pytest.mark.gpu
def test_one_sided_classes_and_single_frame_scene():
    """Class 0 has ground truth and no predictions, class 1 the reverse; a scene of one frame."""
    frames = [([(1, 0.0, 0.0), (2, 5.0, 0.0)], [(1, 1.0, 1.0, 0.5, 1), (2, 6.0, 1.0, 0.4, 1)])]
    out, ref = _compare(H.build(frames), events_pass="none")
    assert ref["counts"][0, 0, 5] == 2 and ref["counts"][out["classes"].index(1), 0, 4] == 2
    assert np.isnan(ref["thresholds"]).all()


@pytest.mark.gpu
def test_300_scenes_and_threshold_counts():
    d = R.make_case(5, num_scenes=300, num_frames=3, num_objects=6, classes=TRACKED[:3], false_pos=1)
    _compare(d, recall=np.array([0.2, 0.5, 0.8]))
    small = R.make_case(6, num_scenes=2, num_frames=6, num_objects=12, classes=TRACKED[:2])
    _compare(small, recall=np.array([0.5]), events_pass=0)
    _compare(small, recall=np.round(np.linspace(0.05, 1.0, 64), 12))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(H.HAND_CASES))
def test_hand_built_cases(name):
    """The identity of the pairs where the optimum is unique (tests/track_metric_cases.py)."""
    _compare(H.build(H.HAND_CASES[name]), events_pass="none")


@pytest.mark.gpu
def test_rerun_over_sentinels_and_status():
    from unidistill_amd import _lib
    d = R.make_case(7, num_scenes=3, num_frames=6, num_objects=30, classes=TRACKED, false_pos=4)
    recall = R.recall_thresholds()
    a = _device(d, recall, events_pass=2)
    first = {k: a[k].cpu().numpy().tobytes() for k in ("counts", "dist_sum", "valid", "thresholds", "num_scores", "events_type",
                                                        "events_row")}
    _lib.workspace(torch.device("cuda", 0), 1, slot="track_metric").fill_(0xA5)
    b = _device(d, recall, events_pass=2)
    assert {k: b[k].cpu().numpy().tobytes() for k in first} == first
    bad = dict(d, rec=d["rec"].copy(), gt_xyz=d["gt_xyz"].copy())
    bad["rec"][np.nonzero(d["track_id"] > 0)[0][0], 1] = np.inf
    bad["gt_xyz"][np.nonzero(np.isin(d["gt_cls"], TRACKED) & d["gt_keep"] & (d["gt_num_pts"] > 0))[0][0], 0] = np.nan
    _compare(bad, status=R.ST_NONFINITE)
    kept = np.nonzero(~np.isnan(_reference(d, recall[:1])["track_score"]))[0]
    over = dict(d, track_id=d["track_id"].copy())
    over["track_id"][kept[5]] = 10 ** 6                                    # a kept row with an id beyond its scene's rows
    _compare(over, status=R.ST_ID)
    out = _device(d, recall, max_boxes_per_sample=3)
    assert int(out["status"].item()) & R.ST_BOXES


@pytest.mark.gpu
def test_host_rejections():
    from unidistill_amd.evaluation import NuScenesTracker, NuScenesTrackingEval
    from unidistill_amd.ops import track_metric as M
    d = R.make_case(8, num_scenes=1, num_frames=2, num_objects=5, classes=[0])
    recall = R.recall_thresholds()
    with pytest.raises(ValueError, match="recall"):
        _device(d, np.linspace(0.1, 1, 65))
    with pytest.raises(ValueError, match="events_pass"):
        _device(d, recall, events_pass=40)
    with pytest.raises(ValueError, match="row_count"):
        _device(dict(d, row_count=d["row_count"][:-1]), recall)
    with pytest.raises(ValueError, match="gt_off"):
        _device(dict(d, gt_off=d["gt_off"][::-1].copy()), recall)
    with pytest.raises(ValueError, match="twice"):
        _device(dict(d, gt_instance=np.zeros_like(d["gt_instance"])), recall)
    with pytest.raises(ValueError, match="classes"):
        _device(d, recall, track_class=[True] * 16, class_range=[1.0] * 16)
    big = H.build([([], [(1, 0.0, 0.0, 0.5)] * 513)])
    with pytest.raises(ValueError, match="more than 512"):
        _device(big, recall)
    many = H.build([([(i, 0.0, 0.0) for i in range(400)], []) for _ in range(11)])
    many["gt_instance"] = np.arange(len(many["gt_instance"]), dtype=np.int64)
    with pytest.raises(ValueError, match="4096"):
        _device(many, recall)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.evaluate_tracks(torch.zeros((1, 10), dtype=torch.float64), *[None] * 13, track_class=[True], class_range=[1.0],
                          recall=recall)
    assert "non-finite" in M.status_text(1) and "max_boxes" in M.status_text(2) and M.status_text(0) == ""
    ev = NuScenesTrackingEval(device=torch.device("cuda", 0))
    with pytest.raises(RuntimeError, match="add_ground_truth"):
        ev.compute(NuScenesTracker())
    ev.add_ground_truth(d["gt_xyz"], d["gt_cls"], d["gt_instance"], d["gt_num_pts"], d["gt_sample"], d["ego"], d["scene"],
                        d["timestamp_us"])
    with pytest.raises(RuntimeError, match="track\\(\\) first"):
        ev.compute(NuScenesTracker())
