"""CPU: tests/track_interp_reference.py -- the float64 restatement of the track interpolation of DESIGN §2.25 -- on hand-built
scenes whose answers are known."""
import math

import numpy as np
import pytest

import track_interp_cases as K
import track_interp_reference as I
import track_metric_reference as R


def _run(case, mode="devkit", **kw):
    d = K.build(**case) if "frames" in case else dict(case)
    return d, I.interpolate_reference(*[d[k] for k in K.ARGS], tracked=d["tracked"], class_range=d["class_range"], mode=mode,
                                      **kw)


def _lerp(a, b, w):
    omw = 1.0 - w
    p, q = omw * a, w * b
    return p + q


def test_three_frames_middle_row_missing():
    d, out = _run(K.HAND["one_track_three_frames"])
    for side, vals in ((out["pred"], d["rec"]), (out["gt"], d["gt_xyz"])):
        assert side["count"].tolist() == [1, 1, 1] and side["start"].tolist() == [0, 1, 2]
        assert side["src_row"].tolist() == [0, -1, 1] and side["num_interpolated"] == 1 and side["holes"] == [1]
        assert side["vals"][0].tolist() == vals[0].tolist() and side["vals"][2].tolist() == vals[1].tolist()
        for i in range(vals.shape[1]):
            if i != 6:
                assert side["vals"][1, i] == _lerp(vals[0, i], vals[1, i], 0.5)
    yaw = d["rec"][:, 6]
    assert out["pred"]["vals"][1, 6] == yaw[0] + 0.5 * math.remainder(yaw[1] - yaw[0], 2.0 * math.pi)
    assert out["pred"]["key"].tolist() == [1, 1, 1] and out["gt"]["key"].tolist() == [0, 0, 0] and out["status"] == 0


def test_holes_of_1_2_6_frames_and_both_modes():
    d, dev = _run(K.HAND["holes_1_2_6"])
    _, lin = _run(K.HAND["holes_1_2_6"], mode="linear")
    ts = K.UNEVEN_TS
    for out in (dev, lin):
        assert sorted(out["pred"]["holes"]) == [1, 2, 6] and sorted(out["gt"]["holes"]) == [1, 2, 6]
        assert out["pred"]["num_interpolated"] == out["gt"]["num_interpolated"] == 9
        assert out["pred"]["count"].tolist() == [3] * 10 and out["gt"]["count"].tolist() == [3] * 10
    # GT instance 3 (key 2) is missing in frames 1 .. 6: L = frame 0, R = frame 7
    g0 = int(np.nonzero((d["gt_instance"] == 3))[0][0])
    g7 = int(np.nonzero((d["gt_instance"] == 3))[0][1])
    for f in range(1, 7):
        row = int(dev["gt"]["start"][f]) + int(np.nonzero(dev["gt"]["key"][dev["gt"]["start"][f]:][:3] == 2)[0][0])
        assert dev["gt"]["src_row"][row] == -1 and lin["gt"]["src_row"][row] == -1
        wd = float(ts[7] - ts[f]) / float(ts[7] - ts[0])
        wl = float(ts[f] - ts[0]) / float(ts[7] - ts[0])
        assert dev["gt"]["vals"][row, 0] == _lerp(d["gt_xyz"][g0, 0], d["gt_xyz"][g7, 0], wd)
        assert lin["gt"]["vals"][row, 0] == _lerp(d["gt_xyz"][g0, 0], d["gt_xyz"][g7, 0], wl)
    assert dev["pred"]["vals"].tobytes() != lin["pred"]["vals"].tobytes()          # uneven timestamps: the modes differ
    # "linear" moves forward in time through the hole, "devkit" mirrored
    xs = [lin["gt"]["vals"][int(lin["gt"]["start"][f]) + int(np.nonzero(lin["gt"]["key"][lin["gt"]["start"][f]:][:3] == 2)[0][0]), 0]
          for f in range(1, 7)]
    assert xs == sorted(xs)


def test_uniform_one_frame_holes_modes_bit_equal():
    frames = K.merge(K.track((K.ON(7, (1, 3)), K.ON(7, (2, 5))), 1, 1), K.track((K.ON(7, (5,)), K.ON(7, (1,))), 2, 2, x0=-8.0))
    _, a = _run(dict(frames=frames))
    _, b = _run(dict(frames=frames), mode="linear")
    assert a["pred"]["num_interpolated"] == 3 and a["gt"]["num_interpolated"] == 3
    for side in ("pred", "gt"):
        assert a[side]["vals"].tobytes() == b[side]["vals"].tobytes() and np.array_equal(a[side]["src_row"], b[side]["src_row"])


def test_hole_across_a_frame_without_rows():
    d, out = _run(K.HAND["hole_across_empty_frame"])
    assert np.diff(d["gt_off"])[2] == 0 and d["row_count"][2] == 0
    # track 1 misses only the empty frame; track 2's GT misses frames 1 and 2, its prediction frames 2 and 3
    assert out["gt"]["count"].tolist() == [2] * 5 and out["pred"]["count"].tolist() == [2] * 5
    assert out["gt"]["src_row"][out["gt"]["start"][2]:][:2].tolist() == [-1, -1]
    assert sorted(out["gt"]["holes"]) == [1, 2] and sorted(out["pred"]["holes"]) == [1, 2]


def test_first_or_last_frame_only_adds_nothing():
    _, out = _run(K.HAND["first_or_last_only"])
    for side in ("pred", "gt"):
        assert out[side]["num_interpolated"] == 0 and (out[side]["src_row"] >= 0).all()
        assert out[side]["count"].tolist() == [2, 1, 1, 2]


@pytest.mark.parametrize("how", ["range", "num_pts", "keep"])
def test_filtered_middle_row_is_replaced(how):
    frames = K.track((K.ON(3), K.ON(3)))
    d = K.build(frames)
    if how == "range":
        d["gt_xyz"][1, 0] = 60.0                   # car: 50 m
        d["rec"][1, 0] = 60.0
    elif how == "num_pts":
        d["gt_num_pts"][1] = 0
    else:
        d["gt_keep"][1] = False
    _, out = _run(d)
    g = out["gt"]
    assert g["src_row"].tolist() == [0, -1, 2] and g["num_interpolated"] == 1
    assert g["vals"][1, 0] == _lerp(d["gt_xyz"][0, 0], d["gt_xyz"][2, 0], 0.5)
    assert g["vals"][1, 2] == _lerp(d["gt_xyz"][0, 2], d["gt_xyz"][2, 2], 0.5) and g["vals"][1, 2] != d["gt_xyz"][1, 2]
    assert out["pred"]["src_row"].tolist() == ([0, -1, 2] if how == "range" else [0, 1, 2])
    # the metric on the interpolated rows counts three objects; on the rows as given, two
    ref, _ = I.evaluate_interpolated_reference(*[d[k] for k in K.ARGS], tracked=d["tracked"], class_range=d["class_range"],
                                               recall=R.recall_thresholds())
    plain = R.evaluate_reference(*[d[k] for k in K.ARGS], tracked=d["tracked"], class_range=d["class_range"],
                                 recall=R.recall_thresholds())
    assert ref["counts"][0, 0, 1] == 3 and plain["counts"][0, 0, 1] == 2 and ref["counts"][0, 0, 2] == 3 and ref["status"] == 0


def test_yaw_takes_the_short_arc_across_pi():
    d = K.build(K.track((K.ON(3), K.ON(3, (1,)))))
    d["rec"][:, 6] = [3.0, -3.0]
    _, out = _run(d)
    yaw = out["pred"]["vals"][1, 6]
    assert yaw == 3.0 + 0.5 * math.remainder(-6.0, 2.0 * math.pi) and 3.0 < yaw < 3.3          # past pi, not re-wrapped
    d["rec"][:, 6] = [-3.0, 3.0]
    _, out = _run(d)
    assert -3.3 < out["pred"]["vals"][1, 6] < -3.0
    d["rec"][:, 6] = [0.25, 1.0]
    _, out = _run(d)
    assert out["pred"]["vals"][1, 6] == 0.25 + 0.5 * 0.75


def test_duplicate_key_and_equal_timestamps_rejected():
    frames = K.track((K.ON(3), K.ON(3)))
    frames[1] = (frames[1][0], frames[1][1] + [(1, 0.0, 0.0, 0.4)])
    with pytest.raises(ValueError, match="twice"):
        _run(dict(frames=frames))
    frames = K.track((K.ON(3), K.ON(3)))
    frames[1] = (frames[1][0] + [(1, 0.0, 1.0)], frames[1][1])
    with pytest.raises(ValueError, match="twice"):
        _run(dict(frames=frames))
    with pytest.raises(ValueError, match="same timestamp"):
        _run(dict(frames=K.track((K.ON(3), K.ON(3))), timestamps=[0, 500_000, 500_000]))
    # a duplicate among rows that are not kept is no duplicate
    frames = K.track((K.ON(3), K.ON(3)))
    frames[1] = (frames[1][0], frames[1][1] + [(1, 500.0, 0.0, 0.4)])
    _, out = _run(dict(frames=frames))
    assert out["pred"]["count"].tolist() == [1, 1, 1]


def test_output_order_kept_rows_then_interpolated_by_key():
    d, out = _run(K.HAND["order"])
    p, g = out["pred"], out["gt"]
    for side, orig_key in ((p, d["track_id"]), (g, None)):
        for s in range(4):
            rows = slice(int(side["start"][s]), int(side["start"][s]) + int(side["count"][s]))
            src, key = side["src_row"][rows], side["key"][rows]
            nk = int((src >= 0).sum())
            assert (src[:nk] >= 0).all() and (src[nk:] == -1).all()               # originals first
            assert (np.diff(src[:nk]) > 0).all() and (np.diff(key[nk:]) > 0).all()  # in row order; then ascending key
            if orig_key is not None:
                assert np.array_equal(key[:nk], orig_key[src[:nk]])
    assert p["key"][p["start"][1]:][:4].tolist() == [7, 2, 4, 9] and p["key"][p["start"][2]:][:4].tolist() == [4, 2, 7, 9]
    assert g["count"].tolist() == [4, 4, 4, 4] and p["count"].tolist() == [4, 4, 4, 4]
    # GT keys are the rank of the instance id within the scene: 20, 30, 40, 50 -> 0 .. 3
    assert sorted(set(g["key"].tolist())) == [0, 1, 2, 3]
    assert g["key"][g["start"][2]:][:4].tolist()[2:] == [0, 3]                     # instances 20 and 50 are interpolated in frame 2


def test_status_bits_and_untracked_classes():
    d = K.build(K.track((K.ON(3), K.ON(3))))
    d["rec"][1, 4] = np.nan
    _, out = _run(d)
    assert out["status"] == I.ST_NONFINITE and out["pred"]["src_row"].tolist() == [0, -1, 2]
    d = K.build(K.track((K.ON(3), K.ON(3)), tid=40))
    _, out = _run(d)
    assert out["status"] == I.ST_KEY and out["pred"]["count"].sum() == 0
    _, out = _run(K.build(K.merge(K.track((K.ON(2), K.ON(2)), 1, 1), K.track((K.ON(2), K.ON(2)), 2, 2, x0=-3.0))),
                  max_boxes_per_sample=1)
    assert out["status"] == I.ST_BOXES
    # class 2 (construction_vehicle) is not tracked: its rows leave, nothing is interpolated for them
    frames = [([(1, 0.0, 0.0, 2)], [(1, 0.0, 0.0, 0.5, 2)]), ([], []), ([(1, 0.0, 0.0, 2)], [(1, 0.0, 0.0, 0.5, 2)])]
    _, out = _run(dict(frames=frames))
    assert out["pred"]["count"].sum() == 0 and out["gt"]["count"].sum() == 0 and out["status"] == 0
