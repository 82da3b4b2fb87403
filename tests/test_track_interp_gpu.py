"""GPU: ops.track_metric.interpolate_tracks (csrc/track_interp.hip) against tests/track_interp_reference.py.  Counts,
layouts, classes, keys and src_row are equal as integers and every float column as bits -- the yaw included, which holds only if
the device's remainder() is exact."""
import numpy as np
import pytest
import torch

import track_interp_cases as K
import track_interp_reference as I
import track_metric_cases as H
import track_metric_reference as R

TRACKED = [c for c, on in enumerate(R.default_config()[0]) if on]
MAX_AGE = 3          # the tracker's default: a predicted track from the device tracker has no longer hole


def _device(d, mode="devkit", **kw):
    from unidistill_amd.ops import track_metric as M
    dev = torch.device("cuda", 0)
    tracked, rng = R.default_config()
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(dev)
    args = dict(track_class=tracked, class_range=rng, mode=mode)
    args.update(kw)
    return M.interpolate_tracks(up(d["rec"], np.float64), up(d["cls"], np.int32), up(d["track_id"], np.int32), d["row_start"],
                                d["row_count"], up(d["gt_xyz"], np.float64).reshape(-1, 3), up(d["gt_cls"], np.int32),
                                up(d["gt_num_pts"], np.int32), up(d["gt_keep"], np.uint8), d["gt_instance"], d["gt_off"],
                                up(d["ego"], np.float64), d["scene"], d["timestamp_us"], **args)


def _reference(d, mode="devkit", **kw):
    tracked, rng = R.default_config()
    return I.interpolate_reference(*[d[k] for k in K.ARGS], tracked=tracked, class_range=rng, mode=mode, **kw)


def _bytes(out):
    return {f"{s}.{k}": out[s][k].cpu().numpy().tobytes() for s, v in (("pred", "rec"), ("gt", "xyz"))
            for k in (v, "cls", "key", "src_row")}


def _compare(d, mode="devkit", ref=None):
    ref = _reference(d, mode) if ref is None else ref
    out = _device(d, mode)
    assert ref["status"] == 0 and int(out["status"].item()) == 0
    for side, vals in (("pred", "rec"), ("gt", "xyz")):
        got, want = out[side], ref[side]
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["start"], want["start"]), side
        assert got["num_interpolated"] == want["num_interpolated"], side
        for k in ("cls", "key", "src_row"):
            g = got[k].cpu().numpy()
            assert g.dtype == np.int32 and np.array_equal(g, want[k]), (side, k)
        g = got[vals].cpu().numpy()
        assert g.shape == want["vals"].shape
        diff = np.nonzero((g.view(np.int64) != want["vals"].view(np.int64)).any(0))[0]
        print(side, "columns that differ in a bit:", diff.tolist())
        assert g.tobytes() == want["vals"].tobytes(), (side, diff.tolist())
    assert np.array_equal(out["gt_class_rows"], np.bincount(ref["gt"]["cls"], minlength=len(out["gt_class_rows"])))
    return out, ref


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["devkit", "linear"])
@pytest.mark.parametrize("name", sorted(K.HAND))
def test_hand_built_cases(name, mode):
    out, ref = _compare(K.build(**K.HAND[name]), mode)
    if name == "one_track_three_frames":
        assert out["pred"]["src_row"].tolist() == [0, -1, 1] and out["gt"]["num_interpolated"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["range", "num_pts", "keep"])
def test_filtered_middle_row_is_replaced(how):
    d = K.build(K.track((K.ON(3), K.ON(3))))
    if how == "range":
        d["gt_xyz"][1, 0] = d["rec"][1, 0] = 60.0
    elif how == "num_pts":
        d["gt_num_pts"][1] = 0
    else:
        d["gt_keep"][1] = False
    out, _ = _compare(d)
    assert out["gt"]["src_row"].tolist() == [0, -1, 2]


@pytest.mark.gpu
def test_yaw_across_pi():
    d = K.build(K.track((K.ON(4), K.ON(4, (1, 2)))), timestamps=K.UNEVEN_TS[:4])
    for yaws in ([3.0, -3.0], [-3.1, 3.1], [0.25, 1.0], [3.0, 3.0 - 2 * np.pi]):
        d["rec"][:, 6] = yaws
        _compare(d)
        _compare(d, "linear")


@pytest.mark.gpu
def test_seeded_scenes_with_long_holes():
    """Shuffled samples, the 7 tracked and 3 untracked classes, empty frames, detections missing half of the time."""
    d = R.make_case(21, num_scenes=3, num_frames=12, num_objects=40, classes=TRACKED, extra_classes=(2, 5, 9) * 3,
                    empty_frames=(4,), shuffle_samples=True, miss=0.5, switch=0.02, false_pos=4)
    ref = _reference(d)
    assert ref["pred"]["num_interpolated"] > 0 and ref["gt"]["num_interpolated"] > 0
    assert max(ref["pred"]["holes"]) > MAX_AGE and max(ref["pred"]["holes"] + ref["gt"]["holes"]) > MAX_AGE
    _compare(d, ref=ref)
    _compare(d, "linear")


@pytest.mark.gpu
def test_more_rows_than_a_wave_and_long_gt_holes():
    d = R.make_case(22, num_scenes=2, num_frames=9, num_objects=150, classes=TRACKED[:2], spread=40.0, miss=0.3, false_pos=10)
    d["gt_num_pts"][np.random.default_rng(1).random(len(d["gt_num_pts"])) < 0.6] = 0       # GT holes of many frames
    ref = _reference(d)
    assert ref["gt"]["count"].max() > 64 and max(ref["gt"]["holes"]) > MAX_AGE and ref["pred"]["num_interpolated"] > 0
    _compare(d, ref=ref)


@pytest.mark.gpu
def test_300_scenes():
    d = R.make_case(23, num_scenes=300, num_frames=4, num_objects=6, classes=TRACKED[:3], miss=0.4, false_pos=1)
    out, ref = _compare(d)
    assert ref["pred"]["num_interpolated"] > 100 and ref["gt"]["num_interpolated"] > 0


def _full_frame(extra):
    """Frame 1 holds 500 kept predictions (the devkit's cap) and misses `extra` tracks that frames 0 and 2 hold."""
    far = [(501 + i, 1.0 + 0.05 * i, 4.0, 0.5) for i in range(extra)]
    near = [(i + 1, -20.0 + 0.08 * i, -3.0, 0.4) for i in range(500)]
    return H.build([([], far), ([], near), ([], far)])


@pytest.mark.gpu
def test_512_rows_after_interpolation_and_513():
    d = _full_frame(12)
    out, ref = _compare(d)
    assert out["pred"]["count"].tolist() == [12, 512, 12] and out["pred"]["num_interpolated"] == 12
    with pytest.raises(ValueError, match="sample 1 has 513 prediction rows after interpolation"):
        _device(_full_frame(13))
    ends = [(i, 0.05 * i, 0.0) for i in range(300)]                                 # 300 objects that frame 1 misses
    out, ref = _compare(H.build([(ends, []), ([(i, 0.05 * i, 1.0) for i in range(300, 512)], []), (ends, [])]))
    assert out["gt"]["count"].tolist() == [300, 512, 300]
    gt = H.build([(ends, []), ([(i, 0.05 * i, 1.0) for i in range(300, 513)], []), (ends, [])])
    with pytest.raises(ValueError, match="sample 1 has 513 ground-truth rows after interpolation"):
        _device(gt)


@pytest.mark.gpu
def test_rerun_over_sentinels_and_two_runs():
    from unidistill_amd import _lib
    d = R.make_case(24, num_scenes=3, num_frames=8, num_objects=30, classes=TRACKED, miss=0.4, false_pos=4)
    first = _bytes(_device(d))
    assert _bytes(_device(d)) == first
    _lib.workspace(torch.device("cuda", 0), 1, slot="track_interp").fill_(0xA5)
    assert _bytes(_device(d)) == first


@pytest.mark.gpu
def test_status_bits(monkeypatch):
    from unidistill_amd.ops import track_metric as M
    d = R.make_case(25, num_scenes=2, num_frames=5, num_objects=12, classes=TRACKED, miss=0.3)
    kept = np.nonzero(_reference(d)["pred"]["src_row"] >= 0)[0]
    row = int(_reference(d)["pred"]["src_row"][kept[3]])
    bad = dict(d, rec=d["rec"].copy())
    bad["rec"][row, 7] = np.inf
    assert _reference(bad)["status"] == I.ST_NONFINITE
    with pytest.raises(ValueError, match="non-finite"):
        _device(bad)
    bad = dict(d, gt_xyz=d["gt_xyz"].copy())
    bad["gt_xyz"][np.nonzero(np.isin(d["gt_cls"], TRACKED) & d["gt_keep"] & (d["gt_num_pts"] > 0))[0][0], 2] = np.nan
    assert _reference(bad)["status"] == I.ST_NONFINITE
    with pytest.raises(ValueError, match="non-finite"):
        _device(bad)
    over = dict(d, track_id=d["track_id"].copy())
    over["track_id"][row] = 10 ** 6
    assert _reference(over)["status"] == I.ST_KEY
    with pytest.raises(ValueError, match="track id exceeds"):
        _device(over)
    assert _reference(d, max_boxes_per_sample=3)["status"] == I.ST_BOXES
    with pytest.raises(ValueError, match="max_boxes_per_sample"):
        _device(d, max_boxes_per_sample=3)
    twice = dict(d, track_id=d["track_id"].copy())
    s = int(np.argmax(d["row_count"]))
    kept_rows = set(_reference(d)["pred"]["src_row"].tolist())
    rows = [r for r in range(d["row_start"][s], d["row_start"][s] + d["row_count"][s]) if r in kept_rows]
    twice["track_id"][rows[1]] = d["track_id"][rows[0]]
    with pytest.raises(ValueError, match="twice"):
        _reference(twice)
    with pytest.raises(ValueError, match="appears twice in one sample"):
        _device(twice)
    twice = dict(d, gt_instance=d["gt_instance"].copy())
    g = np.nonzero(np.isin(d["gt_cls"], TRACKED) & d["gt_keep"] & (d["gt_num_pts"] > 0) & (d["gt_sample"] == 0))[0]
    twice["gt_instance"][g[1]] = d["gt_instance"][g[0]]
    with pytest.raises(ValueError, match="appears twice in one sample"):
        _device(twice)
    # a frame list that names a sample outside the inputs: the frame counts as empty and the status says so
    real = M.scene_frames

    def broken(scene, ts):
        fs, off, dt = real(scene, ts)
        fs = fs.copy()
        fs[1] = -1
        return fs, off, dt
    monkeypatch.setattr(M, "scene_frames", broken)
    with pytest.raises(ValueError, match="do not fit the inputs"):
        _device(d)
    assert M.interp_status_text(0) == "" and all(M.interp_status_text(1 << b) for b in range(5))


@pytest.mark.gpu
def test_host_rejections():
    from unidistill_amd.ops import track_metric as M
    d = R.make_case(26, num_scenes=1, num_frames=3, num_objects=5, classes=[0])
    with pytest.raises(ValueError, match="mode"):
        _device(d, "nearest")
    same = dict(d, timestamp_us=d["timestamp_us"].copy())
    same["timestamp_us"][1] = same["timestamp_us"][0]
    with pytest.raises(ValueError, match="same timestamp"):
        _device(same)
    with pytest.raises(ValueError, match="same timestamp"):
        _reference(same)
    with pytest.raises(ValueError, match="row_count"):
        _device(dict(d, row_count=d["row_count"][:-1]))
    with pytest.raises(ValueError, match="gt_off"):
        _device(dict(d, gt_off=d["gt_off"][::-1].copy()))
    with pytest.raises(ValueError, match="classes"):
        _device(d, track_class=[True] * 16, class_range=[1.0] * 16)
    with pytest.raises(ValueError, match="max_boxes_per_sample"):
        _device(d, max_boxes_per_sample=0)
    with pytest.raises(ValueError, match="more than 512"):
        _device(H.build([([], [(1, 0.0, 0.0, 0.5)] * 513)]))
    many = H.build([([(i, 0.0, 0.0) for i in range(400)], []) for _ in range(11)])
    many["gt_instance"] = np.arange(len(many["gt_instance"]), dtype=np.int64)
    with pytest.raises(ValueError, match="4096"):
        _device(many)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.interpolate_tracks(torch.zeros((1, 10), dtype=torch.float64), *[None] * 13, track_class=[True], class_range=[1.0])
