"""CPU: the host side of the GT-sampling paste (ops/gt_paste.py) -- the sampler's draws, the database's
construction-time filter, the paste record, the segment limit, the header's new prototypes -- and the float64
reference's own generators (tests/gt_paste_reference.py): the committed seeds stay inside the caps the GPU tests assert."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gt_paste_reference as ref                                                   # noqa: E402

from unidistill_amd.ops import gt_paste as gp                                       # noqa: E402  (absent before this feature)
from unidistill_amd.ops import input_prep as ip                                     # noqa: E402
from unidistill_amd.ops import lidar_prep as lp                                     # noqa: E402

NAMES = ["car", "truck", "bicycle", "bus"]


def small_db(n_per_class=(7, 3, 5), rows=None, **kw):
    """A host-resident database: class k has n_per_class[k] objects, object i has rows[i] points (default i % 4 + 3)."""
    ids = np.concatenate([np.full(n, k) for k, n in enumerate(n_per_class)])
    n = len(ids)
    rows = np.array([i % 4 + 3 for i in range(n)] if rows is None else rows)
    offsets = np.concatenate([[0], np.cumsum(rows)])
    pts = np.arange(offsets[-1] * 5, dtype=np.float32).reshape(-1, 5)
    boxes = np.zeros((n, 9), np.float32)
    boxes[:, 0] = np.arange(n) * 10.0
    boxes[:, 3:6] = 1.0
    return gp.ObjectDatabase.from_arrays(pts, offsets, boxes, ids, NAMES[:len(n_per_class)], device="cpu", **kw)


def sample(n_car=0, n_truck=0, with_names=True):
    labels = np.array([0] * n_car + [1] * n_truck, np.int64)
    d = {"points": np.zeros((4, 5), np.float32), "gt_boxes": np.zeros((len(labels), 9), np.float32) + 1.0,
         "gt_labels": labels}
    if with_names:
        d["gt_names"] = np.array(NAMES, object)[labels]
    return d


def test_reexported_from_input_prep():
    assert ip.GTSampling is gp.GTSampling and ip.ObjectDatabase is gp.ObjectDatabase and ip.gt_paste is gp.gt_paste


def test_group_counts_with_and_without_limit_whole_scene():
    db = small_db()
    groups = ["car:4", "truck:2", "bicycle:3", "bus:5"]                             # bus: not in the database's classes
    t = gp.GTSampling(db, NAMES, groups, seed=1)
    p = t(sample(n_car=3, n_truck=5))["lidar_aug"]["paste"]
    assert np.bincount(p["cand_group"], minlength=4).tolist() == [4, 2, 3, 0]
    for names in (True, False):                                                     # counted from gt_names, else gt_labels
        t = gp.GTSampling(db, NAMES, groups, limit_whole_scene=True, seed=1)
        p = t(sample(n_car=3, n_truck=5, with_names=names))["lidar_aug"]["paste"]
        assert np.bincount(p["cand_group"], minlength=4).tolist() == [1, 0, 3, 0]    # max(0, N - count in scene)
    assert (np.diff(p["cand_group"]) >= 0).all() and p["cand_group"].dtype == np.int32
    assert (db.class_ids[p["cand_idx"]] == np.array([0, 2, 2, 2])).all()
    assert p["cand_labels"].tolist() == [0, 2, 2, 2]
    t = gp.GTSampling(db, ["bicycle", "car"], groups, seed=1)                        # labels index the sampler's class_names
    p = t(sample())["lidar_aug"]["paste"]
    assert np.bincount(p["cand_group"], minlength=4).tolist() == [4, 0, 3, 0] and set(p["cand_labels"]) == {0, 1}


def test_pointer_advance_wrap_and_reshuffle():
    db = small_db()
    t = gp.GTSampling(db, NAMES, ["car:3"], seed=5)
    cars = set(db.indices_of("car").tolist())
    assert t.state["car"]["pointer"] == 7                                          # past the end: the first draw shuffles
    a = t(sample())["lidar_aug"]["paste"]["cand_idx"]
    first = t.state["car"]["indices"].copy()
    assert t.state["car"]["pointer"] == 3 and sorted(first) == list(range(7))
    b = t(sample())["lidar_aug"]["paste"]["cand_idx"]
    c = t(sample())["lidar_aug"]["paste"]["cand_idx"]                               # the slice at the end is short
    assert t.state["car"]["pointer"] == 9 and len(c) == 1
    assert np.concatenate([a, b, c]).tolist() == db.indices_of("car")[first].tolist()   # one pass: a permutation
    assert set(np.concatenate([a, b, c]).tolist()) == cars
    d = t(sample())["lidar_aug"]["paste"]["cand_idx"]                               # exhausted: reshuffled, pointer 0 + 3
    assert t.state["car"]["pointer"] == 3 and len(d) == 3
    assert d.tolist() == db.indices_of("car")[t.state["car"]["indices"][:3]].tolist()


def test_same_seed_same_draws_and_own_generator():
    db = small_db()
    runs = []
    for _ in range(2):
        np.random.seed(0)
        t = gp.GTSampling(db, NAMES, ["car:2", "bicycle:2"], seed=123)
        runs.append(np.concatenate([t(sample())["lidar_aug"]["paste"]["cand_idx"] for _ in range(6)]))
        state = np.random.get_state()[1].copy()
        np.random.seed(0)
        assert (np.random.get_state()[1] == state).all()                           # the global generator is not touched
    assert runs[0].tolist() == runs[1].tolist()
    t = gp.GTSampling(db, NAMES, ["car:2", "bicycle:2"], seed=124)
    other = np.concatenate([t(sample())["lidar_aug"]["paste"]["cand_idx"] for _ in range(6)])
    assert other.tolist() != runs[0].tolist()


def test_stop_epoch_identity_and_no_points():
    db = small_db()
    t = gp.GTSampling(db, NAMES, ["car:2"], stop_epoch=3, seed=0)
    assert t.epoch == -1
    t.set_epoch(1)
    assert "paste" in t(sample())["lidar_aug"]
    t.set_epoch(2)                                                                  # epoch + 1 >= stop_epoch
    d = sample()
    keys = set(d)
    assert t(d) is d and set(d) == keys and "lidar_aug" not in d
    t.set_epoch(0)
    d = {"gt_boxes": np.zeros((0, 9), np.float32)}                                  # no points: nothing happens
    assert t(d) is d and "lidar_aug" not in d
    with pytest.raises(NotImplementedError):
        gp.GTSampling(db, NAMES, ["car:2"], use_road_plane=True)
    with pytest.raises(ValueError, match="64|63"):
        gp.GTSampling(db, NAMES, ["car:40", "truck:30"])


def test_filter_by_min_points_at_construction():
    rows = [1, 9, 4, 5, 6, 2, 7, 3, 3, 3]
    db = small_db((7, 3), rows=rows, filter_by_min_points_cfg=["car:5", "bus:9"])
    assert len(db) == 3 + 4 and db.rows.tolist() == [9, 5, 6, 7, 3, 3, 3]           # trucks are not named: unfiltered
    assert db.offsets.tolist() == np.concatenate([[0], np.cumsum(db.rows)]).tolist()
    assert db.points.shape == (db.offsets[-1], 5) and db.boxes[:, 0].tolist() == [10, 30, 40, 60, 70, 80, 90]
    assert float(db.points[0, 0]) == 1 * 5.0                                        # object 1's first row follows object 0's one row
    infos = {"car": [{"box3d_lidar": np.arange(9.0), "num_points_in_gt": 4, "path": "a"},
                     {"box3d_lidar": np.arange(9.0) + 1, "num_points_in_gt": 6, "path": "b"}],
             "truck": [{"box3d_lidar": np.arange(9.0) + 2, "num_points_in_gt": 1, "path": "c"}]}
    load = lambda info: np.full((3, 5), ord(info["path"]), np.float32)
    db2 = gp.ObjectDatabase.from_infos(infos, load, device="cpu", filter_by_min_points_cfg=["car:5"])
    assert db2.class_names == ["car", "truck"] and len(db2) == 2 and db2.boxes.shape == (2, 9)
    assert db2.boxes[:, 0].tolist() == [1.0, 2.0] and float(db2.points[0, 0]) == ord("b")
    assert pickle.loads(pickle.dumps(db2)) is db2                                   # travels by name


def test_paste_record_contents():
    db = small_db()
    t = gp.GTSampling(db, NAMES, ["car:2", "truck:1"], remove_extra_width=(0.2, 0.1, 0.0), seed=3)
    d = sample(n_car=2)
    d["gt_boxes"][:, 0] = [5.0, 6.0]
    boxes0, pts0 = d["gt_boxes"].copy(), d["points"].copy()
    d = ip.CollectLidarSweeps()(dict(d, info={"sweep_lidar_infos": [], "lidar_to_ego": np.eye(4),
                                              "ego_to_global": np.eye(4), "timestamp": 0}))
    d = t(d)
    p = d["lidar_aug"]["paste"]
    assert set(p) >= {"database", "cand_idx", "cand_group", "cand_labels", "gt_boxes", "remove_extra_width"}
    assert p["database"] is db and p["cand_idx"].dtype == np.int64 and len(p["cand_idx"]) == 3
    assert p["cand_group"].tolist() == [0, 0, 1] and p["remove_extra_width"] == (0.2, 0.1, 0.0)
    np.testing.assert_array_equal(p["gt_boxes"], boxes0)
    assert p["gt_boxes"] is not d["gt_boxes"]
    np.testing.assert_array_equal(d["gt_boxes"], boxes0)                            # neither boxes nor points change
    np.testing.assert_array_equal(d["points"], pts0)
    np.random.seed(0)
    d = ip.BevAffineTransformation(rot_lim=(-45.0, 45.0), scale_lim=(0.9, 1.1), trans_lim=(0.5, 0.5, 0.5),
                                   flip_dx_ratio=0.5, flip_dy_ratio=0.5)(d)
    np.testing.assert_array_equal(p["gt_boxes"], boxes0)                            # the record keeps the pre-BDA boxes
    assert len(d["lidar_aug"]["bda_params"]) == 4
    with pytest.raises(ValueError, match="before"):                                 # after the BDA: refused
        t(d)


def test_more_than_64_segments_is_a_value_error_naming_the_numbers():
    db = small_db((40, 3, 5))
    cs = [np.zeros((2, 5), np.float32)] * 10
    aug = {"segments": [2] * 10, "sweep_mats": np.stack([np.eye(4)] * 9), "time_lags": np.zeros(9, np.float32),
           "bda_mat": None, "range": None,
           "paste": {"database": db, "cand_idx": np.arange(55), "cand_group": np.zeros(55, np.int32),
                     "gt_boxes": np.zeros((0, 7), np.float32), "remove_extra_width": (0, 0, 0)}}
    with pytest.raises(ValueError, match=r"1 key frame \+ 9 sweeps \+ 55 candidates = 65"):
        gp._paste_plan([([2] * 10, *lp._plan_segments(cs, aug, 5))], [aug["paste"]], 5)
    with pytest.raises(ValueError, match="64 candidates"):
        gp.check_segments(0, 64)
    gp.check_segments(9, 54)                                                        # 64 segments: fine
    with pytest.raises(ValueError, match="columns"):                                # the database's D must be the scene's
        gp._paste_plan([([2], [None], [False], [np.nan], None, None)],
                       [dict(aug["paste"], cand_idx=np.arange(2), cand_group=np.zeros(2, np.int32))], 4)


def test_append_pasted_boxes_go_through_bda_and_range():
    db = small_db()
    d = sample(n_car=2)
    mat = ip.bev_transform_matrix(30.0, 1.05, (0.1, 0.2, 0.0), True, False)
    d["lidar_aug"] = {"bda_mat": mat, "bda_params": (30.0, 1.05, True, False),
                      "range": np.array(ref.PCR, np.float32),
                      "paste": {"database": db, "cand_idx": np.array([1, 9, 3]), "cand_labels": np.array([0, 1, 0]),
                                "accept": np.array([True, True, False])}}
    out = gp.append_pasted(d)
    want = ip.bda_boxes(db.boxes[[1, 9]], mat, 30.0, 1.05, True, False)              # 9: x = 90 m, outside the range
    mask = ip.boxes_in_range_mask(want, ref.PCR)
    assert mask.tolist() == [True, False]
    np.testing.assert_array_equal(out["gt_boxes"], np.concatenate([d["gt_boxes"], want[mask]]))
    assert out["gt_labels"].tolist() == [0, 0, 0] and out is not d and len(d["gt_boxes"]) == 2
    assert gp.append_pasted(sample()) is not None and "lidar_aug" not in gp.append_pasted(sample())


def test_new_prototypes_parse_through_the_derived_ctypes_path(hip_lib):
    from unidistill_amd import _lib
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    sigs = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert sigs["ud_gt_paste_select"] == (I, [P] * 7 + [I, P, L, P])
    plan = [P, L, I, P, P, I, I, P, P, P, P]
    paste = [P, P, P, P, P, L]
    assert sigs["ud_lidar_paste_count"] == (I, plan + paste + [P, P, ctypes.c_size_t, P])
    assert sigs["ud_lidar_paste_compact"] == (I, plan + paste + [P, P, L, I, P, L, P, ctypes.c_size_t, P])
    for name in ("ud_gt_paste_select", "ud_lidar_paste_count", "ud_lidar_paste_compact"):
        assert list(getattr(hip_lib, name).argtypes) == sigs[name][1]
    # host validation: nothing is launched for these (no device pointer is dereferenced)
    i64 = lambda v: np.ascontiguousarray(np.asarray(v, np.int64))
    fake = 1 << 40
    off = i64([0, 64])
    assert hip_lib.ud_gt_paste_select(fake, i64([0, 0]).ctypes.data, fake, fake, fake, off.ctypes.data, fake, 1, fake, 64,
                                      None) == -1                                  # Nc > 63
    many = 65
    assert hip_lib.ud_lidar_paste_count(None, 0, 5, i64(np.zeros(many + 1)).ctypes.data, i64([0, many]).ctypes.data, many,
                                        1, fake, fake, fake, fake, fake, fake, i64([0, 0]).ctypes.data, fake, fake, 0,
                                        fake, None, 0, None) == -1                 # more than 64 segments
    assert hip_lib.ud_gt_paste_select(None, None, None, None, None, None, None, 0, None, 0, None) == 0


def test_generators_stay_inside_the_caps_of_the_gpu_tests():
    """The committed seeds: no pair of the selection case is within PAIR_MARGIN of touching (cap 2 %), the case holds
    the three situations the rule is about, and the chain cases' near rows stay below 1 %."""
    case = ref.selection_case()
    assert [(len(c), len(g)) for c, _, g in case] == [(0, 5), (40, 0), (63, 50)]
    assert [len(set(grp.tolist())) for _, grp, _ in case] == [0, 10, 3]
    intra = cross_only = False
    for cand, grp, gt in case:
        share = ref.near_pair_share(cand, gt)
        print("near-touching pair share", share)
        assert share <= 0.02
        acc, _ = ref.select(cand, grp, gt)
        g1, g2 = ref.gaps(cand, gt)
        for i in range(len(cand)):
            same = grp == grp[i]
            hit_scene = (g1[i] < 0).any()
            intra |= bool((g2[i][same] < 0).any())
            if not hit_scene and not (g2[i][same] < 0).any() and not acc[i] and np.isfinite(cand[i]).all():
                assert (g2[i][acc & (grp < grp[i])] < 0).any()                     # rejected by an ACCEPTED earlier one only
                cross_only = True
    assert intra and cross_only
    assert np.isnan(case[1][0]).any() and not ref.select(*case[1][:2], case[1][2])[0][17]
    assert 5 < ref.select(*case[2][:2], case[2][2])[0].sum() < 63


def test_chain_cases_stay_inside_the_row_cap_and_cover_their_situations():
    (pts, off, boxes, ids), cases = ref.chain_cases()
    margs, _ = ref.bda_setup()
    mat = ip.bev_transform_matrix(*margs)
    assert sorted(set(np.diff(off).tolist())) == [1, 5, 300]
    seen = set()
    for name, smps in cases.items():
        for on in (False, True):
            near_rows = rows = removed = 0
            for s in smps:
                seen.add(sum(len(c) for c in s["clouds"]))
                aug = dict(s["aug"], bda_mat=mat if on else None, range=ref.PCR if on else None)
                p = s["paste"]
                acc = ref.select(boxes[p["cand_idx"], :7], p["cand_group"], p["gt_boxes"])[0] if p is not None else []
                r, keep, near = ref.chain(s["clouds"], aug, pts, off, boxes, p, acc)
                near_rows, rows = near_rows + int(near.sum()), rows + len(r)
                removed += int((~keep & (r[:, 3] < 100000)).sum())
                if p is not None and len(p["cand_idx"]):
                    assert ref.near_pair_share(boxes[p["cand_idx"], :7], p["gt_boxes"]) == 0.0
            print(name, on, "near rows", near_rows, "of", rows, "scene rows removed", removed)
            assert near_rows <= 0.01 * rows
            assert (removed > 0) == (name in ("mixed", "extra_width"))
    assert seen == {255, 256, 257, 775}                                             # tile - 1, tile, tile + 1, 3 tile + 7
