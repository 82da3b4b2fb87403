"""CPU: the numpy restatement of the nuScenes detection metric (tests/nus_eval_reference.py) on hand-worked cases, the
evaluator's host helpers against it, and the evaluator's argument checks that need no GPU."""
import math

import numpy as np
import pytest

import nus_eval_reference as R

CAR, TRUCK, BUS, BARRIER, MOTO, BIKE, PED, CONE = 0, 1, 3, 5, 6, 7, 8, 9


def boxes(rows, pred=False):
    """rows: (sample, cls, x, y, [score], **extra) -> column dict.  Defaults: size 2 x 4 x 1.5, yaw 0, velocity 0,
    attr 'vehicle.parked' (id 6), num_pts 5."""
    cols = {k: [] for k in ("translation", "size", "yaw", "velocity", "cls", "attr", "sample", "num_pts", "score")}
    for r in rows:
        s, c, x, y = r[:4]
        ex = r[-1] if isinstance(r[-1], dict) else {}
        cols["sample"].append(s)
        cols["cls"].append(c)
        cols["translation"].append([x, y, 0.5])
        cols["size"].append(ex.get("size", [2.0, 4.0, 1.5]))
        cols["yaw"].append(ex.get("yaw", 0.0))
        cols["velocity"].append(ex.get("vel", [0.0, 0.0]))
        cols["attr"].append(ex.get("attr", 6))
        cols["num_pts"].append(-1 if pred else ex.get("num_pts", 5))
        cols["score"].append(r[4] if pred else 0.0)
    out = {k: np.asarray(v, dtype=np.float64 if k in ("translation", "size", "yaw", "velocity", "score") else np.int64)
           for k, v in cols.items()}
    out["translation"] = out["translation"].reshape(-1, 3)
    out["size"] = out["size"].reshape(-1, 3)
    out["velocity"] = out["velocity"].reshape(-1, 2)
    if not pred:
        del out["score"]
    return out


def ego(S):
    return np.zeros((S, 3))


# every case: (gt rows, pred rows, number of samples); reused by tests/test_nus_eval_gpu.py
def case_perfect():
    g, p = [], []
    for c in range(10):
        attr = -1 if c in (BARRIER, CONE) else (4 if c == PED else 6)
        g.append((0, c, 3.0 * c, 1.0, {"attr": attr}))
        p.append((0, c, 3.0 * c, 1.0, 0.9, {"attr": attr}))
    return g, p, 1


def case_all_fp():
    return [(0, CAR, 0.0, 0.0), (1, PED, 5.0, 5.0, {"attr": 4})], [(0, CAR, 10.0, 0.0, 0.8),
                                                                 (1, PED, 5.0, 10.0, 0.7, {"attr": 4})], 2


def case_no_gt_class():
    return [(0, CAR, 0.0, 0.0)], [(0, CAR, 0.1, 0.0, 0.9), (0, BUS, 3.0, 3.0, 0.8)], 1


def case_4m_not_2m():
    return [(0, CAR, 0.0, 0.0)], [(0, CAR, 3.0, 0.0, 0.9)], 1


def case_competing():
    return [(0, CAR, 0.0, 0.0)], [(0, CAR, 1.5, 0.0, 0.9), (0, CAR, 0.3, 0.0, 0.8)], 1


def case_barrier_period():
    return ([(0, BARRIER, 0.0, 0.0, {"yaw": 0.0, "attr": -1}), (0, CAR, 10.0, 0.0, {"yaw": 0.0})],
            [(0, BARRIER, 0.1, 0.0, 0.9, {"yaw": math.pi, "attr": -1}), (0, CAR, 10.1, 0.0, 0.9, {"yaw": math.pi})], 1)


def case_nan_velocity_empty_attr():
    return ([(0, CAR, 0.0, 0.0, {"vel": [math.nan, math.nan], "attr": -1}), (0, CAR, 10.0, 0.0, {"vel": [1.0, 0.0]}),
             (0, PED, 0.0, 5.0, {"vel": [math.nan, math.nan], "attr": -1})],
            [(0, CAR, 0.1, 0.0, 0.9, {"vel": [0.5, 0.0]}), (0, CAR, 10.2, 0.0, 0.8, {"vel": [0.5, 0.0]}),
             (0, PED, 0.1, 5.0, 0.7, {"vel": [0.0, 0.0], "attr": 4})], 1)


def case_repeated_recall():
    g = [(0, CAR, 0.0, 0.0), (0, CAR, 10.0, 0.0), (0, CAR, 20.0, 0.0)]
    p = [(0, CAR, 0.1, 0.0, 0.9), (0, CAR, 30.0, 0.0, 0.8), (0, CAR, 35.0, 5.0, 0.7), (0, CAR, 10.1, 0.0, 0.6),
         (0, CAR, 40.0, 0.0, 0.5), (0, CAR, 20.3, 0.0, 0.4)]
    return g, p, 1


def case_ties():
    g = [(0, CAR, 0.0, 0.0), (1, CAR, 0.0, 0.0)]
    p = [(0, CAR, 0.1, 0.0, 0.5), (0, CAR, 0.2, 0.0, 0.5), (1, CAR, 0.3, 0.0, 0.5), (1, CAR, 9.0, 0.0, 0.5)]
    return g, p, 2


def case_filters():
    g = [(0, CAR, 49.9, 0.0), (0, CAR, 50.1, 0.0), (0, PED, 0.0, 39.9, {"attr": 4}), (0, PED, 0.0, 40.0, {"attr": 4}),
         (0, CAR, -5.0, 0.0, {"num_pts": 0}), (0, CONE, 0.0, -29.0, {"attr": -1})]
    p = [(0, CAR, 49.8, 0.0, 0.9), (0, CAR, 50.2, 0.0, 0.95), (0, PED, 0.0, 39.8, 0.5, {"attr": 4}),
         (0, CAR, -5.1, 0.0, 0.6), (0, CONE, 0.0, -29.5, 0.4, {"attr": -1}), (0, CONE, 0.0, -30.5, 0.99, {"attr": -1})]
    return g, p, 1


CASES = {n[5:]: f for n, f in dict(globals()).items() if n.startswith("case_")}


def run(case):
    g, p, S = case()
    return R.evaluate(boxes(g), boxes(p, pred=True), ego(S))


def test_perfect_detector():
    summ, _, _ = run(case_perfect)
    assert all(abs(v - 1.0) < 1e-12 for d in summ["label_aps"].values() for v in d.values())
    for n, d in summ["label_tp_errors"].items():
        for m, v in d.items():
            nan_expected = (n == "traffic_cone" and m in ("attr_err", "vel_err", "orient_err")) or \
                (n == "barrier" and m in ("attr_err", "vel_err"))
            assert math.isnan(v) if nan_expected else v == 0.0, (n, m, v)
    assert abs(summ["mean_ap"] - 1.0) < 1e-12 and abs(summ["nd_score"] - 1.0) < 1e-12


def test_all_false_positives():
    summ, detail, _ = run(case_all_fp)
    assert summ["mean_ap"] == 0.0
    assert summ["label_tp_errors"]["car"]["trans_err"] == 1.0 and summ["label_tp_errors"]["pedestrian"]["attr_err"] == 1.0
    assert detail["car"]["tp"].sum() == 0


def test_class_without_gt_is_no_predictions():
    summ, detail, md = run(case_no_gt_class)
    assert detail["bus"]["npos"] == 0 and len(detail["bus"]["order"]) == 1
    assert summ["mean_dist_aps"]["bus"] == 0.0 and not md["bus"][2.0]["confidence"].any()
    assert summ["label_tp_errors"]["bus"]["trans_err"] == 1.0
    assert abs(summ["mean_dist_aps"]["car"] - 1.0) < 1e-12


def test_match_at_4m_not_2m():
    summ, detail, _ = run(case_4m_not_2m)
    assert detail["car"]["tp"][:, 0].tolist() == [0, 0, 0, 1]
    aps = summ["label_aps"]["car"]
    assert aps[0.5] == aps[1.0] == aps[2.0] == 0.0 and abs(aps[4.0] - 1.0) < 1e-12
    assert summ["label_tp_errors"]["car"]["trans_err"] == 1.0


def test_competing_predictions_greedy_by_score():
    _, detail, md = run(case_competing)
    # at 0.5 m the 0.9 prediction (1.5 m away) finds the GT as its nearest but fails the threshold; the 0.8 one matches
    assert detail["car"]["tp"].tolist() == [[0, 1], [0, 1], [1, 0], [1, 0]]
    assert detail["car"]["match_gt"].tolist() == [0, -1]
    assert md["car"][2.0]["trans_err"][0] == 1.5


def test_barrier_period_pi_and_nan_classes():
    summ, _, md = run(case_barrier_period)
    assert abs(md["barrier"][2.0]["orient_err"][0]) < 1e-15
    assert abs(md["car"][2.0]["orient_err"][0] - math.pi) < 1e-15
    assert math.isnan(summ["label_tp_errors"]["barrier"]["vel_err"]) and \
        not math.isnan(summ["label_tp_errors"]["barrier"]["orient_err"])
    assert math.isnan(summ["label_tp_errors"]["traffic_cone"]["orient_err"])


def test_nan_velocity_and_empty_attribute_cummean():
    _, _, md = run(case_nan_velocity_empty_attr)
    np.testing.assert_array_equal(R.cummean(np.array([np.nan, 0.5])), [0.0, 0.5])
    np.testing.assert_array_equal(R.cummean(np.array([np.nan, np.nan])), [1.0, 1.0])
    car = md["car"][2.0]
    assert car["vel_err"][0] == 0.0 and car["vel_err"][100] == 0.5          # cummean [0 (NaN only), 0.5]
    assert car["attr_err"][100] == 0.0                                        # [NaN, 0] -> [0, 0]
    np.testing.assert_array_equal(md["pedestrian"][2.0]["vel_err"], np.ones(101))   # all NaN -> ones
    assert md["pedestrian"][2.0]["attr_err"][0] == 1.0


def test_interp_repeated_abscissae():
    np.testing.assert_array_equal(np.interp([0.5, 0.25], [0, .5, .5, .5, 1], [1, 2, 3, 4, 5]), [4, 1.5])
    _, detail, md = run(case_repeated_recall)
    assert detail["car"]["tp"][2].tolist() == [1, 0, 0, 1, 0, 1]
    rec = np.cumsum(detail["car"]["tp"][2]) / 3.0
    assert len(set(rec)) < len(rec)
    prec = md["car"][2.0]["precision"]
    assert prec[33] == 1.0 and prec[34] < prec[33] and prec[100] == 0.5


def test_tie_order():
    _, detail, _ = run(case_ties)
    # all four scores equal: a later sample first, within a sample a later box first
    assert detail["car"]["order"].tolist() == [3, 2, 1, 0]
    assert detail["car"]["match_gt"].tolist() == [-1, 1, 0, -1]


@pytest.mark.parametrize("name,speed,expect", [
    ("car", 0.2, "vehicle.parked"), ("car", 0.2001, "vehicle.moving"), ("bus", 0.2, "vehicle.stopped"),
    ("bus", 0.21, "vehicle.moving"), ("pedestrian", 0.2, "pedestrian.standing"), ("pedestrian", 0.3, "pedestrian.moving"),
    ("bicycle", 0.1, "cycle.without_rider"), ("bicycle", 0.3, "cycle.with_rider"), ("barrier", 5.0, ""),
    ("pedestrian", math.nan, "pedestrian.standing"), ("car", math.nan, "vehicle.parked")])
def test_attribute_threshold(name, speed, expect):
    assert R.attribute_name(name, [speed, 0.0]) == expect


def test_class_range_and_num_pts_filters():
    g, p, S = case_filters()
    gt, pr = boxes(g), boxes(p, pred=True)
    assert R.keep_mask(gt, ego(S)).tolist() == [True, False, True, False, False, True]
    assert R.keep_mask(pr, ego(S)).tolist() == [True, False, True, True, True, False]
    _, detail, _ = R.evaluate(gt, pr, ego(S))
    assert detail["car"]["npos"] == 1 and detail["car"]["order"].tolist() == [0, 3]
    assert detail["car"]["tp"][2].tolist() == [1, 0]


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _qrot(q, v):
    r = _qmul(_qmul(q, np.r_[0.0, v]), q * np.array([1, -1, -1, -1]))
    return r[1:]


def _qmat(q):
    return np.stack([_qrot(q, e) for e in np.eye(3)], 1)


def test_frame_conversion_against_quaternion_product():
    rng = np.random.default_rng(3)
    for _ in range(20):
        q_cs, q_pose = (q / np.linalg.norm(q) for q in rng.standard_normal((2, 4)))
        t_cs, t_pose = rng.standard_normal(3), rng.standard_normal(3) * 100
        box = np.r_[rng.uniform(-50, 50, 3), rng.uniform(0.5, 5, 3), rng.uniform(-4, 4), rng.standard_normal(2)]
        l2g = np.eye(4)
        l2g[:3, :3] = _qmat(q_pose) @ _qmat(q_cs)
        l2g[:3, 3] = _qmat(q_pose) @ t_cs + t_pose
        t, wlh, yaw, v = R.pred_to_global(box, l2g)
        # devkit Box: rotate(q_cs), translate(t_cs), rotate(q_pose), translate(t_pose); yaw = quaternion_yaw
        c = _qrot(q_pose, _qrot(q_cs, box[:3]) + t_cs) + t_pose
        q = _qmul(q_pose, _qmul(q_cs, np.array([math.cos(box[6] / 2), 0, 0, math.sin(box[6] / 2)])))
        d = _qrot(q, np.array([1.0, 0, 0]))
        vel = _qrot(q_pose, _qrot(q_cs, np.r_[box[7:9], 0.0]))
        np.testing.assert_allclose(t, c, rtol=0, atol=1e-9)
        assert wlh == [box[4], box[3], box[5]]
        assert abs(math.remainder(yaw - math.atan2(d[1], d[0]), 2 * math.pi)) < 1e-12
        np.testing.assert_allclose(v, vel[:2], rtol=0, atol=1e-12)


def test_package_host_helpers_match_oracle():
    """evaluation.boxes_to_global / summarize (host code of the package) equal the oracle."""
    from unidistill_amd import evaluation as E
    rng = np.random.default_rng(5)
    M = np.eye(4)
    M[:3, :3] = _qmat(rng.standard_normal(4) / 2.0 / np.linalg.norm(rng.standard_normal(4) / 2.0))
    M[:3, :3] = np.linalg.qr(M[:3, :3])[0]
    M[:3, 3] = rng.standard_normal(3)
    bx = np.concatenate([rng.uniform(-40, 40, (6, 3)), rng.uniform(1, 3, (6, 3)), rng.uniform(-3, 3, (6, 1)),
                         rng.standard_normal((6, 2))], 1).astype(np.float32)
    t, wlh, yaw, vel = E.boxes_to_global(bx, M)
    for i in range(6):
        rt, rw, ry, rv = R.pred_to_global(bx[i], M)
        assert t[i].tolist() == rt and wlh[i].tolist() == rw and vel[i].tolist() == rv
        assert abs(yaw[i] - ry) < 1e-15
    moving, still = E.attribute_tables(E.CLASS_NAMES)
    for c, n in enumerate(E.CLASS_NAMES):
        assert E.attr_id(R.attribute_name(n, [1.0, 0.0])) == moving[c]
        assert E.attr_id(R.attribute_name(n, [0.0, 0.0])) == still[c]
    assert E.CLASS_NAMES == R.CLASS_NAMES and E.ATTRIBUTE_NAMES == R.ATTRIBUTE_NAMES
    assert {k: v for k, v in E.DETECTION_CVPR_2019.items() if k != "dist_fcn"} == R.CFG
    for case in CASES.values():
        summ, _, md = run(case)
        prec = np.stack([[md[n][th]["precision"] for th in R.CFG["dist_ths"]] for n in R.CLASS_NAMES])
        conf = np.stack([[md[n][th]["confidence"] for th in R.CFG["dist_ths"]] for n in R.CLASS_NAMES])
        err = np.stack([[md[n][2.0][m] for m in R.TP_METRICS] for n in R.CLASS_NAMES])
        got = E.summarize(prec, conf, err, E.CLASS_NAMES, E.DETECTION_CVPR_2019)
        assert got["mean_ap"] == summ["mean_ap"] and got["nd_score"] == summ["nd_score"]
        assert got["label_aps"] == summ["label_aps"]


def test_gt_from_infos():
    from unidistill_amd import evaluation as E
    car_from_global = np.eye(4)
    car_from_global[:3, 3] = [-100.0, -200.0, 0.0]          # the car sits at (100, 200) in the global frame
    ref_from_car = np.eye(4)
    ref_from_car[:3, 3] = [0.0, 0.0, -1.8]
    info = {"gt_boxes": np.array([[1, 2, 0, 4, 2, 1.5, 0.3, 1, 0], [0, 0, 0, 1, 1, 1, 0, 0, 0]], np.float64),
            "gt_names": np.array(["car", "ignore"]), "num_lidar_pts": np.array([3, 0]),
            "num_radar_pts": np.array([1, 0]), "car_from_global": car_from_global, "ref_from_car": ref_from_car}
    out = E.gt_from_infos([info, info])
    assert out["cls"].tolist() == [0, 0] and out["sample"].tolist() == [0, 1] and out["attr"].tolist() == [-1, -1]
    assert out["num_pts"].tolist() == [4, 4]
    np.testing.assert_allclose(out["translation"][0], [101, 202, 1.8])
    np.testing.assert_allclose(out["size"][0], [2, 4, 1.5])
    np.testing.assert_allclose(out["ego_translation"][0], [100, 200, 0])


def test_evaluator_argument_checks():
    from unidistill_amd import evaluation as E
    with pytest.raises(RuntimeError, match="GPU only"):
        E.NuScenesDetectionEval(device="cpu")
    with pytest.raises(ValueError, match="no range"):
        E.NuScenesDetectionEval(class_names=["car", "tram"], device="cpu")
    with pytest.raises(ValueError, match="dist_th_tp"):
        E.NuScenesDetectionEval(cfg=dict(E.DETECTION_CVPR_2019, dist_th_tp=3.0), device="cpu")
    with pytest.raises(ValueError, match="max_boxes_per_sample"):
        E.NuScenesDetectionEval(cfg=dict(E.DETECTION_CVPR_2019, max_boxes_per_sample=5000), device="cpu")


def test_oracle_against_devkit():
    """When the nuScenes devkit is importable, its accumulate / calc_ap / calc_tp agree with the oracle."""
    nuscenes = pytest.importorskip("nuscenes", reason="nuScenes devkit not installed: oracle-vs-devkit check skipped")
    from nuscenes.eval.common.data_classes import EvalBoxes
    from nuscenes.eval.common.utils import center_distance
    from nuscenes.eval.detection.algo import accumulate, calc_ap, calc_tp
    from nuscenes.eval.detection.data_classes import DetectionBox
    del nuscenes
    g, p, S = case_repeated_recall()
    gt, pr = boxes(g), boxes(p, pred=True)

    def to_eval(b, pred):
        eb = EvalBoxes()
        for s in range(S):
            rows = [i for i in range(len(b["cls"])) if b["sample"][i] == s]
            eb.add_boxes(str(s), [DetectionBox(
                sample_token=str(s), translation=tuple(b["translation"][i]), size=tuple(b["size"][i]),
                rotation=(math.cos(b["yaw"][i] / 2), 0, 0, math.sin(b["yaw"][i] / 2)),
                velocity=tuple(b["velocity"][i]), detection_name=R.CLASS_NAMES[b["cls"][i]],
                detection_score=float(b["score"][i]) if pred else -1.0,
                attribute_name=R.ATTRIBUTE_NAMES[b["attr"][i]] if b["attr"][i] >= 0 else "") for i in rows])
        return eb
    _, _, md = R.evaluate(gt, pr, ego(S))
    dk = accumulate(to_eval(gt, False), to_eval(pr, True), "car", center_distance, 2.0)
    np.testing.assert_allclose(dk.precision, md["car"][2.0]["precision"], rtol=0, atol=1e-12)
    assert abs(calc_ap(dk, 0.1, 0.1) - R.calc_ap(md["car"][2.0], 0.1, 0.1)) < 1e-12
    assert abs(calc_tp(dk, 0.1, "trans_err") - R.calc_tp(md["car"][2.0], 0.1, "trans_err")) < 1e-12
