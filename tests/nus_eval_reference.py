"""numpy restatement of the nuScenes devkit's detection metric (DetectionEval, config detection_cvpr_2019) and of the
reference's prediction conversion (eval_utils.box3d_to_nuscenesbox), in float64.  The devkit is not installed; this
file is the specification the kernels of csrc/nus_eval.hip are tested against.

Boxes are plain arrays.  GT: translation [G, 3], size wlh [G, 3], yaw [G], velocity [G, 2], cls [G], attr [G] (-1 = ''),
num_pts [G], sample [G], keep [G]; predictions: the same columns plus score [P] (num_pts -1), in (sample, box) order.

Deliberate choices, shared with the kernels:
  * ties of equal score: np.argsort(conf, kind="stable")[::-1] over the (sample, box) list (the devkit's unstable sort
    over a queue-dependent sample order has no reproducible tie order);
  * distances are sqrt(dx * dx + dy * dy) in plain float64 arithmetic (the devkit's np.linalg.norm of a 2-vector);
  * bike-rack filtering (needs the map) is replaced by the caller's keep mask.
"""
import math

import numpy as np

CLASS_NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle",
               "pedestrian", "traffic_cone"]
ATTRIBUTE_NAMES = ["cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.sitting_lying_down",
                   "pedestrian.standing", "vehicle.moving", "vehicle.parked", "vehicle.stopped"]
TP_METRICS = ["trans_err", "scale_err", "orient_err", "vel_err", "attr_err"]
DefaultAttribute = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
                    "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
                    "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
                    "traffic_cone": ""}
CFG = {"class_range": {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
                       "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30},
       "dist_ths": [0.5, 1.0, 2.0, 4.0], "dist_th_tp": 2.0, "min_recall": 0.1, "min_precision": 0.1,
       "max_boxes_per_sample": 500, "mean_ap_weight": 5}


# ---- eval_utils.box3d_to_nuscenesbox -------------------------------------------------------------------------------
def attribute_name(name, velocity):
    if math.sqrt(velocity[0] ** 2 + velocity[1] ** 2) > 0.2:
        if name in ["car", "construction_vehicle", "bus", "truck", "trailer"]:
            return "vehicle.moving"
        if name in ["bicycle", "motorcycle"]:
            return "cycle.with_rider"
        return DefaultAttribute[name]
    if name in ["pedestrian"]:
        return "pedestrian.standing"
    if name in ["bus"]:
        return "vehicle.stopped"
    return DefaultAttribute[name]


def pred_to_global(box, l2g):
    """One LiDAR-frame box [x y z dx dy dz rot (vx vy)] through the LiDAR -> global matrix [4, 4]:
    (translation, wlh, yaw, velocity[2])."""
    M = np.asarray(l2g, dtype=np.float64)
    b = [float(v) for v in box]
    x, y, z, rot = b[0], b[1], b[2], b[6]
    t = [M[r, 0] * x + M[r, 1] * y + M[r, 2] * z + M[r, 3] for r in range(3)]
    wlh = [b[4], b[3], b[5]]
    c, s = math.cos(rot), math.sin(rot)
    yaw = math.atan2(M[1, 0] * c + M[1, 1] * s, M[0, 0] * c + M[0, 1] * s)
    if len(b) >= 9:
        v = [M[0, 0] * b[7] + M[0, 1] * b[8], M[1, 0] * b[7] + M[1, 1] * b[8]]
    else:
        v = [math.nan, math.nan]
    return t, wlh, yaw, v


def preds_from_dicts(pred_dicts, sample_ids, l2g, class_names=CLASS_NAMES):
    """generate_prediction_dicts + box3d_to_nuscenesbox on host copies (labels start at 1) -> prediction arrays."""
    cols = {k: [] for k in ("translation", "size", "yaw", "velocity", "cls", "attr", "score", "sample")}
    for pd, sid, M in zip(pred_dicts, sample_ids, l2g):
        boxes = np.asarray(pd["pred_boxes"], dtype=np.float32)
        for box, score, label in zip(boxes, np.asarray(pd["pred_scores"], np.float32), np.asarray(pd["pred_labels"])):
            name = class_names[int(label) - 1]
            t, wlh, yaw, v = pred_to_global(box, M)
            cols["translation"].append(t)
            cols["size"].append(wlh)
            cols["yaw"].append(yaw)
            cols["velocity"].append(v)
            cols["cls"].append(int(label) - 1)
            a = attribute_name(name, v)
            cols["attr"].append(ATTRIBUTE_NAMES.index(a) if a else -1)
            cols["score"].append(float(score))
            cols["sample"].append(int(sid))
    out = {k: np.asarray(v, dtype=np.float64 if k in ("translation", "size", "yaw", "velocity", "score") else np.int64)
           for k, v in cols.items()}
    out["translation"] = out["translation"].reshape(-1, 3)
    out["size"] = out["size"].reshape(-1, 3)
    out["velocity"] = out["velocity"].reshape(-1, 2)
    return out


def preds_from_arrays(boxes, scores, labels, sample, l2g, class_names=CLASS_NAMES):
    """preds_from_dicts for many boxes at once: the same expressions, elementwise in numpy.  boxes f32 [n, 7 | 9],
    scores f32 [n], labels [n] (starting at 1), sample [n], l2g [S, 4, 4] indexed by sample."""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    M = np.asarray(l2g, dtype=np.float64)[np.asarray(sample)]
    x, y, z, rot = b[:, 0], b[:, 1], b[:, 2], b[:, 6]
    t = np.stack([M[:, r, 0] * x + M[:, r, 1] * y + M[:, r, 2] * z + M[:, r, 3] for r in range(3)], 1)
    c, s = np.cos(rot), np.sin(rot)
    yaw = np.arctan2(M[:, 1, 0] * c + M[:, 1, 1] * s, M[:, 0, 0] * c + M[:, 0, 1] * s)
    if b.shape[1] >= 9:
        v = np.stack([M[:, 0, 0] * b[:, 7] + M[:, 0, 1] * b[:, 8], M[:, 1, 0] * b[:, 7] + M[:, 1, 1] * b[:, 8]], 1)
    else:
        v = np.full((len(b), 2), np.nan)
    cls = np.asarray(labels, dtype=np.int64) - 1
    moving = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2) > 0.2
    table = {(n, m): attribute_name(n, [1.0, 0.0] if m else [0.0, 0.0]) for n in class_names for m in (False, True)}
    attr = np.array([ATTRIBUTE_NAMES.index(a) if a else -1 for a in
                     (table[(class_names[k], bool(m))] for k, m in zip(cls, moving))], dtype=np.int64)
    return {"translation": t, "size": b[:, [4, 3, 5]], "yaw": yaw, "velocity": v, "cls": cls, "attr": attr,
            "score": np.asarray(scores, dtype=np.float32).astype(np.float64), "sample": np.asarray(sample, np.int64)}


# ---- filter_eval_boxes ---------------------------------------------------------------------------------------------
def ego_dist(translation, sample, ego):
    d = translation[:, :2] - ego[sample][:, :2]
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def keep_mask(boxes, ego, class_names=CLASS_NAMES, cfg=CFG):
    rng = np.array([cfg["class_range"][n] for n in class_names], dtype=np.float64)
    keep = ego_dist(boxes["translation"], boxes["sample"], ego) < rng[boxes["cls"]]
    if "num_pts" in boxes:
        keep &= boxes["num_pts"] != 0
    if "keep" in boxes:
        keep &= np.asarray(boxes["keep"], dtype=bool)
    return keep


# ---- algo.accumulate ------------------------------------------------------------------------------------------------
def angle_diff(x, y, period):
    diff = (x - y + period / 2) % period - period / 2
    if diff > math.pi:
        diff = diff - 2 * math.pi
    return diff


def scale_err(a, b):
    mn = [min(a[0], b[0]), min(a[1], b[1]), min(a[2], b[2])]
    va, vr, inter = a[0] * a[1] * a[2], b[0] * b[1] * b[2], mn[0] * mn[1] * mn[2]
    return 1 - inter / (va + vr - inter)


def cummean(x):
    if sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x.astype(float))
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


def sort_order(score):
    """Global order of a (sample, box)-ordered list: descending score, ties a later sample / box first."""
    return np.argsort(score, kind="stable")[::-1]


def match_class(gt, pred, c, ths, tp_th, barrier_c):
    """Greedy matching of one class at every threshold (the devkit runs one threshold per call; matching at one
    threshold never looks at another, so one pass does all).  Returns the sorted prediction indices, tp [T, n] and the
    match data at tp_th: (matched GT index, the five errors, conf) per match, in order."""
    pi = np.nonzero(pred["cls"] == c)[0]
    order = pi[sort_order(pred["score"][pi])]
    gi = np.nonzero(gt["cls"] == c)[0]
    by_sample = {}
    for g in gi:
        by_sample.setdefault(int(gt["sample"][g]), []).append(int(g))
    taken = [set() for _ in ths]
    tp = np.zeros((len(ths), len(order)), dtype=np.int64)
    match_gt = np.full(len(order), -1, dtype=np.int64)
    errs = []
    gx, gy = gt["translation"][:, 0], gt["translation"][:, 1]
    for k, p in enumerate(order):
        px, py = pred["translation"][p, 0], pred["translation"][p, 1]
        cand = by_sample.get(int(pred["sample"][p]), ())
        dists = [math.sqrt((px - gx[g]) * (px - gx[g]) + (py - gy[g]) * (py - gy[g])) for g in cand]
        for w, th in enumerate(ths):
            min_dist, match = np.inf, -1
            for g, d in zip(cand, dists):
                if g not in taken[w] and d < min_dist:
                    min_dist, match = d, g
            if min_dist < th:
                taken[w].add(match)
                tp[w, k] = 1
                if th == tp_th:
                    match_gt[k] = match
                    period = math.pi if c == barrier_c else 2 * math.pi
                    ga = gt["attr"][match]
                    errs.append((min_dist,
                                 scale_err(gt["size"][match], pred["size"][p]),
                                 abs(angle_diff(gt["yaw"][match], pred["yaw"][p], period)),
                                 math.sqrt((pred["velocity"][p, 0] - gt["velocity"][match, 0]) ** 2
                                           + (pred["velocity"][p, 1] - gt["velocity"][match, 1]) ** 2),
                                 math.nan if ga < 0 else 1 - float(ga == pred["attr"][p]),
                                 pred["score"][p]))
    return order, tp, match_gt, errs, len(gi)


def no_predictions():
    return {"precision": np.zeros(101), "confidence": np.zeros(101),
            **{m: np.ones(101) for m in TP_METRICS}}


def curves(tp_row, conf, npos, errs=None):
    """accumulate's tail for one (class, threshold): tp flags in sorted order -> metric data."""
    if npos == 0 or tp_row.sum() == 0:
        return no_predictions()
    tp = np.cumsum(tp_row).astype(float)
    fp = np.cumsum(1 - tp_row).astype(float)
    prec = tp / (fp + tp)
    rec = tp / float(npos)
    rec_interp = np.linspace(0, 1, 101)
    prec = np.interp(rec_interp, rec, prec, right=0)
    conf = np.interp(rec_interp, rec, conf, right=0)
    md = {"precision": prec, "confidence": conf}
    if errs is not None:
        match_conf = np.array([e[5] for e in errs])
        for m, name in enumerate(TP_METRICS):
            tmp = cummean(np.array([e[m] for e in errs]))
            md[name] = np.interp(conf[::-1], match_conf[::-1], tmp[::-1])[::-1]
    return md


def max_recall_ind(md):
    nz = np.nonzero(md["confidence"])[0]
    return int(nz[-1]) if len(nz) else 0


def calc_ap(md, min_recall, min_precision):
    # prec[round(100 * min_recall) + 1:] is prec[11:] at min_recall 0.1 (the devkit's slice, which calc_tp's first
    # index 11 matches), not prec[12:]
    prec = np.copy(md["precision"])
    prec = prec[round(100 * min_recall) + 1:]
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(md, min_recall, metric_name):
    first_ind = round(100 * min_recall) + 1
    last_ind = max_recall_ind(md)
    if last_ind < first_ind:
        return 1.0
    return float(np.mean(md[metric_name][first_ind: last_ind + 1]))


def evaluate(gt, pred, ego, class_names=CLASS_NAMES, cfg=CFG):
    """-> (metrics_summary without eval_time / cfg, per-class detail: order, tp, match_gt, metric data per threshold).
    gt / pred: dicts of arrays (see the module docstring); ego [S, 3]."""
    ego = np.asarray(ego, dtype=np.float64)
    gk = keep_mask(gt, ego, class_names, cfg)
    pk = keep_mask(pred, ego, class_names, cfg)
    gtf = {k: v[gk] for k, v in gt.items()}
    pf = {k: v[pk] for k, v in pred.items()}
    kept_rows = np.nonzero(pk)[0]
    gt_rows = np.nonzero(gk)[0]
    ths = list(cfg["dist_ths"])
    barrier = class_names.index("barrier") if "barrier" in class_names else -1
    detail, md_all = {}, {}
    for c, name in enumerate(class_names):
        order, tp, match_gt, errs, npos = match_class(gtf, pf, c, ths, cfg["dist_th_tp"], barrier)
        conf = pf["score"][order]
        mds = {th: curves(tp[w], conf, npos, errs if th == cfg["dist_th_tp"] else None) for w, th in enumerate(ths)}
        for th in ths:
            if th != cfg["dist_th_tp"]:
                for m in TP_METRICS:
                    mds[th].setdefault(m, np.ones(101))
        md_all[name] = mds
        detail[name] = {"order": kept_rows[order], "tp": tp, "npos": npos,
                        "match_gt": np.where(match_gt >= 0, gt_rows[np.maximum(match_gt, 0)], -1)}
    label_aps, label_tp = {}, {}
    for name in class_names:
        label_aps[name] = {th: calc_ap(md_all[name][th], cfg["min_recall"], cfg["min_precision"]) for th in ths}
        md = md_all[name][cfg["dist_th_tp"]]
        label_tp[name] = {}
        for m in TP_METRICS:
            if name in ["traffic_cone"] and m in ["attr_err", "vel_err", "orient_err"]:
                label_tp[name][m] = np.nan
            elif name in ["barrier"] and m in ["attr_err", "vel_err"]:
                label_tp[name][m] = np.nan
            else:
                label_tp[name][m] = calc_tp(md, cfg["min_recall"], m)
    mean_dist_aps = {n: float(np.mean(list(d.values()))) for n, d in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = {m: float(np.nanmean([label_tp[n][m] for n in class_names])) for m in TP_METRICS}
    tp_scores = {m: max(0.0, 1.0 - tp_errors[m]) for m in TP_METRICS}
    nd = float(cfg["mean_ap_weight"] * mean_ap + np.sum(list(tp_scores.values())))
    nd = nd / float(cfg["mean_ap_weight"] + len(tp_scores))
    summary = {"label_aps": label_aps, "mean_dist_aps": mean_dist_aps, "mean_ap": mean_ap, "label_tp_errors": label_tp,
               "tp_errors": tp_errors, "tp_scores": tp_scores, "nd_score": nd}
    return summary, detail, md_all
