"""float64 Python restatement of the tracking metric of DESIGN §2.24 (include/unidistill_hip.h, `ud_track_metric`) and the seeded
generator the tracking-metric tests and tools/time_track_metric.py share.

Plain loops keep the per-scene state; the per-frame assignment is scipy's `linear_sum_assignment` on a matrix whose
inadmissible pairs cost BIG, so nothing here shares code or an algorithm with the kernel's solver (`brute_force_assign` checks
scipy's answer on small problems).  Every float64 operation is its own rounded step: numpy and Python never fuse a multiply with
an add."""
import math

import numpy as np
from scipy.optimize import linear_sum_assignment

ST_NONFINITE, ST_BOXES, ST_RANGE, ST_ID = 1, 2, 4, 8
COUNTS = ("frames", "objects", "matches", "switches", "fp", "miss", "mt", "ml", "frag", "tid", "lgd", "inst")
TRACKING_CLASSES = ("bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck")
CLASS_NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
               "traffic_cone"]
CLASS_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "pedestrian": 40, "motorcycle": 40, "bicycle": 40}
METRIC_WORST = {"amota": 0.0, "amotp": 2.0, "recall": 0.0, "motar": 0.0, "gt": -1, "mota": 0.0, "motp": 2.0, "mt": 0.0,
                "ml": -1, "faf": 500, "tp": 0.0, "fp": -1, "fn": -1, "ids": -1, "frag": -1, "tid": 20, "lgd": 20}
SUMMED = ("mt", "ml", "tp", "fp", "fn", "ids", "frag", "gt")
BIG = 1e4


def default_config(class_names=CLASS_NAMES):
    """-> (tracked flag per class, range per class)."""
    return [n in TRACKING_CLASSES for n in class_names], [float(CLASS_RANGE.get(n, 0.0)) for n in class_names]


def recall_thresholds(min_recall=0.1, num=40):
    return np.round(np.linspace(min_recall, 1.0, num), 12)


def scene_frames_reference(scene, timestamp_us):
    """-> (frame_sample, scene_off): samples grouped by ascending scene value, ordered by (timestamp, index)."""
    scene = [int(s) for s in scene]
    ts = [int(t) for t in timestamp_us]
    frame_sample, scene_off = [], [0]
    for sc in sorted(set(scene)):
        frame_sample += [i for _, i in sorted((ts[i], i) for i in range(len(scene)) if scene[i] == sc)]
        scene_off.append(len(frame_sample))
    return frame_sample, scene_off


def assign(D, th):
    """Maximum-cardinality, then minimum-cost matching over the pairs with D < th -> [(row, col), ...] by row."""
    adm = D < th
    if not adm.any():
        return []
    r, c = linear_sum_assignment(np.where(adm, D, BIG))
    return [(int(i), int(j)) for i, j in zip(r, c) if adm[i, j]]


def brute_force_assign(D, th):
    """-> (pairs, cost) of the best matching by enumeration (small problems only)."""
    n, m = D.shape
    best = (0, 0.0)

    def rec(i, used, k, cost):
        nonlocal best
        if i == n:
            if k > best[0] or (k == best[0] and cost < best[1]):
                best = (k, cost)
            return
        rec(i + 1, used, k, cost)
        for j in range(m):
            if j not in used and D[i, j] < th:
                rec(i + 1, used | {j}, k + 1, cost + D[i, j])

    rec(0, frozenset(), 0, 0.0)
    return best


def interp_thresholds(scores_desc, P, recall):
    """The float64 arithmetic of np.interp(recall, rec, s), NaN where the recall is not reached."""
    n = len(scores_desc)
    out = np.full(len(recall), np.nan)
    if n == 0 or P == 0:
        return out
    s = [float(v) for v in scores_desc]
    rec = [float(np.float64(i + 1) / np.float64(P)) for i in range(n)]
    for k, r in enumerate(float(v) for v in recall):
        if r > float(np.float64(n) / np.float64(P)):
            continue
        if r <= rec[0]:
            out[k] = s[0]
            continue
        j = max(i for i in range(n) if rec[i] <= r)
        if rec[j] == r or j == n - 1:
            out[k] = s[j]
        else:
            out[k] = s[j] + ((s[j + 1] - s[j]) / (rec[j + 1] - rec[j])) * (r - rec[j])
    return out


def _walk(frames, theta, th, events):
    """One pass over one scene's frames of one class.  frames: [(frame index, objects [(gt row, instance, x, y)], hypotheses
    [(pred row, id, x, y, score)])] -> (counts dict, dist_sum, match scores); events: dict gt row -> (type, pred row)."""
    m, inst = {}, {}
    cnt = dict.fromkeys(COUNTS, 0)
    dist_sum, scores = 0.0, []
    for fidx, objs, hyps_all in frames:
        hyps = [h for h in hyps_all if theta is None or h[4] >= theta]
        if not objs and not hyps:
            continue
        cnt["frames"] += 1
        cnt["objects"] += len(objs)
        ox, oy = (np.array([o[i] for o in objs], np.float64).reshape(-1, 1) for i in (2, 3))
        hx, hy = (np.array([h[i] for h in hyps], np.float64).reshape(1, -1) for i in (2, 3))
        dx, dy = ox - hx, oy - hy
        D = np.sqrt(dx * dx + dy * dy)            # three rounded steps per entry, as the text has them
        match = [-1] * len(objs)
        claimed = [False] * len(hyps)
        for i, o in enumerate(objs):
            if o[1] in m:
                for j, h in enumerate(hyps):
                    if h[1] == m[o[1]] and not claimed[j] and D[i, j] < th:
                        match[i], claimed[j] = j, True
                        break
        ro = [i for i in range(len(objs)) if match[i] < 0]
        rh = [j for j in range(len(hyps)) if not claimed[j]]
        if ro and rh:
            for a, b in assign(D[np.ix_(ro, rh)], th):
                match[ro[a]], claimed[rh[b]] = rh[b], True
        for i, o in enumerate(objs):
            st = inst.setdefault(o[1], {"app": 0, "trk": 0, "first": fidx, "tid": 0, "run": 0, "maxrun": 0, "frag": 0,
                                        "ever": False, "gap": False})
            st["app"] += 1
            j = match[i]
            kind = 0
            if j >= 0:
                hid = hyps[j][1]
                kind = 2 if (o[1] in m and m[o[1]] != hid) else 1
                m[o[1]] = hid
                cnt["matches" if kind == 1 else "switches"] += 1
                dist_sum = dist_sum + D[i, j]
                if kind == 1:
                    scores.append(hyps[j][4])
                st["trk"] += 1
                if not st["ever"]:
                    st["ever"], st["tid"] = True, fidx - st["first"]
                if st["gap"]:
                    st["frag"] += 1
                    st["gap"] = False
                st["run"] = 0
            else:
                cnt["miss"] += 1
                st["run"] += 1
                st["maxrun"] = max(st["maxrun"], st["run"])
                if st["ever"]:
                    st["gap"] = True
            if events is not None:
                events[o[0]] = (kind, hyps[j][0] if j >= 0 else -1)
        cnt["fp"] += len(hyps) - sum(claimed)
    for st in inst.values():
        ratio = float(np.float64(st["trk"]) / np.float64(st["app"]))
        cnt["mt"] += ratio >= 0.8
        cnt["ml"] += ratio < 0.2
        cnt["frag"] += st["frag"]
        if st["ever"]:
            cnt["tid"] += st["tid"]
            cnt["lgd"] += st["maxrun"]
            cnt["inst"] += 1
    return cnt, dist_sum, scores


def evaluate_reference(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_instance, gt_num_pts, gt_keep, gt_off, ego,
                       scene, timestamp_us, *, tracked, class_range, recall, dist_th_tp=2.0, max_boxes_per_sample=500,
                       events_pass=None, scenes=None):
    """-> dict: counts int64 [T, K + 1, 12], dist_sum / valid [T, K + 1], thresholds [T, K], num_scores [T], status, track_score
    [P] (NaN: not kept), events_type / events_row [G] of `events_pass` ("none" or k).  `scenes`: only the first so many scenes."""
    rec = np.asarray(rec, np.float64)
    gt_xyz = np.asarray(gt_xyz, np.float64).reshape(-1, 3)
    ego = np.asarray(ego, np.float64).reshape(-1, 3)
    recall = np.asarray(recall, np.float64)
    C, K, G, P_rows = len(tracked), len(recall), len(gt_xyz), len(rec)
    slots = [c for c in range(C) if tracked[c]]
    frame_sample, scene_off = scene_frames_reference(scene, timestamp_us)
    NS = len(scene_off) - 1 if scenes is None else min(scenes, len(scene_off) - 1)
    max_scene_rows = max(sum(int(row_count[s]) for s in frame_sample[scene_off[k]:scene_off[k + 1]])
                         for k in range(len(scene_off) - 1))
    status = 0
    track_score = np.full(P_rows, np.nan)
    per = {}                                     # (scene, class slot) -> frames
    for k in range(NS):
        fr = frame_sample[scene_off[k]:scene_off[k + 1]]
        acc, kept_rows = {}, []
        for s in fr:
            nkept = 0
            for row in range(int(row_start[s]), int(row_start[s]) + int(row_count[s])):
                c, tid = int(cls[row]), int(track_id[row])
                if not (tid > 0 and 0 <= c < C and tracked[c]):
                    continue
                x, y, z, score = (float(rec[row, i]) for i in (0, 1, 2, 9))
                if not all(math.isfinite(v) for v in (x, y, z, score)):
                    status |= ST_NONFINITE
                    continue
                dx, dy = x - float(ego[s, 0]), y - float(ego[s, 1])
                if not math.sqrt(dx * dx + dy * dy) <= class_range[c]:
                    continue
                if tid > max_scene_rows:
                    status |= ST_ID
                    continue
                a = acc.setdefault(tid, [0.0, 0])
                a[0] = a[0] + score
                a[1] += 1
                kept_rows.append((row, tid))
                nkept += 1
            if nkept > max_boxes_per_sample:
                status |= ST_BOXES
        for row, tid in kept_rows:
            track_score[row] = float(np.float64(acc[tid][0]) / np.float64(acc[tid][1]))
        for t, c in enumerate(slots):
            frames = []
            for fidx, s in enumerate(fr):
                objs, hyps = [], []
                for g in range(int(gt_off[s]), int(gt_off[s + 1])):
                    if int(gt_cls[g]) != c or not gt_keep[g] or not gt_num_pts[g] > 0:
                        continue
                    x, y, z = (float(v) for v in gt_xyz[g])
                    if not all(math.isfinite(v) for v in (x, y, z)):
                        status |= ST_NONFINITE
                        continue
                    dx, dy = x - float(ego[s, 0]), y - float(ego[s, 1])
                    if math.sqrt(dx * dx + dy * dy) <= class_range[c]:
                        objs.append((g, int(gt_instance[g]), x, y))
                for row in range(int(row_start[s]), int(row_start[s]) + int(row_count[s])):
                    if int(cls[row]) == c and not math.isnan(track_score[row]):
                        hyps.append((row, int(track_id[row]), float(rec[row, 0]), float(rec[row, 1]), float(track_score[row])))
                frames.append((fidx, objs, hyps))
            per[k, t] = frames
    T = len(slots)
    counts = np.zeros((T, K + 1, len(COUNTS)), np.int64)
    dist_sum = np.zeros((T, K + 1))
    valid = np.zeros((T, K + 1), np.int32)
    thresholds = np.full((T, K), np.nan)
    num_scores = np.zeros(T, np.int64)
    ev_type, ev_row = np.full(G, -1, np.int32), np.full(G, -1, np.int32)

    def run(t, theta, p, want):
        events = {} if want else None
        for k in range(NS):
            cnt, d, sc = _walk(per[k, t], theta, dist_th_tp, events)
            counts[t, p] += [cnt[n] for n in COUNTS]
            dist_sum[t, p] = dist_sum[t, p] + d
            if theta is None:
                scores.extend(sc)
        if want:
            for g, (kind, row) in events.items():
                ev_type[g], ev_row[g] = kind, row

    for t in range(T):
        scores = []
        run(t, None, 0, events_pass == "none")
        valid[t, 0] = 1
        s = sorted(scores, reverse=True)
        num_scores[t] = len(s)
        thresholds[t] = interp_thresholds(s, int(counts[t, 0, 1]), recall)
        for k in range(K):
            if not math.isnan(thresholds[t, k]):
                valid[t, k + 1] = 1
                run(t, float(thresholds[t, k]), k + 1, events_pass == k)
    return {"counts": counts, "dist_sum": dist_sum, "valid": valid, "thresholds": thresholds, "num_scores": num_scores,
            "status": status, "track_score": track_score, "events_type": ev_type, "events_row": ev_row}


def pass_metrics(counts, dist_sum, valid, recall, frame_period_s=0.5):
    """One class: counts [K + 1, 12], ... -> {metric: float64 [K]} over the threshold passes (NaN where the pass did not run)."""
    K = len(recall)
    out = {n: np.full(K, np.nan) for n in METRIC_WORST if n not in ("amota", "amotp")}
    for k in range(K):
        if not valid[k + 1]:
            continue
        c = dict(zip(COUNTS, (int(v) for v in counts[k + 1])))
        P = float(c["objects"])
        tp, fp, fn, ids = c["matches"] + c["switches"], c["fp"], c["miss"], c["switches"]
        out["tp"][k], out["fp"][k], out["fn"][k], out["ids"][k], out["gt"][k] = tp, fp, fn, ids, P
        out["recall"][k] = tp / P
        out["mota"][k] = max(0.0, 1.0 - (fn + ids + fp) / P)
        ra = tp / P                               # the recall the pass achieved, as the devkit's motar uses it, not r_k
        out["motar"][k] = max(0.0, 1.0 - (ids + fp + fn - (1.0 - ra) * P) / (ra * P)) if tp else np.nan
        out["motp"][k] = float(dist_sum[k + 1]) / tp if tp else np.nan
        out["faf"][k] = 100.0 * fp / c["frames"]
        out["mt"][k], out["ml"][k], out["frag"][k] = c["mt"], c["ml"], c["frag"]
        out["tid"][k] = c["tid"] / c["inst"] * frame_period_s if c["inst"] else np.nan
        out["lgd"][k] = c["lgd"] / c["inst"] * frame_period_s if c["inst"] else np.nan
    return out


def summarize_reference(out, names, recall, frame_period_s=0.5, metric_worst=METRIC_WORST):
    """names: the tracked classes' names in slot order -> {"label_metrics": {metric: {class: value}}, metric: value}."""
    label = {m: {} for m in metric_worst}
    for t, name in enumerate(names):
        pm = pass_metrics(out["counts"][t], out["dist_sum"][t], out["valid"][t], recall, frame_period_s)
        if np.all(np.isnan(pm["mota"])):
            for m, w in metric_worst.items():
                label[m][name] = float("nan") if w == -1 else float(w)
            continue
        ks = int(np.nanargmax(pm["mota"]))
        label["amota"][name] = float(np.mean(np.where(np.isnan(pm["motar"]), metric_worst["amota"], pm["motar"])))
        label["amotp"][name] = float(np.mean(np.where(np.isnan(pm["motp"]), metric_worst["amotp"], pm["motp"])))
        for m in pm:
            label[m][name] = float(pm[m][ks])
    summary = {"label_metrics": label}
    for m in metric_worst:
        vals = np.array(list(label[m].values()), np.float64)
        if np.all(np.isnan(vals)):
            summary[m] = float("nan")
        else:
            summary[m] = float(np.nansum(vals)) if m in SUMMED else float(np.nanmean(vals))
    return summary


def make_case(seed, num_scenes, num_frames, num_objects, classes, *, spread=45.0, extra_classes=(), empty_frames=(),
              shuffle_samples=False, miss=0.12, switch=0.04, false_pos=3, noise=0.25):
    """Seeded scenes with ground truth and tracked predictions in the evaluator's layout.  Each scene holds `num_objects` objects
    that move at constant velocity and appear and vanish; a detection follows an object with centre noise, is missing now and
    then, changes its track id now and then, and `false_pos` false positives with ids of their own are added per frame, with as
    many rows of each of `extra_classes` (not tracked).  Coordinates and scores are continuous: exact ties have no probability.
    -> dict rec f64 [P, 10], cls i32 [P], track_id i32 [P], row_start, row_count, scene, timestamp_us, ego [S, 3], gt_xyz [G, 3],
    gt_cls, gt_instance (int64, unique over everything), gt_num_pts, gt_keep, gt_sample (ascending), gt_off [S + 1]."""
    rng = np.random.default_rng(seed)
    S = num_scenes * num_frames
    sample_of = rng.permutation(S) if shuffle_samples else np.arange(S)
    scene, ts, ego = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros((S, 3))
    prow, grow = [None] * S, [None] * S
    for sc in range(num_scenes):
        n = num_objects
        oc = rng.choice(np.asarray(classes), n)
        centre = rng.uniform(-500, 500, 2)
        p0 = rng.uniform(-spread, spread, (n, 2)) + centre
        v = rng.normal(0.0, 3.0, (n, 2))
        first = rng.integers(0, max(1, num_frames // 3), n) if num_frames > 2 else np.zeros(n, np.int64)
        last = rng.integers(max(1, 2 * num_frames // 3), num_frames + 1, n) if num_frames > 2 else np.full(n, num_frames)
        tid = np.arange(1, n + 1)
        next_id = n + 1
        t0 = int(rng.integers(1_500_000_000_000_000, 1_600_000_000_000_000))
        t = t0
        for f in range(num_frames):
            t += int(rng.integers(400_000, 600_000)) if f else 0
            s = int(sample_of[sc * num_frames + f])
            scene[s], ts[s] = 1000 + sc, t
            ego[s] = [centre[0] + 0.5 * f, centre[1] - 0.3 * f, 1.0]
            pr, gr = [], []
            if f not in empty_frames:
                sec = (t - t0) * 1e-6
                for o in range(n):
                    if not first[o] <= f < last[o]:
                        continue
                    c = p0[o] + v[o] * sec
                    gr.append([c[0], c[1], rng.normal(0, 1), oc[o], sc * 100000 + o, int(rng.random() > 0.05) * 7,
                               rng.random() > 0.04])
                    if rng.random() < switch:
                        tid[o], next_id = next_id, next_id + 1
                    if rng.random() < miss:
                        continue
                    d = c + rng.normal(0.0, noise, 2)
                    pr.append([d[0], d[1], rng.normal(0, 1), *rng.uniform(0.5, 4.0, 3), rng.uniform(-3, 3),
                               *(v[o] + rng.normal(0.0, 0.3, 2)), rng.uniform(0.3, 1.0), oc[o], tid[o]])
                for _ in range(false_pos):
                    pr.append([*(rng.uniform(-spread, spread, 2) + centre), 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0,
                               rng.uniform(0.05, 0.6), rng.choice(np.asarray(classes)), next_id])
                    next_id += 1
                for c in extra_classes:
                    pr.append([*(rng.uniform(-spread, spread, 2) + centre), 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0,
                               rng.uniform(0.05, 1.0), c, 0])
                    gr.append([*(rng.uniform(-spread, spread, 2) + centre), 0.0, c, sc * 100000 + 90000 + len(gr), 5, True])
                pr = [pr[i] for i in rng.permutation(len(pr))]
                gr = [gr[i] for i in rng.permutation(len(gr))]
            prow[s] = np.array(pr, np.float64).reshape(-1, 12)
            grow[s] = np.array(gr, np.float64).reshape(-1, 7)
    order = rng.permutation(S) if shuffle_samples else np.arange(S)       # the order the prediction rows are stored in
    row_start, row_count = np.zeros(S, np.int64), np.array([len(r) for r in prow], np.int64)
    at = 0
    for s in order:
        row_start[s] = at
        at += row_count[s]
    pall = np.concatenate([prow[s] for s in order]) if at else np.zeros((0, 12))
    gall = np.concatenate(grow)
    gt_off = np.zeros(S + 1, np.int64)
    np.cumsum([len(g) for g in grow], out=gt_off[1:])
    return {"rec": np.ascontiguousarray(pall[:, :10]), "cls": pall[:, 10].astype(np.int32), "track_id": pall[:, 11].astype(np.int32),
            "row_start": row_start, "row_count": row_count, "scene": scene, "timestamp_us": ts, "ego": ego,
            "gt_xyz": np.ascontiguousarray(gall[:, :3]), "gt_cls": gall[:, 3].astype(np.int32),
            "gt_instance": gall[:, 4].astype(np.int64), "gt_num_pts": gall[:, 5].astype(np.int32),
            "gt_keep": gall[:, 6].astype(bool), "gt_sample": np.repeat(np.arange(S), np.diff(gt_off)), "gt_off": gt_off}
