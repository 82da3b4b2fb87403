"""float64 Python restatement of the track interpolation of DESIGN §2.25 (include/unidistill_hip.h, `ud_track_interp_count`): the
devkit's linear interpolation of every predicted and every ground-truth track across the frames that miss it, after the filters and
before the metric.  Plain loops over Python floats: `(1.0 - w) * a + w * b` is a rounded difference, two rounded products and a
rounded sum, the yaw uses `math.remainder`.  `evaluate_interpolated_reference` filters, interpolates and then runs
tests/track_metric_reference.evaluate_reference with its filters neutralised.  Nothing here imports the package under test."""
import math

import numpy as np

import track_metric_reference as R

ST_NONFINITE, ST_BOXES, ST_RANGE, ST_KEY, ST_DUPLICATE = 1, 2, 4, 8, 16
TWO_PI = 2.0 * math.pi


def scene_keys_reference(gt_instance, gt_sample, scene):
    """-> the GT track key per row: the rank of the instance id among the instance ids of its scene, ascending."""
    inst = [int(v) for v in gt_instance]
    sc = [int(scene[int(s)]) for s in gt_sample]
    ranks = {}
    for k in set(sc):
        ranks[k] = {v: i for i, v in enumerate(sorted({inst[g] for g in range(len(inst)) if sc[g] == k}))}
    return np.array([ranks[sc[g]][inst[g]] for g in range(len(inst))], np.int32)


def row_kept(candidate, c, vals, ego, tracked, class_range):
    """Section ROWS of the metric for one row -> (kept, non-finite)."""
    if not candidate or not (0 <= c < len(tracked)) or not tracked[c]:
        return False, False
    if not all(math.isfinite(float(v)) for v in vals):
        return False, True
    dx, dy = float(vals[0]) - float(ego[0]), float(vals[1]) - float(ego[1])
    return math.sqrt(dx * dx + dy * dy) <= class_range[c], False


def interp_weight(tL, tf, tR, mode):
    tL, tf, tR = int(tL), int(tf), int(tR)
    if mode == "devkit":
        return float(tR - tf) / float(tR - tL)
    if mode == "linear":
        return float(tf - tL) / float(tR - tL)
    raise ValueError(f"mode {mode!r}")


def interp_row(a, b, w, yaw_col=None):
    out = []
    for i, (x, y) in enumerate(zip((float(v) for v in a), (float(v) for v in b))):
        if i == yaw_col:
            d = math.remainder(y - x, TWO_PI)
            p = w * d
            out.append(x + p)
        else:
            omw = 1.0 - w
            p, q = omw * x, w * y
            out.append(p + q)
    return out


def interpolate_side(vals, cls, key, kept, starts, counts, frames_of_scene, ts, mode, yaw_col):
    """One side.  vals [n, cols], cls / key / kept per row, starts / counts per sample, frames_of_scene: the samples of every
    scene in time order.  -> dict vals, cls, key, src_row, start, count (per sample, samples in index order), num_interpolated,
    holes (the length of every hole).  Raises ValueError on a key that occurs twice in a frame."""
    S = len(starts)
    per_sample = [[] for _ in range(S)]             # (key or -1 for an original, src_row, values, cls)
    extra = [[] for _ in range(S)]
    holes = []
    for frames in frames_of_scene:
        last = {}                                   # key -> (frame index, row)
        for f, s in enumerate(frames):
            seen = set()
            for row in range(int(starts[s]), int(starts[s]) + int(counts[s])):
                if not kept[row]:
                    continue
                k = int(key[row])
                if k in seen:
                    raise ValueError(f"key {k} appears twice in sample {s}")
                seen.add(k)
                per_sample[s].append((row, [float(v) for v in vals[row]], int(cls[row]), k))
                if k in last and f - last[k][0] > 1:
                    pf, pr = last[k]
                    holes.append(f - pf - 1)
                    for g in range(pf + 1, f):
                        w = interp_weight(ts[frames[pf]], ts[frames[g]], ts[s], mode)
                        extra[frames[g]].append((k, interp_row(vals[pr], vals[row], w, yaw_col), int(cls[row])))
                last[k] = (f, row)
    out_vals, out_cls, out_key, out_src, count = [], [], [], [], np.zeros(S, np.int64)
    for s in range(S):
        for row, v, c, k in per_sample[s]:
            out_vals.append(v), out_cls.append(c), out_key.append(k), out_src.append(row)
        for k, v, c in sorted(extra[s], key=lambda e: e[0]):
            out_vals.append(v), out_cls.append(c), out_key.append(k), out_src.append(-1)
        count[s] = len(per_sample[s]) + len(extra[s])
    cols = np.asarray(vals).shape[1]
    return {"vals": np.array(out_vals, np.float64).reshape(-1, cols), "cls": np.array(out_cls, np.int32),
            "key": np.array(out_key, np.int32), "src_row": np.array(out_src, np.int32), "start": np.cumsum(count) - count,
            "count": count, "num_interpolated": int(sum(len(e) for e in extra)), "holes": holes}


def interpolate_reference(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_instance, gt_num_pts, gt_keep, gt_off, ego,
                          scene, timestamp_us, *, tracked, class_range, mode="devkit", max_boxes_per_sample=500):
    """-> {"pred": side, "gt": side, "status"}; the argument order is tests/track_metric_reference.evaluate_reference's.  Raises
    ValueError where two frames of a scene share a timestamp or a key occurs twice in a frame."""
    rec = np.asarray(rec, np.float64).reshape(-1, 10)
    gt_xyz = np.asarray(gt_xyz, np.float64).reshape(-1, 3)
    ego = np.asarray(ego, np.float64).reshape(-1, 3)
    S = len(ego)
    ts = [int(t) for t in timestamp_us]
    frame_sample, scene_off = R.scene_frames_reference(scene, timestamp_us)
    frames_of_scene = [frame_sample[scene_off[k]:scene_off[k + 1]] for k in range(len(scene_off) - 1)]
    for frames in frames_of_scene:
        for a, b in zip(frames, frames[1:]):
            if ts[a] == ts[b]:
                raise ValueError(f"samples {a} and {b} of one scene have the same timestamp")
    max_id = max(sum(int(row_count[s]) for s in frames) for frames in frames_of_scene)
    gt_sample = np.repeat(np.arange(S), np.diff(np.asarray(gt_off, np.int64)))
    gkey = scene_keys_reference(gt_instance, gt_sample, scene)
    status = 0
    pkept = np.zeros(len(rec), bool)
    for s in range(S):
        n = 0
        for row in range(int(row_start[s]), int(row_start[s]) + int(row_count[s])):
            k, bad = row_kept(int(track_id[row]) > 0, int(cls[row]), rec[row], ego[s], tracked, class_range)
            status |= ST_NONFINITE if bad else 0
            if k and int(track_id[row]) > max_id:
                status |= ST_KEY
                k = False
            pkept[row] = k
            n += k
        if n > max_boxes_per_sample:
            status |= ST_BOXES
    gkept = np.zeros(len(gt_xyz), bool)
    for g in range(len(gt_xyz)):
        s = int(gt_sample[g])
        k, bad = row_kept(bool(gt_keep[g]) and int(gt_num_pts[g]) > 0, int(gt_cls[g]), gt_xyz[g], ego[s], tracked, class_range)
        status |= ST_NONFINITE if bad else 0
        gkept[g] = k
    pred = interpolate_side(rec, cls, track_id, pkept, row_start, row_count, frames_of_scene, ts, mode, 6)
    gt = interpolate_side(gt_xyz, gt_cls, gkey, gkept, np.asarray(gt_off)[:-1], np.diff(np.asarray(gt_off, np.int64)),
                          frames_of_scene, ts, mode, None)
    return {"pred": pred, "gt": gt, "status": status}


def evaluate_interpolated_reference(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_instance, gt_num_pts, gt_keep,
                                    gt_off, ego, scene, timestamp_us, *, tracked, class_range, recall, mode="devkit", dist_th_tp=2.0,
                                    max_boxes_per_sample=500, events_pass=None):
    """Filter, interpolate, then the metric's reference on the new rows with nothing filtered a second time: every GT row kept
    with one point, an infinite range for the tracked classes, max_boxes_per_sample raised to the fullest new sample.  The track
    ids are renumbered per scene in order of appearance -- the metric only compares ids, and its reference bounds them by the
    scene's (now smaller) row count.  -> (evaluate_reference's dict, interpolate_reference's dict)."""
    it = interpolate_reference(rec, cls, track_id, row_start, row_count, gt_xyz, gt_cls, gt_instance, gt_num_pts, gt_keep, gt_off,
                               ego, scene, timestamp_us, tracked=tracked, class_range=class_range, mode=mode,
                               max_boxes_per_sample=max_boxes_per_sample)
    p, g = it["pred"], it["gt"]
    frame_sample, scene_off = R.scene_frames_reference(scene, timestamp_us)
    ids = np.zeros(len(p["key"]), np.int32)
    for k in range(len(scene_off) - 1):
        names = {}
        for s in frame_sample[scene_off[k]:scene_off[k + 1]]:
            for row in range(int(p["start"][s]), int(p["start"][s]) + int(p["count"][s])):
                ids[row] = names.setdefault(int(p["key"][row]), len(names) + 1)
    G = len(g["key"])
    wide = [float("inf") if t else float(r) for t, r in zip(tracked, class_range)]
    off = np.concatenate([[0], np.cumsum(g["count"])]).astype(np.int64)
    out = R.evaluate_reference(p["vals"], p["cls"], ids, p["start"], p["count"], g["vals"], g["cls"], g["key"], np.ones(G, np.int32),
                               np.ones(G, bool), off, ego, scene, timestamp_us, tracked=tracked, class_range=wide, recall=recall,
                               dist_th_tp=dist_th_tp, max_boxes_per_sample=max(int(max_boxes_per_sample), int(p["count"].max())),
                               events_pass=events_pass)
    return out, it
