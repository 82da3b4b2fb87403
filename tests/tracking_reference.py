"""numpy float64 restatement of the tracker of DESIGN §2.23 (include/unidistill_hip.h, `ud_track_scenes`), in plain Python
loops, and the seeded scene generators the tracking tests and tools/time_tracking.py share.

Every float64 operation is written as its own rounded step, in the order the text gives: `ct = ct + v * dt`,
`d2 = dx * dx + dy * dy`, `d2 <= max_dist * max_dist`; there is no square root.  Python floats are IEEE doubles and the
interpreter never fuses a multiply with an add."""
import numpy as np

ST_NONFINITE = 1
TRACKING_CLASSES = ("bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck")
MAX_DIST = {"car": 4.0, "truck": 4.0, "bus": 5.5, "trailer": 3.0, "pedestrian": 1.0, "motorcycle": 13.0, "bicycle": 3.0}
CLASS_NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
               "traffic_cone"]


def default_config(class_names=CLASS_NAMES):
    return [n in TRACKING_CLASSES for n in class_names], [MAX_DIST.get(n, 0.0) for n in class_names]


def scene_frames_reference(scene, timestamp_us):
    """-> (frame_sample, scene_off, frame_dt): samples grouped by ascending scene value, ordered by (timestamp, index)."""
    scene = [int(s) for s in scene]
    ts = [int(t) for t in timestamp_us]
    frame_sample, scene_off, frame_dt = [], [0], []
    for sc in sorted(set(scene)):
        members = sorted((ts[i], i) for i in range(len(scene)) if scene[i] == sc)
        for k, (t, i) in enumerate(members):
            frame_sample.append(i)
            frame_dt.append(0.0 if k == 0 else float(np.float64(t - members[k - 1][0]) * np.float64(1e-6)))
        scene_off.append(len(frame_sample))
    return np.array(frame_sample, np.int64), np.array(scene_off, np.int64), np.array(frame_dt, np.float64)


def track_reference(rec, cls, row_start, row_count, frame_sample, scene_off, frame_dt, track_class, max_dist, max_age=3,
                    score_threshold=0.0, stats=None):
    """-> (track_id int32 [P], track_hits int32 [P], status).  `stats` (a dict, optional) receives "peak_live": the longest
    track list any frame left behind."""
    rec = np.asarray(rec, dtype=np.float64)
    P = len(rec)
    track_id = np.zeros(P, np.int32)
    track_hits = np.zeros(P, np.int32)
    status = 0
    C = len(track_class)
    for sc in range(len(scene_off) - 1):
        tracks = []                         # dicts: ct [x, y], v [x, y], cls, id, age, hits
        next_id = 0
        for fi in range(int(scene_off[sc]), int(scene_off[sc + 1])):
            sample = int(frame_sample[fi])
            dt = float(frame_dt[fi])
            cands = []
            for row in range(int(row_start[sample]), int(row_start[sample]) + int(row_count[sample])):
                c = int(cls[row])
                if not (0 <= c < C and track_class[c]):
                    continue
                vals = [float(rec[row, k]) for k in (0, 1, 2, 7, 8, 9)]
                if not all(np.isfinite(v) for v in vals):
                    status |= ST_NONFINITE
                    continue
                if float(rec[row, 9]) >= score_threshold:
                    cands.append(row)
            cands.sort(key=lambda r: (-float(rec[r, 9]), r))
            for t in tracks:
                t["ct"][0] = t["ct"][0] + t["v"][0] * dt
                t["ct"][1] = t["ct"][1] + t["v"][1] * dt
            claimed = [False] * len(tracks)
            new = []
            for row in cands:
                c = int(cls[row])
                cx, cy = float(rec[row, 0]), float(rec[row, 1])
                best, best_slot = float("inf"), -1
                for slot, t in enumerate(tracks):
                    if claimed[slot] or t["cls"] != c:
                        continue
                    dx = cx - t["ct"][0]
                    dy = cy - t["ct"][1]
                    d2 = dx * dx + dy * dy
                    if d2 < best:
                        best, best_slot = d2, slot
                md = float(max_dist[c])
                entry = {"ct": [cx, cy], "v": [float(rec[row, 7]), float(rec[row, 8])], "cls": c, "age": 0}
                if best_slot >= 0 and best <= md * md:
                    claimed[best_slot] = True
                    old = tracks[best_slot]
                    entry["id"] = old["id"]
                    entry["hits"] = old["hits"] + 1 if old["age"] == 0 else 1
                else:
                    next_id += 1
                    entry["id"] = next_id
                    entry["hits"] = 1
                new.append(entry)
                track_id[row] = entry["id"]
                track_hits[row] = entry["hits"]
            for slot, t in enumerate(tracks):
                if not claimed[slot] and t["age"] + 1 < max_age:
                    t["age"] += 1
                    new.append(t)
            tracks = new
            if stats is not None:
                stats["peak_live"] = max(stats.get("peak_live", 0), len(tracks))
    return track_id, track_hits, status


def live_tracks_peak(rec, cls, row_start, row_count, frame_sample, scene_off, frame_dt, track_class, max_dist, max_age=3,
                     score_threshold=0.0):
    """The largest number of candidates of one frame and an upper bound of the live tracks of one scene (the candidates of
    max_age consecutive frames), for the generators' cap checks."""
    C = len(track_class)
    peak_c = peak_t = 0
    for sc in range(len(scene_off) - 1):
        counts = []
        for fi in range(int(scene_off[sc]), int(scene_off[sc + 1])):
            s = int(frame_sample[fi])
            rows = range(int(row_start[s]), int(row_start[s]) + int(row_count[s]))
            counts.append(sum(1 for r in rows if 0 <= cls[r] < C and track_class[cls[r]] and rec[r, 9] >= score_threshold))
            peak_c = max(peak_c, counts[-1])
            peak_t = max(peak_t, sum(counts[-max_age:]))
    return peak_c, peak_t


def make_scenes(seed, num_scenes, num_frames, num_objects, classes, *, empty_frames=(), spread=60.0, shuffle_samples=False,
                extra_classes=(), alternate=False, score_levels=0):
    """Seeded scenes in the evaluator's layout.  Each scene holds `num_objects` objects of the given classes that move at constant
    velocity, appear at a random frame, vanish for 1 to 4 frames now and then, and are detected with centre noise, a noisy
    velocity and a random score; `extra_classes` adds as many rows of classes that are not tracked.  `empty_frames`: frame
    numbers without rows.  `alternate`: odd frames hold a disjoint second set of objects far away (live tracks beyond one frame's
    count).  `shuffle_samples`: the sample order, and so row_start, is shuffled.  `score_levels` > 0: every score is one of that many
    values k / levels, so equal scores abound within a class and across classes.
    -> dict rec f64 [P, 10], cls i32 [P], row_start, row_count, scene, timestamp_us (per sample)."""
    rng = np.random.default_rng(seed)
    S = num_scenes * num_frames
    sample_of = rng.permutation(S) if shuffle_samples else np.arange(S)       # (scene, frame) -> sample index
    scene = np.zeros(S, np.int64)
    ts = np.zeros(S, np.int64)
    rows_of = [None] * S
    for sc in range(num_scenes):
        n = num_objects
        oc = rng.choice(np.asarray(classes), n)
        p0 = rng.uniform(-spread, spread, (n, 2))
        v = rng.normal(0.0, 3.0, (n, 2))
        first = rng.integers(0, max(1, num_frames // 3), n)
        if num_frames <= 2:
            first[:] = 0
        gone = np.zeros(n, np.int64)
        t0 = int(rng.integers(1_500_000_000_000_000, 1_600_000_000_000_000))
        t = t0
        for f in range(num_frames):
            t += int(rng.integers(400_000, 600_000)) if f else 0
            s = int(sample_of[sc * num_frames + f])
            scene[s], ts[s] = 1000 + sc, t
            rows = []
            if f not in empty_frames:
                sec = (t - t0) * 1e-6
                for o in range(n):
                    if f < first[o]:
                        continue
                    if gone[o] > 0:
                        gone[o] -= 1
                        continue
                    if num_frames > 2 and rng.random() < 0.08:
                        gone[o] = int(rng.integers(1, 5)) - 1
                        continue
                    off = 500.0 if (alternate and f % 2) else 0.0
                    c = p0[o] + v[o] * sec + rng.normal(0.0, 0.15, 2) + off
                    rows.append([c[0], c[1], rng.normal(0, 1), *rng.uniform(0.5, 4.0, 3), rng.uniform(-3, 3),
                                 *(v[o] + rng.normal(0.0, 0.3, 2)), rng.uniform(0.05, 1.0), oc[o]])
                for c in extra_classes:
                    rows.append([*rng.uniform(-spread, spread, 2), 0.0, 1.0, 1.0, 1.0, 0.0, np.nan, np.nan,
                                 rng.uniform(0.05, 1.0), c])
                rows = [rows[i] for i in rng.permutation(len(rows))]
                if score_levels:
                    for r in rows:
                        r[9] = float(rng.integers(1, score_levels + 1)) / score_levels
            rows_of[s] = np.array(rows, np.float64).reshape(-1, 11)
    order = rng.permutation(S) if shuffle_samples else np.arange(S)            # the order the rows are stored in
    row_start = np.zeros(S, np.int64)
    row_count = np.array([len(r) for r in rows_of], np.int64)
    at = 0
    for s in order:
        row_start[s] = at
        at += row_count[s]
    allrows = np.concatenate([rows_of[s] for s in order]) if at else np.zeros((0, 11))
    return {"rec": np.ascontiguousarray(allrows[:, :10]), "cls": allrows[:, 10].astype(np.int32), "row_start": row_start,
            "row_count": row_count, "scene": scene, "timestamp_us": ts}
