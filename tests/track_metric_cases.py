"""Hand-built scenes for the tracking-metric tests: each case is a list of frames of one scene, a frame is
(objects [(instance, x, y)], hypotheses [(track id, x, y, score)]), everything of class car (0) unless a fifth / fourth entry
names the class.  `build` turns a case into the keyword arguments of tests/track_metric_reference.evaluate_reference."""
import numpy as np

import track_metric_reference as R

BELOW_2 = float(np.nextafter(2.0, 0.0))


def build(frames, ego=(0.0, 0.0), num_pts=None, keep=None):
    S = len(frames)
    rec, cls, tid, gt, gcls, ginst = [], [], [], [], [], []
    row_start, row_count, gt_off = [], [], [0]
    for objs, hyps in frames:
        row_start.append(len(rec))
        row_count.append(len(hyps))
        for h in hyps:
            rec.append([h[1], h[2], 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, h[3]])
            tid.append(h[0])
            cls.append(h[4] if len(h) > 4 else 0)
        for o in objs:
            gt.append([o[1], o[2], 0.0])
            ginst.append(o[0])
            gcls.append(o[3] if len(o) > 3 else 0)
        gt_off.append(len(gt))
    G = len(gt)
    tracked, rng = R.default_config()
    return dict(rec=np.array(rec, np.float64).reshape(-1, 10), cls=np.array(cls, np.int32), track_id=np.array(tid, np.int32),
                row_start=np.array(row_start, np.int64), row_count=np.array(row_count, np.int64),
                gt_xyz=np.array(gt, np.float64).reshape(-1, 3), gt_cls=np.array(gcls, np.int32),
                gt_instance=np.array(ginst, np.int64),
                gt_num_pts=np.array([5] * G if num_pts is None else num_pts, np.int32),
                gt_keep=np.array([True] * G if keep is None else keep, bool), gt_off=np.array(gt_off, np.int64),
                ego=np.tile(np.array([ego[0], ego[1], 0.0]), (S, 1)), scene=np.full(S, 7, np.int64),
                timestamp_us=np.arange(S, dtype=np.int64) * 500_000, tracked=tracked, class_range=rng,
                recall=R.recall_thresholds())


def run(frames, events_pass="none", **kw):
    a = build(frames, **kw)
    pos = [a.pop(k) for k in ("rec", "cls", "track_id", "row_start", "row_count", "gt_xyz", "gt_cls", "gt_instance",
                              "gt_num_pts", "gt_keep", "gt_off", "ego", "scene", "timestamp_us")]
    return R.evaluate_reference(*pos, events_pass=events_pass, **a)


OFFSET = 0.25
PERFECT = [([(1, 10.0 + f, 5.0)], [(1, 10.0 + f + OFFSET, 5.0, 0.9)]) for f in range(6)]
ID_SWAP = [([(1, 0.0, 0.0), (2, 10.0, 0.0)], [(1, 0.1, 0.0, 0.9), (2, 10.1, 0.0, 0.9)]) for _ in range(3)] + \
          [([(1, 0.0, 0.0), (2, 10.0, 0.0)], [(2, 0.1, 0.0, 0.9), (1, 10.1, 0.0, 0.9)]) for _ in range(3)]
MISSED_SAME_ID = [([(1, 0.0, 0.0)], [(4, 0.1, 0.0, 0.9)] if f not in (2, 3) else []) for f in range(6)]
MISSED_NEW_ID = [([(1, 0.0, 0.0)], [] if f in (2, 3) else [(1 if f < 2 else 2, 0.1, 0.0, 0.9)]) for f in range(6)]
# frame 1: the hypothesis with the previous id (1.5 m) wins over a closer new one (0.2 m)
REESTABLISH = [([(1, 0.0, 0.0)], [(1, 0.3, 0.0, 0.9)]),
               ([(1, 0.0, 0.0)], [(2, 0.2, 0.0, 0.9), (1, 1.5, 0.0, 0.8)])]
# o1-h1 0.1, o1-h2 1.9, o2-h1 1.9, o2-h2 inadmissible: two matches (o1-h2, o2-h1), not the cheap one
CARDINALITY = [([(1, 0.0, 0.0), (2, 2.0, 0.0)], [(1, 0.1, 0.0, 0.9), (2, -1.9, 0.0, 0.8)])]
AT_THRESHOLD = [([(1, 0.0, 0.0), (2, 30.0, 0.0)], [(1, 2.0, 0.0, 0.9), (2, 30.0, BELOW_2, 0.8)])]
# frame 0: object 1 <- id 1; frame 1: only object 2 <- id 1; frame 2: both present, one hypothesis of id 1 admissible to both: row
# order lets object 1 claim it, object 2 (whose m is 1 too) finds it claimed and is a MISS.  Ids stay within the scene's row count.
CLAIMED = [([(1, 0.0, 0.0)], [(1, 0.1, 0.0, 0.9)]),
           ([(2, 1.0, 0.0)], [(1, 0.9, 0.0, 0.9)]),
           ([(1, 0.0, 0.0), (2, 1.0, 0.0)], [(1, 0.8, 0.0, 0.9)])]
HAND_CASES = {"perfect": PERFECT, "id_swap": ID_SWAP, "missed_same_id": MISSED_SAME_ID, "missed_new_id": MISSED_NEW_ID,
              "reestablish": REESTABLISH, "cardinality": CARDINALITY, "at_threshold": AT_THRESHOLD, "claimed": CLAIMED}
