"""Hand-built scenes for the track-interpolation tests, in the frame notation of tests/track_metric_cases.py: a
frame is (objects [(instance, x, y)], hypotheses [(track id, x, y, score)]).  `build` returns the keyword arguments of
tests/track_interp_reference.interpolate_reference (tests/track_metric_cases.build's, with sizes, yaw and velocity that vary)."""
import numpy as np

import track_metric_cases as H

ARGS = ("rec", "cls", "track_id", "row_start", "row_count", "gt_xyz", "gt_cls", "gt_instance", "gt_num_pts", "gt_keep", "gt_off",
        "ego", "scene", "timestamp_us")


def build(frames, timestamps=None, **kw):
    d = H.build(frames, **kw)
    n = len(d["rec"])
    rng = np.random.default_rng(n)
    d["rec"][:, 2] = rng.normal(0.0, 1.0, n)
    d["rec"][:, 3:6] = rng.uniform(0.5, 4.0, (n, 3))
    d["rec"][:, 6] = rng.uniform(-3.0, 3.0, n)
    d["rec"][:, 7:9] = rng.normal(0.0, 3.0, (n, 2))
    d["gt_xyz"][:, 2] = rng.normal(0.0, 1.0, len(d["gt_xyz"]))
    if timestamps is not None:
        d["timestamp_us"] = np.asarray(timestamps, np.int64)
    d.pop("recall")
    return d


def track(present, tid=1, inst=1, x0=3.0, score=0.5):
    """One object and one hypothesis that follows it, each present in the frames whose flag is set: (gt flags, pred flags)."""
    gt, pr = present
    return [([(inst, x0 + 1.7 * f, 2.0 - 0.3 * f)] if gt[f] else [],
             [(tid, x0 + 1.7 * f + 0.2, 2.1 - 0.3 * f, score + 0.03 * f)] if pr[f] else []) for f in range(len(gt))]


def merge(*cases):
    """Frame-wise union of cases of equal length."""
    return [(sum((c[f][0] for c in cases), []), sum((c[f][1] for c in cases), [])) for f in range(len(cases[0]))]


ON = lambda n, off=(): [f not in off for f in range(n)]
UNEVEN_TS = [0, 400_000, 1_000_003, 1_450_000, 2_100_000, 2_500_001, 3_000_000, 3_700_000, 4_100_000, 4_600_000]
HAND = {
    "one_track_three_frames": dict(frames=track((ON(3, (1,)), ON(3, (1,))))),
    "holes_1_2_6": dict(frames=merge(track((ON(10, (1,)), ON(10, (2,))), 1, 1),
                                     track((ON(10, (4, 5)), ON(10, (5, 6))), 2, 2, x0=-9.0),
                                     track((ON(10, (1, 2, 3, 4, 5, 6)), ON(10, (2, 3, 4, 5, 6, 7))), 3, 3, x0=12.0)),
                        timestamps=UNEVEN_TS),
    "hole_across_empty_frame": dict(frames=[f if i != 2 else ([], []) for i, f in enumerate(merge(
        track((ON(5), ON(5)), 1, 1), track((ON(5, (1,)), ON(5, (3,))), 2, 2, x0=-4.0)))]),
    "first_or_last_only": dict(frames=merge(track(([True, False, False, False], [True, False, False, False]), 1, 1),
                                            track(([False, False, False, True], [False, False, False, True]), 2, 2, x0=-5.0),
                                            track((ON(4), ON(4)), 3, 3, x0=9.0))),
    "order": dict(frames=merge(track((ON(4, (1, 2)), ON(4, (1, 2))), 9, 50, x0=1.0),
                               track((ON(4, (2,)), ON(4, (1,))), 4, 20, x0=-6.0),
                               track((ON(4, (1,)), ON(4, (2,))), 7, 30, x0=14.0),
                               track((ON(4), ON(4)), 2, 40, x0=-15.0)), timestamps=UNEVEN_TS[:4]),
}
