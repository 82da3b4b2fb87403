"""The track interpolation (ops.track_metric.interpolate_tracks, csrc/track_interp.hip) at validation size: the case
of tools/time_track_metric.py -- 150 scenes x 40 frames, about 200 tracked candidates per frame over the 7 tracking classes, the ids
from the device tracker.  Prints one JSON line: `device_ms` -- HIP events around `interpolate_tracks` alone (both calls and the
read of the counts between them), warmed, median of the repeats with min and max --, the whole metric with and without
interpolation (`evaluate_tracks_interpolated` / `evaluate_tracks`, timed the same way), `reference_ms` -- the float64 reference of
tests/track_interp_reference.py on this machine's CPU for the first `--ref-scenes` scenes, scaled by scenes -- and the interpolated
row counts of both sides.  The device's integer outputs on the reference's scenes must equal the reference's.
Run it under a time limit:  timeout -k 10 500 python tools/time_track_interp.py"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cvpr2023-unidistill_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import track_interp_reference as I
import track_metric_reference as R
from unidistill_amd.ops import track_metric as M
from unidistill_amd.ops import tracking as T

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=150)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--objects", type=int, default=285)
ap.add_argument("--ref-scenes", type=int, default=2)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--mode", default="devkit")
args = ap.parse_args()
assert torch.cuda.is_available(), "time_track_interp.py measures on the GPU only"
dev = torch.device("cuda:0")
tracked, rng = R.default_config()
classes = [c for c, on in enumerate(tracked) if on]
MAX_DIST = {"car": 4.0, "truck": 4.0, "bus": 5.5, "trailer": 3.0, "pedestrian": 1.0, "motorcycle": 13.0, "bicycle": 3.0}
recall = R.recall_thresholds()


def case(num_scenes):
    d = R.make_case(0, num_scenes=num_scenes, num_frames=args.frames, num_objects=args.objects, classes=classes, spread=80.0,
                    extra_classes=(2, 5, 9), false_pos=12)
    fs, off, dt = T.scene_frames(d["scene"], d["timestamp_us"])
    rec, cls = torch.from_numpy(d["rec"]).to(dev), torch.from_numpy(d["cls"]).to(dev)
    ids, _, status = T.track_scenes(rec, cls, d["row_start"], d["row_count"], fs, off, dt, track_class=tracked,
                                    max_dist=[MAX_DIST.get(n, 0.0) for n in R.CLASS_NAMES])
    assert int(status.item()) == 0
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a.astype(t))).to(dev)
    gt = (up(d["gt_xyz"], np.float64), up(d["gt_cls"], np.int32), up(d["gt_num_pts"], np.int32), up(d["gt_keep"], np.uint8))
    pos = (rec, cls, ids, d["row_start"], d["row_count"], *gt, d["gt_instance"], d["gt_off"], up(d["ego"], np.float64), d["scene"],
           d["timestamp_us"])
    kw = dict(track_class=tracked, class_range=rng)
    return d, ids, {"interp": lambda: M.interpolate_tracks(*pos, mode=args.mode, **kw),
                    "metric": lambda: M.evaluate_tracks(*pos, recall=recall, **kw),
                    "metric_interpolated": lambda: M.evaluate_tracks_interpolated(*pos, recall=recall, mode=args.mode, **kw)}


def timed(fn):
    for _ in range(2):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return out, {"median": round(float(np.median(times)), 3), "min": round(float(min(times)), 3), "max": round(float(max(times)), 3)}


d, ids, run = case(args.scenes)
it, t_interp = timed(run["interp"])
assert int(it["status"].item()) == 0
plain, t_plain = timed(run["metric"])
both, t_both = timed(run["metric_interpolated"])
assert int(plain["status"].item()) == 0 and int(both["status"].item()) == 0 and int(both["interp_status"].item()) == 0

n_ref = max(1, min(args.ref_scenes, args.scenes))
ds, ids_s, run_s = case(n_ref)
sub = run_s["interp"]()
t0 = time.perf_counter()
ref = I.interpolate_reference(ds["rec"], ds["cls"], ids_s.cpu().numpy(), ds["row_start"], ds["row_count"], ds["gt_xyz"], ds["gt_cls"],
                              ds["gt_instance"], ds["gt_num_pts"], ds["gt_keep"], ds["gt_off"], ds["ego"], ds["scene"],
                              ds["timestamp_us"], tracked=tracked, class_range=rng, mode=args.mode)
ref_s = time.perf_counter() - t0
equal = all(np.array_equal(sub[s]["count"], ref[s]["count"]) and np.array_equal(sub[s]["src_row"].cpu().numpy(), ref[s]["src_row"])
            and np.array_equal(sub[s]["key"].cpu().numpy(), ref[s]["key"]) for s in ("pred", "gt"))
equal = equal and sub["pred"]["rec"].cpu().numpy().tobytes() == ref["pred"]["vals"].tobytes() \
    and sub["gt"]["xyz"].cpu().numpy().tobytes() == ref["gt"]["vals"].tobytes()
assert equal, "the device rows differ from the reference"
print(json.dumps({"tool": "time_track_interp", "scenes": args.scenes, "frames": args.frames, "mode": args.mode,
                  "rows": int(len(d["rec"])), "gt_rows": int(len(d["gt_xyz"])),
                  "rows_out": int(it["pred"]["count"].sum()), "gt_rows_out": int(it["gt"]["count"].sum()),
                  "interpolated_pred": it["pred"]["num_interpolated"], "interpolated_gt": it["gt"]["num_interpolated"],
                  "device_ms": t_interp["median"], "device_ms_min": t_interp["min"], "device_ms_max": t_interp["max"],
                  "metric_ms": t_plain, "metric_interpolated_ms": t_both,
                  "reference_ms": round(ref_s * 1e3 * args.scenes / n_ref, 1), "reference_scenes_timed": n_ref,
                  "rows_equal_on_timed_scenes": bool(equal)}))
